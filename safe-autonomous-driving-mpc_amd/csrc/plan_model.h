// plan_model.h -- the planner's NLP model, stated once for its kernels (plan_kernel.h, plan_evaluate_kernel.h) and
// for its host backend (plan_host.h, plan_evaluate_host.h): the sizes and tuning constants of the solver, the row
// kinds and which stage has which, the route's curvature and speed limit, the dynamics with their derivatives, the
// Hermite-Simpson defect, the 3x3 factorisation, and the evaluator's per-stage step.  Both sides keep their own
// storage, loops, reductions and searches and hand single values in; the route comes as a view R with the members
// M, s, cx, cy, vmax and the two searches R.lower(v) (first i with s[i] >= v) and R.upper(v) (first i with
// s[i] > v), which each side answers its own way (binary on the host, from a grid cell on the device).
// What may be written here: single rounded FP64 operations, sqrt / sin / cos / floor / fabs, integer arithmetic
// and comparisons.  The build has -ffp-contract=off, so the device pass, the host pass and a plain C++ compiler
// form the same operation sequence; the results differ between device and host only where the device's sin / cos
// differ from libm's.  oracle/plan_oracle.c shares nothing with this file: it is the independent parity reference.
#pragma once
#include "../../include/mpcplan_evaluate.h"
#include <math.h>

#ifdef __HIPCC__
#define PLAN_MODEL __host__ __device__
#define PLAN_MODEL_INLINE __host__ __device__ __forceinline__
#define PLAN_UNROLL _Pragma("unroll")
#else
#define PLAN_MODEL
#define PLAN_MODEL_INLINE inline
#define PLAN_UNROLL
#endif

namespace plan_model {

constexpr int NZ = 8;                  // stage variables: x (s, d, o, k, v), w (u1, u2, S)
constexpr int NR = 11;                 // rows per stage at most
constexpr double RHO = 1e8;            // penalty of the active rows in the equality-constrained solve
constexpr int AL_STEPS = 4;            // refinement + multiplier updates of that solve
constexpr double AL_TOL = 1e-13;       // stop the refinements once the multiplier update is at rounding level
constexpr int POLISH_ROUNDS = 6;
constexpr int WARM_ROUNDS = 5;         // active-set rounds from the previous QP's classification before the interior point
constexpr double MU_CHECK = 1e-4;      // interior-point checkpoint: a polish is tried once mu and phi are below this ...
constexpr double CHECK_SEP = 100.0;    // ... and every row's s and lambda differ by this factor (no near-tie to classify)
constexpr int CHECK_ROUNDS = 2;        // polish rounds at the checkpoint (the interior point resumes if they fail)
constexpr double SHIFT0 = 1.0;         // interior-point start: s = max(row, 0) + SHIFT0, lambda = 1
constexpr double TAU = 0.995;
constexpr double CYCLE_REL = 1e-6;
constexpr double DELTA0 = 1e-6;        // first Hessian regularisation when a pivot fails; x10 per retry
constexpr double DELTA_MAX = 1e4;
constexpr double EXACT_STEP = 0.1;     // exact Lagrangian Hessian once the last SQP step is at most this (max norm) ...
constexpr int EXACT_AFTER = 20;        // ... or from this SQP iteration on (a Gauss-Newton SQP can zigzag with steps of
                                       // ~0.2 around an active lateral-acceleration row without ever meeting EXACT_STEP)
constexpr double LS_ARMIJO = 1e-4;     // line search on the L1 merit f + mu * violation: sufficient decrease
constexpr int LS_STEPS = 12;           // halvings at most (the last one is taken regardless)
constexpr double LS_FULL = 1e-3;       // steps at most this long (max norm) are taken whole (local phase)
constexpr int LS_MEMORY = 4;           // non-monotone line search: decrease against the largest of the last merits

// ------------------------------------------------------------------------------------------------------
// the rows of a stage
// ------------------------------------------------------------------------------------------------------
enum { ROW_VMIN, ROW_VMAX, ROW_LATP, ROW_LATM, ROW_KMIN, ROW_KMAX, ROW_U1MIN, ROW_U1MAX, ROW_U2MIN, ROW_U2MAX,
       ROW_S, ROW_STERM };

// the rows of stage k, in order: [v_min, v_max, (k > 0) lateral +, lateral -] unless the final chunk's last
// stage; (k > 0) curvature min, max; (k < N) u1 min, max, u2 min, max, slack; the intermediate chunk's
// terminal row at k = N (trajectory_planning.py:238-349).  Counted and indexed arithmetically (no per-lane
// array, which would live in scratch memory).
PLAN_MODEL constexpr bool row_on(int kind, int k, int N, int fin) {
    switch (kind) {
        case ROW_VMIN: case ROW_VMAX: return !(fin && k == N);
        case ROW_LATP: case ROW_LATM: return !(fin && k == N) && k > 0;
        case ROW_KMIN: case ROW_KMAX: return k > 0;
        case ROW_STERM: return k == N && !fin;
        default: return k < N;
    }
}
PLAN_MODEL constexpr int stage_nrows(int k, int N, int fin) {
    return ((fin && k == N) ? 0 : (k > 0 ? 4 : 2)) + (k > 0 ? 2 : 0) + (k < N ? 5 : 0) + ((k == N && !fin) ? 1 : 0);
}
PLAN_MODEL constexpr int row_kind(int k, int N, int fin, int j) {
    const int n0 = (fin && k == N) ? 0 : (k > 0 ? 4 : 2);
    if (j < n0) return j;                                   // ROW_VMIN, ROW_VMAX, ROW_LATP, ROW_LATM
    j -= n0;
    const int n1 = k > 0 ? 2 : 0;
    if (j < n1) return ROW_KMIN + j;
    j -= n1;
    if (k < N) return ROW_U1MIN + j;                        // ROW_U1MIN .. ROW_S
    return ROW_STERM;
}
// the storage slot of a row kind: its own, except the intermediate chunk's terminal row (k = N only), which takes
// the u1-min slot (no stage has both), so a stage's rows fit in NR slots in row order
PLAN_MODEL constexpr int kind_slot(int kind) { return kind == ROW_STERM ? ROW_U1MIN : kind; }

// ------------------------------------------------------------------------------------------------------
// route: k_ref_fun and v_max_fun of optimize_full_trajectory (trajectory_planning.py:437-477)
// ------------------------------------------------------------------------------------------------------
// k_ref_fun (:445-459): t = s_to_t(s) (interp1d linear, extrapolated, :440-442: searchsorted left, index clipped
// to [1, M-1]); curvature of the CubicSpline pair at t (PPoly: interval floor(t) clipped to [0, M-2]); first and
// second derivatives in s on the same pieces (t is linear in s there).  k1, or k2 alone, may be null
template <class R>
PLAN_MODEL static double route_kappa(const R& rt, double s, double* k1, double* k2) {
    const int M = rt.M;
    int i = rt.lower(s);
    i = i < 1 ? 1 : (i > M - 1 ? M - 1 : i);
    const double slope = 1.0 / (rt.s[i] - rt.s[i - 1]);
    const double t = slope * (s - rt.s[i - 1]) + (double)(i - 1);
    int j = (int)floor(t);
    j = j < 0 ? 0 : (j > M - 2 ? M - 2 : j);
    const double tau = t - (double)j;
    const double* a = rt.cx + 4 * j;
    const double* b = rt.cy + 4 * j;
    const double x1 = (3.0 * a[0] * tau + 2.0 * a[1]) * tau + a[2], x2 = 6.0 * a[0] * tau + 2.0 * a[1], x3 = 6.0 * a[0];
    const double y1 = (3.0 * b[0] * tau + 2.0 * b[1]) * tau + b[2], y2 = 6.0 * b[0] * tau + 2.0 * b[1], y3 = 6.0 * b[0];
    const double num = x1 * y2 - y1 * x2;
    const double q = x1 * x1 + y1 * y1;
    const double sq = sqrt(q);
    double den = q * sq + 1e-9;
    const bool clamp = den < 1e-8;
    if (clamp) den = 1e-8;
    const double k = num / den;
    if (k1) {
        const double dnum = x1 * y3 - y1 * x3;
        const double dden = clamp ? 0.0 : 3.0 * sq * (x1 * x2 + y1 * y2);
        const double kt = (dnum - k * dden) / den;
        *k1 = kt * slope;
        if (k2) {
            // num'' = x2 y3 - y2 x3 (cubic pieces); den'' = 3/4 q^-1/2 q'^2 + 3/2 q^1/2 q''
            const double d2num = x2 * y3 - y2 * x3;
            const double qd = 2.0 * (x1 * x2 + y1 * y2), qdd = 2.0 * (x2 * x2 + x1 * x3 + y2 * y2 + y1 * y3);
            const double d2den = (clamp || sq == 0.0) ? 0.0 : 0.75 * qd * qd / sq + 1.5 * sq * qdd;
            *k2 = (d2num - 2.0 * kt * dden - k * d2den) / den * slope * slope;
        }
    }
    return k;
}

// v_max_fun (:470-473): interp1d kind='previous' (below the first knot: the first limit, see mpcplan.h)
template <class R>
PLAN_MODEL static double route_vmax(const R& rt, double s) {
    const int i = rt.upper(s);
    return rt.vmax[i > 0 ? i - 1 : 0];
}

// ------------------------------------------------------------------------------------------------------
// the NLP's functions (trajectory_planning.py:50-89, :181-210) and derivatives
// ------------------------------------------------------------------------------------------------------
PLAN_MODEL static double guard_den(double den) {       // :74-77
    if (fabs(den) < 1e-4) den = den > 0.0 ? 1e-4 : (den < 0.0 ? -1e-4 : 1e-4);
    return den;
}

// TrajectoryOptimizer.dynamics (:50-89)
PLAN_MODEL static void dyn(const double x[5], double u1, double u2, double kr, double f[5]) {
    const double den = guard_den(1.0 - x[1] * kr);
    const double sd = (x[4] * cos(x[2])) / den;
    f[0] = sd;
    f[1] = x[4] * sin(x[2]);
    f[2] = x[4] * x[3] - sd * kr;
    f[3] = u1;
    f[4] = u2;
}

// d f / d x with kappa = kappa(s), dk its derivative: F row-major 5x5 (d f / d u = e3, e4 for u1, u2)
PLAN_MODEL static void dyn_jac(const double x[5], double kr, double dk, double F[25]) {
    const double d = x[1], o = x[2], k = x[3], v = x[4];
    const double raw = 1.0 - d * kr;
    const bool g = fabs(raw) < 1e-4;
    const double den = guard_den(raw);
    const double c = cos(o), sn = sin(o);
    const double sd = v * c / den;
    double ds[5];
    ds[0] = g ? 0.0 : v * c * d * dk / (den * den);
    ds[1] = g ? 0.0 : v * c * kr / (den * den);
    ds[2] = -v * sn / den;
    ds[3] = 0.0;
    ds[4] = c / den;
    PLAN_UNROLL
    for (int i = 0; i < 25; ++i) F[i] = 0.0;
    PLAN_UNROLL
    for (int j = 0; j < 5; ++j) {
        F[j] = ds[j];
        F[10 + j] = -kr * ds[j];
    }
    F[7] = v * c;
    F[9] = sn;
    F[10] += -dk * sd;
    F[13] += v;
    F[14] += k;
}

// W = sum_i y_i d2 f_i / dx2 at x, kappa = kappa(s) with derivatives k1, k2 (f3, f4 are linear), in two forms that
// differ only in how s_dot's share is multiplied by cs = y[0] - y[2] kappa, and round differently for it:
//   hess_f_folded (the kernels): cs enters each entry's product first, cs * v * c * gss;
//   hess_f_scaled (the host backend): the finished entry v * c * gss is multiplied by cs, as oracle/plan_oracle.c
//   does, to which tests/test_plan_host.py holds the host bit for bit.
// Neither is the more accurate.  The device keeps its own because its recorded results and A/B measurements were
// taken with it; the two are to be unified only together with the oracle and those records.  Everything else in
// them is the same text and must stay so: g = 1 / (1 - d kappa(s)) and its derivatives (constant when guarded),
// s_dot = v cos(o) g with its gradient ds, then f1 = v sin(o), and f2 = v k - s_dot kappa(s): the v k term, and
// -(grad s_dot x grad kappa + transpose + s_dot kappa'').  (One prologue shared through a struct changes the
// order in which the compiler emits the kernels' sin and cos, and with it their register allocation.)
#define PLAN_HESS_F_TERMS                                                                                  \
    const double d = x[1], o = x[2], v = x[4];                                                             \
    const double raw = 1.0 - d * kr;                                                                       \
    const bool gu = fabs(raw) < 1e-4;                                                                      \
    const double g = 1.0 / guard_den(raw);                                                                 \
    const double c = cos(o), sn = sin(o);                                                                  \
    const double gs = gu ? 0.0 : d * k1 * g * g, gd = gu ? 0.0 : kr * g * g;                               \
    const double gss = gu ? 0.0 : d * k2 * g * g + 2.0 * d * d * k1 * k1 * g * g * g;                      \
    const double gsd = gu ? 0.0 : k1 * g * g + 2.0 * d * k1 * kr * g * g * g;                              \
    const double gdd = gu ? 0.0 : 2.0 * kr * kr * g * g * g;                                               \
    const double ds[5] = {v * c * gs, v * c * gd, -v * sn * g, 0.0, c * g};                                \
    const double sd = v * c * g
#define PLAN_HESS_F_REST                                                                                   \
    W[12] += -y[1] * v * sn;                                                                               \
    W[14] += y[1] * c;                                                                                     \
    W[22] += y[1] * c;                                                                                     \
    W[19] += y[2];                                                                                         \
    W[23] += y[2];                                                                                         \
    PLAN_UNROLL                                                                                            \
    for (int j = 0; j < 5; ++j) {                                                                          \
        W[j] += -y[2] * k1 * ds[j];                                                                        \
        W[5 * j] += -y[2] * k1 * ds[j];                                                                    \
    }                                                                                                      \
    W[0] += -y[2] * sd * k2
PLAN_MODEL static void hess_f_folded(const double x[5], double kr, double k1, double k2, const double y[5], double W[25]) {
    PLAN_HESS_F_TERMS;
    const double cs = y[0] - y[2] * kr;
    PLAN_UNROLL
    for (int i = 0; i < 25; ++i) W[i] = 0.0;
    W[0] = cs * v * c * gss;
    W[1] = W[5] = cs * v * c * gsd;
    W[6] = cs * v * c * gdd;
    W[2] = W[10] = cs * -v * sn * gs;
    W[7] = W[11] = cs * -v * sn * gd;
    W[12] = cs * -v * c * g;
    W[4] = W[20] = cs * c * gs;
    W[9] = W[21] = cs * c * gd;
    W[14] = W[22] = cs * -sn * g;
    PLAN_HESS_F_REST;
}
PLAN_MODEL static void hess_f_scaled(const double x[5], double kr, double k1, double k2, const double y[5], double W[25]) {
    PLAN_HESS_F_TERMS;
    double Hs[25];
    for (int i = 0; i < 25; ++i) Hs[i] = 0.0;
    Hs[0] = v * c * gss;
    Hs[1] = Hs[5] = v * c * gsd;
    Hs[6] = v * c * gdd;
    Hs[2] = Hs[10] = -v * sn * gs;
    Hs[7] = Hs[11] = -v * sn * gd;
    Hs[12] = -v * c * g;
    Hs[4] = Hs[20] = c * gs;
    Hs[9] = Hs[21] = c * gd;
    Hs[14] = Hs[22] = -sn * g;
    for (int i = 0; i < 25; ++i) W[i] = (y[0] - y[2] * kr) * Hs[i];
    PLAN_HESS_F_REST;
}
#undef PLAN_HESS_F_TERMS
#undef PLAN_HESS_F_REST

// Hermite-Simpson defect of an interval (:183-208): x_b - (x_a + sign * dt/6 (f_a + 4 f_mid + f_b))
template <class R>
PLAN_MODEL static void defect(const R& rt, const plan_params& P, const double xa[5], const double xb[5], double u1,
                              double u2, double def[5]) {
    const double h = P.dt;
    double fa[5], fb[5], fm[5], xm[5];
    dyn(xa, u1, u2, route_kappa(rt, xa[0], nullptr, nullptr), fa);
    dyn(xb, u1, u2, route_kappa(rt, xb[0], nullptr, nullptr), fb);
    PLAN_UNROLL
    for (int i = 0; i < 5; ++i) xm[i] = 0.5 * (xa[i] + xb[i]) + (h / 8.0) * (fa[i] - fb[i]);
    dyn(xm, u1, u2, route_kappa(rt, xm[0], nullptr, nullptr), fm);
    PLAN_UNROLL
    for (int i = 0; i < 5; ++i) def[i] = xb[i] - (xa[i] + P.defect_sign * (h / 6.0) * (fa[i] + 4.0 * fm[i] + fb[i]));
}

// ------------------------------------------------------------------------------------------------------
// the 3x3 factorisation of the Riccati recursion's control block
// ------------------------------------------------------------------------------------------------------
// H (3 x 3, symmetric positive definite) = L D L' with L unit lower triangular, stored as {1/d0, l10, 1/d1,
// l20, l21, 1/d2}: no square roots, three divisions per factorisation and none in the solves, which sit on
// the solves' dependent chains (oracle/plan_oracle.c uses the same form and rounding).  Fails (false) when a
// pivot is not positive, the Cholesky condition.
PLAN_MODEL static bool chol3(const double H[3][3], double L[6]) {
    const double d0 = H[0][0];
    if (!(d0 > 0.0)) return false;
    L[0] = 1.0 / d0;
    L[1] = H[1][0] * L[0];
    const double d1 = H[1][1] - L[1] * H[1][0];
    if (!(d1 > 0.0)) return false;
    L[2] = 1.0 / d1;
    L[3] = H[2][0] * L[0];
    const double e21 = H[2][1] - L[3] * H[1][0];
    L[4] = e21 * L[2];
    const double d2 = H[2][2] - L[3] * H[2][0] - L[4] * e21;
    if (!(d2 > 0.0)) return false;
    L[5] = 1.0 / d2;
    return true;
}

// b <- (L D L')^-1 b
PLAN_MODEL static inline void chol3_solve(const double L[6], double b[3]) {
    const double y0 = b[0];
    const double y1 = b[1] - L[1] * y0;
    const double y2 = b[2] - L[3] * y0 - L[4] * y1;
    b[2] = y2 * L[5];
    b[1] = y1 * L[2] - L[4] * b[2];
    b[0] = y0 * L[0] - L[1] * b[1] - L[3] * b[2];
}

// ------------------------------------------------------------------------------------------------------
// the evaluator's step of one stage (plan_evaluate_chunks, include/mpcplan_evaluate.h)
// ------------------------------------------------------------------------------------------------------
// numpy's min / max over a sequence that may hold NaN: the value part skips NaN, the flag remembers one
PLAN_MODEL_INLINE void ev_min(double& m, bool& nan, double r) {
    if (r != r) nan = true;
    else if (r < m) m = r;
}
PLAN_MODEL_INLINE void ev_max(double& m, bool& nan, double r) {
    if (r != r) nan = true;
    else if (r > m) m = r;
}

// the cost term of stage k < N (TrajectoryOptimizer.cost, :128-170); cden = max(1, s_total - x0_s)
PLAN_MODEL_INLINE double ev_stage_cost(const plan_params& P, const double x[5], double u1, double u2, double sl,
                                       double s_total, double cden) {
    const double t1 = P.w_y * (x[1] * x[1] + x[2] * x[2]);
    const double e = (s_total - x[0]) / cden;
    const double t2 = P.w_s * (e * e);
    const double t3 = P.w_u * (u1 * u1 + u2 * u2);
    const double t4 = P.w_slack * (sl * sl);
    return ((t1 + t2) + t3) + t4;
}

// The PLAN_EV_NR rows of stage k in column order (:238-349; iv: k < N, else u1 = u2 = sl = 0; term: the stage has
// the intermediate chunk's terminal row), written to ro unless it is null (NaN where the stage has no such row), and
// entered into what a sequence of stages (a lane's on the device, the chunk's on the host) has seen of its rows: the
// first minimum rmin (rnan: it is a NaN) with its place (rstage, rkind) and the number nneg of negative rows.
// Returns the stage's L1 partial of the rows.  The loop over the kinds must unroll fully: a row value indexed at
// run time would put a lane's values in scratch memory.
template <class R>
PLAN_MODEL_INLINE double ev_stage_rows(const R& rt, const plan_params& P, int k, const double x[5], double u1, double u2,
                                       double sl, bool iv, bool term, double starget, double* rows, double& rmin, bool& rnan,
                                       int& rstage, int& rkind, int& nneg) {
    const double vs = x[4] + sl;
    const double kvv = x[3] * (x[4] * x[4]);
    double* ro = rows ? rows + (size_t)k * PLAN_EV_NR : nullptr;
    double p1 = 0.0;
    PLAN_UNROLL
    for (int kind = 0; kind < PLAN_EV_NR; ++kind) {
        double r;
        bool on;
        switch (kind) {
            case PLAN_EVR_VMIN: r = vs - P.v_min; on = true; break;
            case PLAN_EVR_VMAX: r = route_vmax(rt, x[0]) - vs; on = true; break;
            case PLAN_EVR_LATP: r = P.a_max - kvv; on = true; break;
            case PLAN_EVR_LATM: r = P.a_max + kvv; on = true; break;
            case PLAN_EVR_KMIN: r = x[3] - P.k_min; on = true; break;
            case PLAN_EVR_KMAX: r = P.k_max - x[3]; on = true; break;
            case PLAN_EVR_U1MIN: r = u1 - P.u_min[0]; on = iv; break;
            case PLAN_EVR_U1MAX: r = P.u_max[0] - u1; on = iv; break;
            case PLAN_EVR_U2MIN: r = u2 - P.u_min[1]; on = iv; break;
            case PLAN_EVR_U2MAX: r = P.u_max[1] - u2; on = iv; break;
            case PLAN_EVR_S: r = sl; on = iv; break;
            default: r = x[0] - starget / 2.0; on = term; break;
        }
        if (on) {
            // np.argmin: the first NaN wins for good, else the first strictly smaller row
            if (!rnan && (r != r || r < rmin)) {
                rmin = r;
                rstage = k;
                rkind = kind;
                rnan = r != r;
            }
            p1 = p1 + (r != r ? r : (r < 0.0 ? -r : 0.0));
            nneg += r < 0.0 ? 1 : 0;
        }
        if (ro) ro[kind] = on ? r : NAN;
    }
    return p1;
}

}  // namespace plan_model
