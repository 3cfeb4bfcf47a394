// tracker_model.h -- the tracker's model, stated once for its kernels (solve_kernel.h, evaluate_kernel.h,
// gradient_kernel.h, the closed-loop kernels) and for its host backend (cpu_backend.h): the view of the
// reference-signal table and the lookups on it, the solver's constants, the model derived from mpc_params (lane
// bound, which rows exist, the row coefficients, the row and box values of a stage, the A_k coefficients), the
// evaluator's steps and the gradient's steps.  Both sides keep their own storage, loops, lane mapping and
// reductions and hand single values in.  One exception: mpc_solve_kernel
// keeps its own text of stage_A, nearest_obstacle, row_values and box_values (and of loop_steps.h's warm start) in
// its K1 / K2 blocks, because its register allocation moves with any other form of them; the comments there say so.
// What may be written here: single rounded FP64 operations, integer arithmetic, fabs and comparisons (sin / cos for
// the pose).  The build has -ffp-contract=off, so the device pass, the host pass and a plain C++ compiler form the
// same operation sequence.  oracle/mpc_oracle.c shares nothing with this file: it is the independent reference.
#pragma once
#include "../../include/mpcqp.h"
#include <math.h>

#ifdef __HIPCC__
#define TRACKER_MODEL __host__ __device__
#define TRACKER_MODEL_INLINE __host__ __device__ __forceinline__
#define TRACKER_UNROLL _Pragma("unroll")
#else
#define TRACKER_MODEL inline
#define TRACKER_MODEL_INLINE inline
#define TRACKER_UNROLL
#endif

// ------------------------------------------------------------------------------------------
// the solver's constants
// ------------------------------------------------------------------------------------------
constexpr int NROW = 9;               // soft rows per stage: lane +-d, +-(d + L/2 o), +-(d + L o), 2 obstacle, v >= 0
constexpr int NBOX = 4;               // box rows per control: +u1, -u1, +u2, -u2
constexpr double TAU = 0.995;         // fraction of the step to the boundary
constexpr double POLISH_DELTA = 1e-11;
constexpr int POLISH_REFINE = 2;
constexpr int POLISH_ROUNDS = 6;
constexpr int XO_ROUNDS = 1;          // rounds of the crossover attempt before the interior point
// SQP stopping rules besides convergence (oracle orc_solve): a 2-cycle (the QP returns the point of two QPs
// back, |U_k - U_k-2| <= SQP_CYCLE_REL |U_k - U_k-1|), and SQP_INF_STREAK elastic QPs in a row
constexpr double SQP_CYCLE_REL = 1e-6;
constexpr int SQP_INF_STREAK = 5;
constexpr double START_SHIFT = 3.0;   // interior-point start: slack and elastic slack beyond the row value (oracle pdip)
// interior-point checkpoint (oracle pdip): once mu <= MU_CHECK and every row's slack and
// multiplier are CHECK_SEP apart, CHECK_ROUNDS polish rounds try the iterate's classification; a certified point
// is the QP's exact optimum, otherwise the interior point continues from the unchanged iterate (once per QP)
constexpr double MU_CHECK = 1e-4;
constexpr double CHECK_SEP = 100.0;
constexpr int CHECK_ROUNDS = 2;

// ------------------------------------------------------------------------------------------
// the reference-signal table: one buffer of doubles (host_table.h builds it), seen through column pointers.  The
// device context points them into its device copy, HostTable::view() into the host buffer
// ------------------------------------------------------------------------------------------
struct DevTable {
    const double* s;   // [T]  (strict-monotone fixed, trajectory_loader.py:26-30)
    const double* d;
    const double* o;
    const double* k;
    const double* v;
    const double* u1;  // [Tu]
    const double* u2;
    const double* gx;  // [T]  global pose of the reference line (trajectory_loader.py:32-62)
    const double* gy;
    const double* gpsi;
    int T, Tu;
    double smax;
    double last[5];    // X_ref[-1] verbatim (trajectory_loader.py:90-91)
    const int* bidx;   // [nb + 1] bucket index of s: bidx[g] = lower_bound(s, s0 + g h)
    int nb;
    double s0, ibh;    // s[0], 1 / h
};

// scipy interp1d 'linear' + extrapolate (scipy _interpolate.py:457-483).
// Interval of v in the table's s column (n <= T: a prefix of it), i.e. scipy's searchsorted
// (lower bound) clamped to [1, n - 1].  v's bucket g brackets the lower bound: it lies in
// [bidx[g - 1], bidx[g + 2]] (one bucket of slack either side for the rounding of g), so a binary search
// over that window returns the full binary search's answer exactly.  With 4 buckets per table interval
// the window holds ~1 knot (~2 dependent L2 loads instead of log2 T; every instance looks up ~4 N times),
// and a table with clustered knots costs log2 of the knots in the window, never a linear walk.
TRACKER_MODEL_INLINE int seg_t(const DevTable& t, int n, double v) {
    double gf = (v - t.s0) * t.ibh;
    gf = gf > 0.0 ? gf : 0.0;                       // also maps NaN to bucket 0
    const int g = gf < (double)(t.nb - 1) ? (int)gf : t.nb - 1;
    int lo = t.bidx[g > 0 ? g - 1 : 0];
    int hi = g + 2 <= t.nb ? t.bidx[g + 2] : t.T;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t.s[mid] < v) lo = mid + 1; else hi = mid;
    }
    lo = lo < n ? lo : n;
    lo = lo < 1 ? 1 : lo;
    lo = lo > n - 1 ? n - 1 : lo;
    return lo;
}
TRACKER_MODEL_INLINE double lin(const double* x, const double* y, int i, double v) {
    double slope = (y[i] - y[i - 1]) / (x[i] - x[i - 1]);
    return slope * (v - x[i - 1]) + y[i - 1];
}
TRACKER_MODEL_INLINE double slope_at(const double* x, const double* y, int i) {
    return (y[i] - y[i - 1]) / (x[i] - x[i - 1]);
}
// get_state (trajectory_loader.py:86-93): out[5]; slopes (d,o,k,v) for Gauss-Newton (0 past s_max)
TRACKER_MODEL static void get_state(const DevTable& t, double s, double* out, double* sl = nullptr) {
    if (s >= t.smax) {
        for (int j = 0; j < 5; ++j) out[j] = t.last[j];
        if (sl) sl[0] = sl[1] = sl[2] = sl[3] = 0.0;
        return;
    }
    int i = seg_t(t, t.T, s);
    out[0] = s;
    out[1] = lin(t.s, t.d, i, s);
    out[2] = lin(t.s, t.o, i, s);
    out[3] = lin(t.s, t.k, i, s);
    out[4] = lin(t.s, t.v, i, s);
    if (sl) {
        sl[0] = slope_at(t.s, t.d, i);
        sl[1] = slope_at(t.s, t.o, i);
        sl[2] = slope_at(t.s, t.k, i);
        sl[3] = slope_at(t.s, t.v, i);
    }
}
// get_control (trajectory_loader.py:95-102)
TRACKER_MODEL static void get_control(const DevTable& t, double s, double* out) {
    if (s >= t.smax) { out[0] = 0.0; out[1] = 0.0; return; }
    int i = seg_t(t, t.Tu, s);
    out[0] = lin(t.s, t.u1, i, s);
    out[1] = lin(t.s, t.u2, i, s);
}
// get_global_pose (trajectory_loader.py:104-116): out[3] = (x, y, psi) of the point d beside the line at s
TRACKER_MODEL_INLINE void global_pose(const DevTable& t, double s, double d, double* out) {
    if (s > t.smax) s = t.smax;
    const int j = seg_t(t, t.T, s);
    const double xr = lin(t.s, t.gx, j, s), yr = lin(t.s, t.gy, j, s), psi = lin(t.s, t.gpsi, j, s);
    out[0] = xr - d * sin(psi);
    out[1] = yr + d * cos(psi);
    out[2] = psi;
}

// ------------------------------------------------------------------------------------------
// the model derived from mpc_params
// ------------------------------------------------------------------------------------------
// what the kernels are handed; mu_check and dbg are the device context's (the environment's)
struct KParams {
    int N, max_obs, linearization, sqp_iters, max_iter, polish;
    double dt, u_min0, u_min1, u_max0, u_max1;
    double w_d, w_o, w_v, w_u1, w_u2;
    double osd, tgap, L, sl, brake_distance, brake_accel;
    double tol, tol_mu, rho, sqp_tol;
    double mu_check;   // interior-point checkpoint threshold (MU_CHECK; -1 = off, MPC_CHECKPOINT=0)
    int dbg;           // diagnostics only (MPC_DBG, default 0): 1 = the crossover kernel defers without the
                       // work-list atomic (timing probe; the interior-point launch then sees an empty list)
};
// the lane rows' bound (trajectory_tracking.py:169)
inline double lane_bound(const mpc_params& p) { return p.lane_width / 2.0 - p.vehicle_radius - p.safe_lane_margin; }
inline KParams model_params(const mpc_params& p) {
    KParams k;
    k.N = p.N;
    k.max_obs = p.max_obs;
    k.linearization = p.linearization;
    k.sqp_iters = p.sqp_iters;
    k.max_iter = p.max_iter;
    k.polish = p.polish;
    k.dt = p.dt;
    k.u_min0 = p.u_min[0]; k.u_min1 = p.u_min[1];
    k.u_max0 = p.u_max[0]; k.u_max1 = p.u_max[1];
    k.w_d = p.w_d; k.w_o = p.w_o; k.w_v = p.w_v; k.w_u1 = p.w_u1; k.w_u2 = p.w_u2;
    k.osd = p.obstacle_safety_distance;
    k.tgap = p.max_time_2_obs;
    k.L = p.wheelbase;
    k.sl = lane_bound(p);
    k.brake_distance = p.brake_distance;
    k.brake_accel = p.brake_accel;
    k.tol = p.tol;
    k.tol_mu = p.tol_mu;
    k.rho = p.elastic_rho;
    k.sqp_tol = p.sqp_tol;
    k.mu_check = MU_CHECK;
    k.dbg = 0;
    return k;
}

// soft row j exists for an instance: the obstacle rows (6, 7) need obstacles
TRACKER_MODEL_INLINE constexpr bool row_exists(int j, bool has_obs) { return (j != 6 && j != 7) || has_obs; }

// soft row coefficient vectors over (s,d,o,v) (the oracle's C[][] without the k entry):
// h = L / 2, T the time gap
TRACKER_MODEL_INLINE void row_coef(int j, double h, double L, double T, double c[4]) {
    c[0] = c[1] = c[2] = c[3] = 0.0;
    switch (j) {
        case 0: c[1] = 1.0; break;
        case 1: c[1] = -1.0; break;
        case 2: c[1] = 1.0; c[2] = h; break;
        case 3: c[1] = -1.0; c[2] = -h; break;
        case 4: c[1] = 1.0; c[2] = L; break;
        case 5: c[1] = -1.0; c[2] = -L; break;
        case 6: c[0] = -1.0; break;
        case 7: c[0] = -1.0; c[3] = -T; break;
        default: c[3] = 1.0; break;
    }
}

// the position of the nearest obstacle predicted at stage k: the obstacle rows of :194-204 for every obstacle
// collapse to it (infinity without obstacles)
TRACKER_MODEL_INLINE double nearest_obstacle(const double* obs, int nobs, int k, double dt) {
    double shat = INFINITY;
    for (int i = 0; i < nobs; ++i) {
        const double sp = obs[2 * i] + obs[2 * i + 1] * (k * dt);
        shat = sp < shat ? sp : shat;
    }
    return shat;
}
// the row values v[NROW] (by row id) of a stage at its nominal state x, shat its nearest_obstacle
TRACKER_MODEL_INLINE void row_values(const KParams& P, const double* x, double shat, bool has_obs, double* v) {
    const double sl = P.sl;
    const double pv0 = x[1], pv1 = x[1] + (P.L / 2.0) * x[2], pv2 = x[1] + P.L * x[2];
    v[0] = -sl - pv0;
    v[1] = -(sl - pv0);
    v[2] = -sl - pv1;
    v[3] = -(sl - pv1);
    v[4] = -sl - pv2;
    v[5] = -(sl - pv2);
    v[6] = has_obs ? -(shat - P.osd - x[0]) : 0.0;
    v[7] = has_obs ? -(shat - x[0] - P.tgap * x[4]) : 0.0;
    v[8] = -x[4];
}
// the box values bb[NBOX] of a control at its linearisation point (ub1, ub2)
TRACKER_MODEL_INLINE void box_values(const KParams& P, double ub1, double ub2, double* bb) {
    bb[0] = P.u_min0 - ub1;
    bb[1] = -(P.u_max0 - ub1);
    bb[2] = P.u_min1 - ub2;
    bb[3] = -(P.u_max1 - ub2);
}
// the coefficients (a12, a14, a20, a23, a24) of A_k = I + J'_k (J'(0,4) = dt) at the nominal state x: kref the
// reference curvature at x[0], dk its slope (0 without the Gauss-Newton term)
TRACKER_MODEL_INLINE void stage_A(const double* x, double dt, double kref, double dk, double* a) {
    a[0] = dt * x[4];
    a[1] = dt * x[2];
    a[2] = dt * (-x[4] * dk);
    a[3] = dt * x[4];
    a[4] = dt * (x[3] - kref);
}

// ------------------------------------------------------------------------------------------
// the evaluator (mpc_evaluate_batch, include/mpcqp.h): the steps of one control and of one stage, and the sums
// ------------------------------------------------------------------------------------------
enum { EV_NAN_ROW = 1, EV_NAN_LANE = 2, EV_NAN_OBS = 4, EV_NAN_V = 8, EV_NAN_BOX = 16 };

// The running minima of the three row families, the running box excess, and which of them met a NaN: a lane's on
// the device (reduced over the group afterwards), the whole instance's on the host
struct EvRun {
    double fl, fo, fv, bx;
    bool flnan, fonan, fvnan, bxnan;
};
TRACKER_MODEL_INLINE EvRun ev_run_begin() { return EvRun{INFINITY, INFINITY, INFINITY, 0.0, false, false, false, false}; }
// the EV_NAN_* bits of a run and of a stage's (or any stage's) NaN row
TRACKER_MODEL_INLINE int ev_flags(const EvRun& R, bool snan) {
    return (snan ? EV_NAN_ROW : 0) | (R.flnan ? EV_NAN_LANE : 0) | (R.fonan ? EV_NAN_OBS : 0) |
           (R.fvnan ? EV_NAN_V : 0) | (R.bxnan ? EV_NAN_BOX : 0);
}

// NaN-propagating running minimum (numpy's min): once a NaN was seen it stays
TRACKER_MODEL_INLINE void ev_nmin(double& m, bool& nan, double r) {
    if (!nan) {
        if (r != r) nan = true;
        else if (r < m) m = r;
    }
}

// control (u1, u2): its two cost terms to ct[3], ct[4], and the excess over the bounds handed to SLSQP (:249-252)
TRACKER_MODEL_INLINE void ev_control(const KParams& P, double u1, double u2, double* ct, EvRun& R) {
    ct[3] = P.w_u1 * (u1 * u1);
    ct[4] = P.w_u2 * (u2 * u2);
    const double e[4] = {P.u_min0 - u1, u1 - P.u_max0, P.u_min1 - u2, u2 - P.u_max1};
    TRACKER_UNROLL
    for (int a = 0; a < 4; ++a) {
        if (e[a] != e[a]) R.bxnan = true;
        else if (e[a] > R.bx) R.bx = e[a];
    }
}

// what one stage leaves: its minimal row (the first NaN if there is one, else the first minimum: np.argmin) and
// that row's kind, its L1 violation and its count of negative rows
struct EvStage {
    double smin, p1;
    bool snan;
    int skind, nneg;
};
TRACKER_MODEL_INLINE EvStage ev_stage_begin() { return EvStage{INFINITY, 0.0, false, 0, 0}; }
// Stage j at the rolled-out state x with st the reference state at x[0]: its three cost terms to ct[0..2], and
// its rows visited in the reference's order (the six lane rows, the obstacles, v), each stored to ro (row width
// rw, NaN past the obstacles; ro may be null); S starts from ev_stage_begin()
TRACKER_MODEL_INLINE void ev_stage(const KParams& P, int j, const double* x, const double* st, const double* obs,
                                   int nobs, int rw, double* ct, double* ro, EvStage& S, EvRun& R) {
    const double s = x[0], d = x[1], o = x[2], v = x[4];
    const double ed = d - st[1], eo = o - st[2], ev = v - st[4];
    ct[0] = P.w_d * (ed * ed);
    ct[1] = P.w_o * (eo * eo);
    ct[2] = P.w_v * (ev * ev);
    auto visit = [&](double r, int kind) {
        if (!S.snan && (r != r || r < S.smin)) {
            S.smin = r;
            S.skind = kind;
            S.snan = r != r;
        }
        S.p1 = S.p1 + (r != r ? r : (r < 0.0 ? -r : 0.0));
        S.nneg += r < 0.0 ? 1 : 0;
        if (ro) ro[kind] = r;
    };
    const double sl = P.sl;
    const double vf = d + (P.L / 2.0) * o, vl = d + P.L * o;
    const double g[6] = {sl - d, d + sl, sl - vf, vf + sl, sl - vl, vl + sl};
    TRACKER_UNROLL
    for (int a = 0; a < 6; ++a) {
        visit(g[a], a);
        ev_nmin(R.fl, R.flnan, g[a]);
    }
    if (nobs > 0) {
        const double tk = (double)j * P.dt;
        const double vt = v * P.tgap;
        const double safe = vt > P.osd ? vt : P.osd;       // the reference's max(osd, v * tgap)
        for (int i = 0; i < nobs; ++i) {
            const double sop = obs[2 * i] + obs[2 * i + 1] * tk;
            const double r = (sop - s) - safe;
            visit(r, 7 + i);
            ev_nmin(R.fo, R.fonan, r);
        }
    }
    if (ro)
        for (int i = 7 + nobs; i < rw; ++i) ro[i] = NAN;
    visit(v, 6);
    ev_nmin(R.fv, R.fvnan, v);
}

// The sums whose bits must not depend on who adds them, from ct [N][5] (the cost terms d, o, v of stage j + 1 and
// u1, u2 of control j) and part [N] (the stages' L1 violations): the reference's running cost over stages 1..N
// (d, o, v), then controls 0..N-1 (u1, u2), one sum; its five shares t; the L1 violation
struct EvSums {
    double cost, t[5], l1;
};
TRACKER_MODEL_INLINE EvSums ev_sums(int N, const double* ct, const double* part) {
    EvSums Z = {0.0, {0.0, 0.0, 0.0, 0.0, 0.0}, 0.0};
    for (int j = 0; j < N; ++j) {
        TRACKER_UNROLL
        for (int a = 0; a < 3; ++a) {
            Z.cost = Z.cost + ct[5 * j + a];
            Z.t[a] = Z.t[a] + ct[5 * j + a];
        }
        Z.l1 = Z.l1 + part[j];
    }
    for (int j = 0; j < N; ++j) {
        TRACKER_UNROLL
        for (int a = 3; a < 5; ++a) {
            Z.cost = Z.cost + ct[5 * j + a];
            Z.t[a] = Z.t[a] + ct[5 * j + a];
        }
    }
    return Z;
}
// The summary row o [MPC_EV_NQ]: min_row is NaN if a row was, cnt the negative rows, (fl, fo, fv, bx) the instance's
// minima and box excess, flags its EV_NAN_* bits
TRACKER_MODEL_INLINE void ev_summary(double* o, const EvSums& Z, double min_row, int astage, int akind, double cnt,
                                     double fl, double fo, double fv, double bx, int flags, int nobs) {
    o[MPC_EVQ_COST] = Z.cost;
    o[MPC_EVQ_MIN_ROW] = min_row;
    o[MPC_EVQ_ARGMIN_STAGE] = (double)astage;
    o[MPC_EVQ_ARGMIN_KIND] = (double)akind;
    o[MPC_EVQ_L1] = Z.l1;
    o[MPC_EVQ_N_NEG] = cnt;
    // + 0.0: a minimum of -0.0 and 0.0 comes out as 0.0 whichever the reduction met first
    o[MPC_EVQ_MIN_LANE] = (flags & EV_NAN_LANE) ? NAN : fl + 0.0;
    o[MPC_EVQ_MIN_OBS] = ((flags & EV_NAN_OBS) || nobs == 0) ? NAN : fo + 0.0;
    o[MPC_EVQ_MIN_V] = (flags & EV_NAN_V) ? NAN : fv + 0.0;
    o[MPC_EVQ_BOX] = (flags & EV_NAN_BOX) ? NAN : bx + 0.0;
}

// ------------------------------------------------------------------------------------------
// the gradient (mpc_gradient_batch, include/mpcqp.h): the derivative of what the evaluator computes, by one reverse
// (adjoint) sweep over the rollout for the cost and one for the rows weighted by lam.  The table is piecewise linear:
// its slope at s is get_state's sl[] (the interval seg_t selects, so the left one at a knot; 0 past s_max)
// ------------------------------------------------------------------------------------------
// m <- max / min(m, a) with numpy's NaN rule (loop_steps.h's keep_max / keep_min): a NaN enters and stays
TRACKER_MODEL_INLINE void gr_nmax(double& m, double a) {
    if (a > m || a != a) m = a;
}
TRACKER_MODEL_INLINE void gr_nmin(double& m, double a) {
    if (a < m || a != a) m = a;
}
// The running extremes of the summary: a lane's on the device (reduced over the group afterwards), the whole
// instance's on the host.  The maxima are of absolute values, so they start from 0
struct GrRun {
    double ginf, linf, pginf, compl_, minlam;
};
TRACKER_MODEL_INLINE GrRun gr_run_begin() { return GrRun{0.0, 0.0, 0.0, 0.0, INFINITY}; }

// Stage j at the rolled-out state x, with st the reference state at x[0] and sl its slopes (d', o', k', v'):
//   q[5]  the gradient of the stage's cost terms in (s, d, o, k, v)
//   c[5]  sum_r lam[r] grad_x g_r over the stage's rows in the reference's order (the six lane rows, the obstacles,
//         v), each component one running sum from 0 that skips the rows whose coefficient in it is structurally 0;
//         lam is the stage's slice in the `rows` layout (0..5 lane, 6 v, 7 + i obstacle i), columns >= 7 + nobs are
//         not read.  Zero when lam is null
// and into R the complementarity |lam_r g_r| and lam_r of every row read.  The row values are ev_stage's expressions
TRACKER_MODEL_INLINE void gr_stage(const KParams& P, int j, const double* x, const double* st, const double* sl,
                                   const double* obs, int nobs, const double* lam, double* q, double* c, GrRun& R) {
    const double s = x[0], d = x[1], o = x[2], v = x[4];
    const double gd = (2.0 * P.w_d) * (d - st[1]);
    const double go = (2.0 * P.w_o) * (o - st[2]);
    const double gv = (2.0 * P.w_v) * (v - st[4]);
    q[0] = -((gd * sl[0] + go * sl[1]) + gv * sl[3]);
    q[1] = gd;
    q[2] = go;
    q[3] = 0.0;
    q[4] = gv;
    c[0] = c[1] = c[2] = c[3] = c[4] = 0.0;
    if (!lam) return;
    auto visit = [&](double l, double g) {
        gr_nmax(R.compl_, fabs(l * g));
        gr_nmin(R.minlam, l);
    };
    const double bl = P.sl, h = P.L / 2.0;
    const double vf = d + h * o, vl = d + P.L * o;
    const double g[6] = {bl - d, d + bl, bl - vf, vf + bl, bl - vl, vl + bl};
    const double go_[3] = {0.0, h, P.L};              // |dg/do| of the row pairs; dg/dd = -1, +1 within a pair
    TRACKER_UNROLL
    for (int a = 0; a < 6; ++a) {
        const double l = lam[a];
        c[1] = (a & 1) ? c[1] + l : c[1] - l;
        if (a >= 2) c[2] = (a & 1) ? c[2] + l * go_[a >> 1] : c[2] - l * go_[a >> 1];
        visit(l, g[a]);
    }
    if (nobs > 0) {
        const double tk = (double)j * P.dt;
        const double vt = v * P.tgap;
        const bool gap = vt > P.osd;                   // the reference's max(osd, v * tgap) follows v
        const double safe = gap ? vt : P.osd;
        for (int i = 0; i < nobs; ++i) {
            const double l = lam[7 + i];
            const double sop = obs[2 * i] + obs[2 * i + 1] * tk;
            c[0] = c[0] - l;
            if (gap) c[4] = c[4] - l * P.tgap;
            visit(l, (sop - s) - safe);
        }
    }
    c[4] = c[4] + lam[6];
    visit(lam[6], v);
}

// y = A' p with a = stage_A's (a12, a14, a20, a23, a24)
TRACKER_MODEL_INLINE void gr_AT(const double* a, double dt, const double* p, double* y) {
    y[0] = p[0] + a[2] * p[2];
    y[1] = p[1];
    y[2] = p[2] + a[0] * p[1];
    y[3] = p[3] + a[3] * p[2];
    y[4] = ((p[4] + dt * p[0]) + a[1] * p[1]) + a[4] * p[2];
}
// The reverse sweep, in place: z [N][5] holds the stage terms of stages 1..N and returns the costates p_1..p_N
// (p_N = z_N; p_k = z_k + A_k' p_k+1 for k = N-1..1); A [N][5] holds stage_A at x_0..x_N-1; g0 = A_0' p_1
TRACKER_MODEL_INLINE void gr_sweep(int N, double dt, const double* A, double* z, double* g0) {
    double y[5];
    for (int k = N - 1; k >= 1; --k) {
        gr_AT(A + 5 * k, dt, z + 5 * k, y);
        TRACKER_UNROLL
        for (int a = 0; a < 5; ++a) z[5 * (k - 1) + a] = z[5 * (k - 1) + a] + y[a];
    }
    gr_AT(A, dt, z, y);
    TRACKER_UNROLL
    for (int a = 0; a < 5; ++a) g0[a] = y[a];
}
// Control k = (u1, u2) with p = p_k+1 of the cost and pr = p'_k+1 of the rows (null without lam): its gradient g[2],
// its J' lam jt[2] (zero without lam), and into R |g|, |g - jt| and the projected-gradient measure
// |clamp(u - (g - jt), u_min, u_max) - u| for the bounds handed to SLSQP
TRACKER_MODEL_INLINE void gr_control(const KParams& P, double u1, double u2, const double* p, const double* pr,
                                     double* g, double* jt, GrRun& R) {
    g[0] = (2.0 * P.w_u1) * u1 + P.dt * p[3];
    g[1] = (2.0 * P.w_u2) * u2 + P.dt * p[4];
    jt[0] = pr ? P.dt * pr[3] : 0.0;
    jt[1] = pr ? P.dt * pr[4] : 0.0;
    const double u[2] = {u1, u2}, lo[2] = {P.u_min0, P.u_min1}, hi[2] = {P.u_max0, P.u_max1};
    TRACKER_UNROLL
    for (int a = 0; a < 2; ++a) {
        const double r = pr ? g[a] - jt[a] : g[a];
        const double t = u[a] - r;
        const double cl = t < lo[a] ? lo[a] : (t > hi[a] ? hi[a] : t);     // a NaN passes through
        gr_nmax(R.ginf, fabs(g[a]));
        gr_nmax(R.linf, fabs(r));
        gr_nmax(R.pginf, fabs(cl - u[a]));
    }
}
// The summary row o [MPC_GR_NQ] from the instance's extremes; + 0.0: a minimum of -0.0 and 0.0 comes out as 0.0
// whichever the reduction met first
TRACKER_MODEL_INLINE void gr_summary(double* o, double cost, const GrRun& R, bool has_lam) {
    o[MPC_GRQ_COST] = cost;
    o[MPC_GRQ_GRAD_INF] = R.ginf;
    o[MPC_GRQ_LAG_INF] = R.linf;
    o[MPC_GRQ_PG_INF] = R.pginf;
    o[MPC_GRQ_COMPL] = has_lam ? R.compl_ : NAN;
    o[MPC_GRQ_MIN_LAM] = has_lam ? R.minlam + 0.0 : NAN;
}

// ------------------------------------------------------------------------------------------
// the multiplier estimate (mpc_multipliers_batch, include/mpcqp.h): least squares of grad = J' lam over the active
// rows and the free controls.  The steps both sides decide by: the active test, the free test, the list order, a
// row's own gradient and its reverse chain, the drop test and the summary
// ------------------------------------------------------------------------------------------
// a NaN row is never active
TRACKER_MODEL_INLINE bool mu_active(double g, double active_tol) { return g <= active_tol; }
// component c of a control u with its bounds (lo, hi); a NaN control is never free
TRACKER_MODEL_INLINE bool mu_free(double u, double lo, double hi, double bound_tol) {
    return lo + bound_tol < u && u < hi - bound_tol;
}
TRACKER_MODEL_INLINE bool mu_finite(double x) { return fabs(x) < INFINITY; }
// the column (`rows` layout) of the i-th row of a stage in the reference's order, i = 0..6 + nobs: the six lane rows,
// the obstacles, v
TRACKER_MODEL_INLINE int mu_list_col(int i, int nobs) { return i < 6 ? i : (i < 6 + nobs ? i + 1 : 6); }
// grad_x g of the row in column col alone at the rolled-out state x: gr_stage's c for a unit weight on that row
TRACKER_MODEL_INLINE void mu_row_grad(const KParams& P, int col, const double* x, double* c) {
    c[0] = c[1] = c[2] = c[3] = c[4] = 0.0;
    if (col < 6) {
        const double go = col < 2 ? 0.0 : (col < 4 ? P.L / 2.0 : P.L);
        c[1] = (col & 1) ? 1.0 : -1.0;
        if (col >= 2) c[2] = (col & 1) ? go : -go;
    } else if (col == 6) {
        c[4] = 1.0;
    } else {
        c[0] = -1.0;
        if (x[4] * P.tgap > P.osd) c[4] = -P.tgap;
    }
}
// The reverse chain of a row at stage t (1..N) from c = mu_row_grad: p_t = c, p_k = A_k' p_k+1; store(i, v) takes
// j_a[i] for i = 2t-1 .. 0 (the components at or after stage t are zero and are not visited)
template <typename Store>
TRACKER_MODEL_INLINE void mu_row_chain(int t, double dt, const double* A, const double* c, Store store) {
    double p[5] = {c[0], c[1], c[2], c[3], c[4]}, y[5];
    for (int k = t - 1; k >= 0; --k) {
        store(2 * k + 1, dt * p[4]);
        store(2 * k, dt * p[3]);
        if (k >= 1) {
            gr_AT(A + 5 * k, dt, p, y);
            TRACKER_UNROLL
            for (int a = 0; a < 5; ++a) p[a] = y[a];
        }
    }
}
// the drop rule: the pivot d against the original diagonal g0
TRACKER_MODEL_INLINE bool mu_keep(double d, double g0, double rank_tol) { return d > rank_tol * g0; }
// the status from the counts (nonfinite: grad or a row gradient is not finite on a free component)
TRACKER_MODEL_INLINE int mu_status(int n_active, int n_free, bool nonfinite) {
    return n_active > MPC_MAX_ACTIVE ? MPC_MU_OVERFLOW
                                     : (n_active > 0 && n_free == 0 ? MPC_MU_NO_FREE : (nonfinite ? MPC_MU_NONFINITE : MPC_MU_OK));
}
// The summary row o [MPC_MU_NQ]; resid and min_pivot are taken as they are when the status is OK
TRACKER_MODEL_INLINE void mu_summary(double* o, int status, int n_active, int n_free, int n_used, double resid,
                                     double min_pivot) {
    const bool ok = status == MPC_MU_OK;
    o[MPC_MUQ_STATUS] = (double)status;
    o[MPC_MUQ_N_ACTIVE] = (double)n_active;
    o[MPC_MUQ_N_FREE] = (double)n_free;
    o[MPC_MUQ_N_USED] = ok ? (double)n_used : 0.0;
    o[MPC_MUQ_RESID] = ok ? resid : NAN;
    o[MPC_MUQ_MIN_PIVOT] = (ok && n_used > 0) ? min_pivot : NAN;
}

// ------------------------------------------------------------------------------------------
// the Hessian-vector products and row tangents (mpc_hessvec_batch, include/mpcqp.h): for a direction v in U the
// forward tangent chain dx_k over the rollout, the directional derivative of every row, and the second-order reverse
// chain dpi_k whose control components give (d2 L / dU2) v.  Rows and references are piecewise linear, so the only
// second-order terms are the cost's own Hessian (hv_stage) and the bilinear dynamics weighted by the costate
// (hv_second_order)
// ------------------------------------------------------------------------------------------
// the pass width of the device kernel (hessvec_kernel.h): the directions a wavefront carries at once
TRACKER_MODEL_INLINE constexpr int hv_pass_width(int N) { return N <= MPC_HV_N64_MAX ? 64 : 32; }
// component c of control k of direction m: V's entry, or that of the unit vector e_m (m = 2k + c) without V
TRACKER_MODEL_INLINE double hv_dir(const double* V, int m, int k, int c) {
    return V ? V[2 * k + c] : (m == 2 * k + c ? 1.0 : 0.0);
}
// y = dx_k+1 = A_k dx_k + dt (0, 0, 0, v1, v2) with a = stage_A's (a12, a14, a20, a23, a24) at x_k
TRACKER_MODEL_INLINE void hv_tangent_step(const double* a, double dt, const double* dx, double v1, double v2,
                                          double* y) {
    y[0] = dx[0] + dt * dx[4];
    y[1] = (dx[1] + a[0] * dx[2]) + a[1] * dx[4];
    y[2] = ((dx[2] + a[2] * dx[0]) + a[3] * dx[3]) + a[4] * dx[4];
    y[3] = dx[3] + dt * v1;
    y[4] = dx[4] + dt * v2;
}
// grad_x g . dx of the row in column col (`rows` layout) at the rolled-out state x: mu_row_grad's coefficients.
// NaN for a column past the instance's obstacles
TRACKER_MODEL_INLINE double hv_row_tangent(const KParams& P, int col, int nobs, const double* x, const double* dx) {
    if (col < 6) {
        const double go = col < 2 ? 0.0 : (col < 4 ? P.L / 2.0 : P.L);
        const double t = col < 2 ? dx[1] : dx[1] + go * dx[2];
        return (col & 1) ? t : -t;
    }
    if (col == 6) return dx[4];
    if (col - 7 >= nobs) return NAN;
    return x[4] * P.tgap > P.osd ? -dx[0] - P.tgap * dx[4] : -dx[0];
}
// y = Q_k dx: the Hessian of stage k's cost terms (sl = the slopes d', o', k', v' at x_k) applied to dx
TRACKER_MODEL_INLINE void hv_stage(const KParams& P, const double* sl, const double* dx, double* y) {
    const double td = (2.0 * P.w_d) * (dx[1] - sl[0] * dx[0]);
    const double to = (2.0 * P.w_o) * (dx[2] - sl[1] * dx[0]);
    const double tv = (2.0 * P.w_v) * (dx[4] - sl[3] * dx[0]);
    y[0] = -((td * sl[0] + to * sl[1]) + tv * sl[3]);
    y[1] = td;
    y[2] = to;
    y[3] = 0.0;
    y[4] = tv;
}
// e = E_k = (dA_k[dx_k])' pi_k+1: the bilinear dynamics' second-order term, dk = k_ref' at x_k, pi = pi_k+1
TRACKER_MODEL_INLINE void hv_second_order(double dt, double dk, const double* dx, const double* pi, double* e) {
    const double da12 = dt * dx[4], da14 = dt * dx[2], da20 = dt * (-dx[4] * dk), da23 = dt * dx[4];
    const double da24 = dt * (dx[3] - dk * dx[0]);
    e[0] = da20 * pi[2];
    e[1] = 0.0;
    e[2] = da12 * pi[1];
    e[3] = da23 * pi[2];
    e[4] = da14 * pi[1] + da24 * pi[2];
}
// y = dpi_k = (qd + A_k' dpi_k+1) + e with qd = hv_stage's and e = hv_second_order's; e is left out (not read) in
// Gauss-Newton mode
TRACKER_MODEL_INLINE void hv_reverse_step(const double* a, double dt, const double* qd, const double* dpn,
                                          bool exact, const double* e, double* y) {
    double t[5];
    gr_AT(a, dt, dpn, t);
    TRACKER_UNROLL
    for (int i = 0; i < 5; ++i) y[i] = exact ? (qd[i] + t[i]) + e[i] : qd[i] + t[i];
}
// control k of the direction (v1, v2) with dp = dpi_k+1: its two components of H v
TRACKER_MODEL_INLINE void hv_control(const KParams& P, double v1, double v2, const double* dp, double* hv) {
    hv[0] = (2.0 * P.w_u1) * v1 + P.dt * dp[3];
    hv[1] = (2.0 * P.w_u2) * v2 + P.dt * dp[4];
}
// one term of (v'Hv, v'v): both are running sums from 0 over i = 0..2N-1
TRACKER_MODEL_INLINE void hv_curv(double* cv, double v, double hv) {
    cv[0] = cv[0] + v * hv;
    cv[1] = cv[1] + v * v;
}
// The summary row o [MPC_HV_NQ] from curv [M][2], visited in increasing m: the Rayleigh quotients' extremes under
// numpy's NaN rule, np.argmin's direction (the first minimum; the first NaN) and the count of v'Hv < 0
TRACKER_MODEL_INLINE void hv_summary(double* o, double cost, int M, const double* curv) {
    double lo = 0.0, hi = 0.0;
    int arg = 0, nneg = 0;
    for (int m = 0; m < M; ++m) {
        const double r = curv[2 * m] / curv[2 * m + 1];
        if (m == 0) {
            lo = hi = r;
        } else {
            if (lo == lo && (r != r || r < lo)) {
                lo = r;
                arg = m;
            }
            if (hi == hi && (r != r || r > hi)) hi = r;
        }
        nneg += curv[2 * m] < 0.0 ? 1 : 0;
    }
    o[MPC_HVQ_COST] = cost;
    o[MPC_HVQ_MIN_RAYLEIGH] = lo;
    o[MPC_HVQ_MAX_RAYLEIGH] = hi;
    o[MPC_HVQ_ARGMIN_DIR] = (double)arg;
    o[MPC_HVQ_N_NEG] = (double)nneg;
}
