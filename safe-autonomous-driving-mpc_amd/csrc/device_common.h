// device_common.h -- shared device definitions of the tracking-MPC solver (included by mpcqp.hip through the
// kernel headers): the per-instance LDS layout, the row helpers, the fast reciprocals, the cross-lane (DPP /
// permlane) helpers and lane groups, the nominal rollout and the fences of the stage pipelines.  The table, the
// kernel parameters, the reference-signal lookups, the solver's constants and the row coefficients are
// tracker_model.h's, shared with the host backend.
#pragma once
#include <hip/hip_runtime.h>

#include "tracker_model.h"

#define WAVE 64

// ------------------------------------------------------------------------------------------
// wave helpers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, WAVE));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, WAVE));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
    return v;
}
__device__ __forceinline__ void wave_sync() { __syncthreads(); }

// ------------------------------------------------------------------------------------------
// per-instance LDS layout (doubles); stage arrays indexed by stage k = 0..N
// ------------------------------------------------------------------------------------------
// Stage records read by the recursions are padded to an even number of doubles and every array
// starts 16-B aligned, so each pair is one ds_read_b128 (4 LDS cycles) instead of a ds_read2_b64 (8).
// The Riccati recursions are lane-distributed (section "distributed recursions" below): lane i = 0..4
// of a group holds row i of P / component i of the state, so the records they read per lane are laid
// out by row: QR (row i of the stage Hessian), QH (component i of the linear term); KR holds K by rows.
#define A5S 8          // stride of A5: a12, a14, a20, a23, a24, dt, 0, 0 (the zeros and dt serve the
                       // per-lane coefficient gathers of the distributed recursions)
#define SIS 4          // stride of Si (3 used)
#define QRS 20         // stride of QR: rows i = 0..4 (s,d,o,k,v) x columns (s,d,o,v); row 3 (k) zero
#define QHS 6          // stride of QH: (s,d,o,k,v) with k = 0, one pad
#define KRS 12         // stride of KR: rows r = 0, 1 of K_t, each (K(r,0..4), kk_r)
struct Lds {
    double* A5;    // [N][A5S]
    double* cst;   // [N+1][6]  cost data of stage k: (-d_ref', -o_ref', -v_ref') and the residuals r_d, r_o, r_v
    double* QR;    // [N+1][QRS] Riccati stage Hessians (barrier / penalty augmented), by row
    double* Rt;    // [N][2]
    double* KR;    // [N][KRS]  Riccati gains by row, K(r,0..4), with the solve's feed-forward kk_r in slot 5
    double* Si;    // [N][SIS]  (1/l00, l10, 1/l11) of S_t = Ls Ls'
    double* QH;    // [N+1][QHS] LQR stage linear terms (state)
    double* gh;    // [N][2]    LQR stage linear terms (control)
    double* Xr;    // [N+1][5]  nominal rollout (setup, outputs); aliases QH, which is dead then
    double* dX;    // [N+1][5]  rollout of the direction
    double* dud;   // [N][2]    direction dU
    double* ys;    // [N+1][4]  dual-residual stage terms yc + ya (cost part + multiplier part)
    double* zs;    // [N][2]    control terms zc + za
    double* ub;    // [N][2]    linearisation point
    double* kap;   // [N+1]     k_ref(xbar_k) (setup); aliases QH after Xr
    double* AC;    // [N][5][6] closed-loop rows (A_t + B K_t)(i,:) and (B kk_t)_i of the forward solve
                   //           (kernels with acl_on only; rows 0..2 are A's, written at setup)
};
// the forward solve reads closed-loop rows (AC) in the horizon-specialised kernels and for GL = 64; the
// runtime-horizon GL <= 32 kernels keep the K-row form (AC would cost them an occupancy step at N ~ 30)
__host__ __device__ constexpr bool acl_on(int GL, int NT) { return NT > 0 || GL == 64; }
// The crossover launch (MODE_XO) carves a lite layout: no AC (K-row forward solve), no cost data (held
// in registers: lane k-1 is its only writer and reader), no dual-residual terms (ys, zs; interior point
// only), and the direction dud aliases gh (gh is dead once kk is formed; dud is read only after the
// solve, and every solve's caller rewrites gh first).  At N = 20 that is 1251 doubles per instance, so
// 8 two-instance workgroups (20 KB each) fit the 160 KB of a CU: all 2048 crossover waves of a 4096
// batch are resident at once, two per SIMD, instead of running in two rounds.
// At convergence the separate dual-residual terms (yc, ya, zc, za) go to a scratch in QR rows 0..2
// (the factorisation is dead then; the polish rewrites those rows): yc of stage k at QR[k][0..3],
// ya at QR[k][4..7], zc / za of control t at QR[t][8..9] / QR[t][10..11].
#define DQ_YC 0
#define DQ_YA 4
#define DQ_ZC 8
#define DQ_ZA 10

// stage cache record of the split launch, per work-list slot: ub [N][2], Xr [N+1][5], then the crossover's solve
// (the unconstrained optimum of QP(ubar), the interior point's start) by lane: du of control k-1 and x4 of
// stage k, [N][6]; then, from an even offset, the trajectory lookups at each stage's nominal s (get_state's
// d, o, k, v and its slopes d', o', k', v'), [N+1][8], so MODE_IPM repeats no table search.  Even record size:
// every record and its lookup block start 16-byte aligned.
__host__ __device__ constexpr int stage_cache_xo(int N) { return 2 * N + 5 * (N + 1); }
__host__ __device__ constexpr int stage_cache_lk(int N) { return (stage_cache_xo(N) + 6 * N + 1) & ~1; }
__host__ __device__ constexpr int stage_cache_doubles(int N) { return stage_cache_lk(N) + 8 * (N + 1); }

// GL, the lanes an instance takes: the smallest of 16, 32, 64 that holds its N + 1 stages (lane k = stage k), so a
// wavefront serves WAVE / GL instances.  The solver, evaluator and gradient launches all group by it
__host__ __device__ constexpr int lane_group(int N) { return N + 1 <= 16 ? 16 : (N + 1 <= 32 ? 32 : 64); }

__host__ __device__ inline int lds_doubles(int N, bool acl, bool lite = false) {
    int NP = N + 1;
    int n = (acl ? N * 30 : 0) + N * A5S + (lite ? 0 : NP * 6) + NP * QRS + N * 2 + N * KRS + N * SIS + NP * QHS + N * 2 +
            (lite ? 0 : N * 2 + NP * 4 + N * 2) + N * 2 + NP * 5;
    return (n + 1) & ~1;     // groups stay 16-B aligned
}

__device__ inline Lds carve(double* p, int N, bool acl, bool lite = false) {
    Lds L;
    int NP = N + 1;
    // even-sized arrays first (16-B aligned starts), the odd-sized ones last
    L.AC = p; p += acl ? N * 30 : 0;
    L.A5 = p; p += N * A5S;
    L.cst = lite ? nullptr : p; p += lite ? 0 : NP * 6;
    L.QR = p; p += NP * QRS;
    L.Rt = p; p += N * 2;
    L.KR = p; p += N * KRS;
    L.Si = p; p += N * SIS;
    L.QH = p;
    L.Xr = p;                 // Xr [NP][5] and kap [NP] share QH's NP * 6 doubles
    L.kap = p + NP * 5;
    p += NP * QHS;
    L.gh = p; p += N * 2;
    L.dud = lite ? L.gh : p; p += lite ? 0 : N * 2;
    L.ys = lite ? nullptr : p; p += lite ? 0 : NP * 4;
    L.zs = lite ? nullptr : p; p += lite ? 0 : N * 2;
    L.ub = p; p += N * 2;
    L.dX = p; p += NP * 5;
    return L;
}

// packed symmetric 4x4 on (s,d,o,v): index of (a,b)
__host__ __device__ __forceinline__ int p4(int a, int b) {
    if (a > b) { int t = a; a = b; b = t; }
    return a == 0 ? b : (a == 1 ? 3 + b : (a == 2 ? 5 + b : 9));
}
// state index (0..4: s,d,o,k,v) of reduced index (0..3: s,d,o,v)
__device__ __forceinline__ int st4(int a) { return a == 3 ? 4 : a; }

__device__ __forceinline__ double bsign(int j) { return (j & 1) ? -1.0 : 1.0; }   // box rows +u1,-u1,+u2,-u2
__device__ __forceinline__ double dot4(const double c[4], const double x[4]) {
    return fma(c[0], x[0], fma(c[1], x[1], fma(c[2], x[2], c[3] * x[3])));
}
// structural nonzeros of the soft-row coefficient vectors (row_coef): (s,d,o,v) entry a of row j
__host__ __device__ constexpr bool row_nz(int j, int a) {
    return j <= 1 ? a == 1 : (j <= 5 ? (a == 1 || a == 2) : (j == 6 ? a == 0 : (j == 7 ? (a == 0 || a == 3) : a == 3)));
}
// dot4 over the structural nonzeros only, in dot4's association order (identical for finite x: the
// skipped terms are exact zeros); the multiplications by literal zeros are not folded by the compiler
__device__ __forceinline__ double rdot(int j, const double c[4], const double x[4]) {
    double acc = 0.0;
    bool first = true;
#pragma unroll
    for (int a = 3; a >= 0; --a)
        if (row_nz(j, a)) {
            acc = first ? c[a] * x[a] : fma(c[a], x[a], acc);
            first = false;
        }
    return acc;
}
// 1/sqrt(x) to full double precision: v_rsq_f64 + one third-order correction (the Cholesky pivots only
// enter as reciprocals; the IEEE sqrt sequence costs ~100 cycles of dependent latency on gfx950)
__device__ __forceinline__ double frsqrt(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    // one third-order step: with e = 1 - x y^2 (|e| < 2^-22 from v_rsq_f64), 1/sqrt(x) =
    // y (1 + e/2 + 3e^2/8 + O(e^3)); 4 dependent levels instead of the 6 of two Newton steps
    const double e = fma(-x * y, y, 1.0);
    return fma(y * e, fma(0.375, e, 0.5), y);
}
// 1/x to full double precision: v_rcp_f64 + one third-order correction (no IEEE division sequence)
__device__ __forceinline__ double frcp(double x) {
    const double r = __builtin_amdgcn_rcp(x);
    const double e = fma(-x, r, 1.0);
    // one third-order step: 1/x = r (1 + e + e^2 + O(e^3)) with e = 1 - x r
    return fma(r, fma(e, e, e), r);
}

// v_max_f64 / v_min_f64 as single instructions.  For fmax/fmin LLVM first quiets every operand it
// cannot prove canonical (DPP and permlane results, selects, loop-carried values) with an extra
// v_max_f64 x, x, x; arithmetic here only ever makes quiet NaNs, for which the bare instruction already
// has fmax's semantics (the other operand wins), so results are unchanged.
__device__ __forceinline__ double vmax(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double vmin(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// max(a, |b|)
__device__ __forceinline__ double vmaxabs(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// ------------------------------------------------------------------------------------------
// lane groups: IPW instances per 64-lane wavefront, GL = 64 / IPW lanes each
// ------------------------------------------------------------------------------------------
// Cross-lane moves of a double for the group reductions: DPP within a row of 16 lanes (quad_perm
// xor 1 / xor 2, row_half_mirror, row_mirror; a few cycles each) and ds_swizzle xor 16 within 32 lanes,
// instead of ds_bpermute (~80 cycles per hop).  After the quad steps every lane of a quad holds the
// quad value, so the mirrors pair the right partners; a + b == b + a keeps all lanes bit-identical.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// Row pairs and wave halves: v_permlane16_swap / v_permlane32_swap with the value in both operands
// return both sides of the pair (rows 2r and 2r+1 of 16 lanes; lanes i and i+32) on every lane, in two
// VALU slots per double and no LDS round trip (ds_swizzle / ds_bpermute wait ~60-80 cycles per hop).
// tools/probes/xlane_probe.hip checks the semantics.
__device__ __forceinline__ double pack_d(unsigned lo, unsigned hi) {
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
template <int W>
__device__ __forceinline__ void xpair_d(double v, double& a, double& b) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
    if constexpr (W == 16) {
        const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        a = pack_d(l[0], h[0]);
        b = pack_d(l[1], h[1]);
    } else {
        const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        a = pack_d(l[0], h[0]);
        b = pack_d(l[1], h[1]);
    }
}
#define DPP_XOR1 0xB1          // quad_perm [1,0,3,2]
#define DPP_XOR2 0x4E          // quad_perm [2,3,0,1]
#define DPP_HMIRROR 0x141      // row_half_mirror
#define DPP_MIRROR 0x140       // row_mirror

template <int GL>
struct Grp {
    int base;   // first lane of the group
    template <typename OP>
    __device__ __forceinline__ double reduce(double v, OP op) const {
        v = op(v, dpp_d<DPP_XOR1>(v));
        v = op(v, dpp_d<DPP_XOR2>(v));
        v = op(v, dpp_d<DPP_HMIRROR>(v));
        v = op(v, dpp_d<DPP_MIRROR>(v));
        // the same (a, b) operand order on both sides of a pair: every lane ends bit-identical
        double a, b;
        if (GL >= 32) { xpair_d<16>(v, a, b); v = op(a, b); }
        if (GL >= 64) { xpair_d<32>(v, a, b); v = op(a, b); }
        return v;
    }
    __device__ __forceinline__ double sum(double v) const {
        return reduce(v, [](double a, double b) { return a + b; });
    }
    __device__ __forceinline__ double max(double v) const {
        return reduce(v, [](double a, double b) { return vmax(a, b); });
    }
    __device__ __forceinline__ double min(double v) const {
        return reduce(v, [](double a, double b) { return vmin(a, b); });
    }
    __device__ __forceinline__ double get(double v, int rel) const { return __shfl(v, base + rel, WAVE); }
};

// nonlinear rollout (predict, trajectory_tracking.py:87-114), bit-exact.  s, v, k do not depend on
// the k_ref lookups, so they are rolled first; lane j then looks up k_ref(s_j); then d, o.
// st_ln / sl_ln (optional): lane j <= N also returns its whole lookup at s_j with the slopes (get_state), which
// is the stage data's lookup of the QP at this rollout: one table search per stage instead of two.
__device__ void predict_grp(const DevTable& tab, int N, double dt, const double* x0, const double* uU, double* xout,
                            double* kap, int ln, double* st_ln = nullptr, double* sl_ln = nullptr) {
    if (ln == 0) {
        double s = x0[0], k = x0[3], v = x0[4];
        for (int a = 0; a < 5; ++a) xout[a] = x0[a];
        for (int j = 0; j < N; ++j) {
            double s1 = s + dt * v;
            double k1 = k + dt * uU[2 * j];
            double v1 = v + dt * uU[2 * j + 1];
            s = s1; k = k1; v = v1;
            xout[5 * (j + 1) + 0] = s;
            xout[5 * (j + 1) + 3] = k;
            xout[5 * (j + 1) + 4] = v;
        }
    }
    wave_sync();
    if (st_ln ? ln <= N : ln < N) {
        double st[5];
        get_state(tab, xout[5 * ln], st, sl_ln);
        if (ln < N) kap[ln] = st[3];
        if (st_ln)
            for (int a = 0; a < 5; ++a) st_ln[a] = st[a];
    }
    wave_sync();
    if (ln == 0) {
        double d = x0[1], o = x0[2];
        for (int j = 0; j < N; ++j) {
            double v = xout[5 * j + 4], k = xout[5 * j + 3];
            double xd1 = v * o, xd2 = v * (k - kap[j]);
            double d1 = d + dt * xd1;
            double o1 = o + dt * xd2;
            d = d1; o = o1;
            xout[5 * (j + 1) + 1] = d;
            xout[5 * (j + 1) + 2] = o;
        }
    }
    wave_sync();
}

// A_k x with A_k = I + J'_k (sparse)
__device__ __forceinline__ void applyA(const double* a, double dt, const double x[5], double y[5]) {
    y[0] = fma(dt, x[4], x[0]);
    y[1] = fma(a[0], x[2], fma(a[1], x[4], x[1]));
    y[2] = fma(a[2], x[0], fma(a[3], x[3], fma(a[4], x[4], x[2])));
    y[3] = x[3];
    y[4] = x[4];
}
__device__ __forceinline__ void applyAT(const double* a, double dt, const double m[5], double y[5]) {
    y[0] = fma(a[2], m[2], m[0]);
    y[1] = m[1];
    y[2] = fma(a[0], m[1], m[2]);
    y[3] = fma(a[3], m[2], m[3]);
    y[4] = fma(dt, m[0], fma(a[1], m[1], fma(a[4], m[2], m[4])));
}

// packed symmetric 5x5 on (s,d,o,k,v): index of (i,j)
__host__ __device__ constexpr int s5(int i, int j) {
    return i <= j ? i * 5 - i * (i - 1) / 2 + (j - i) : j * 5 - j * (j - 1) / 2 + (i - j);
}

// two doubles from a 16-B aligned LDS address: one ds_read_b128
__device__ __forceinline__ void ld2(const double* p, double& a, double& b) {
    const double2 v = *reinterpret_cast<const double2*>(p);
    a = v.x;
    b = v.y;
}
__device__ __forceinline__ void ld_a5(const double* p, double a[5]) {
    double pad;
    ld2(p, a[0], a[1]);
    ld2(p + 2, a[2], a[3]);
    ld2(p + 4, a[4], pad);
}
// Software pipeline of the stage recursions: every step starts with a full LDS wait (the data of
// this step, prefetched one step earlier), then issues the next step's loads, then computes.  The
// sched barriers keep the compiler from sinking the prefetch to the end of the step (where the next
// wait would expose its whole latency) or hoisting it above the wait.
__device__ __forceinline__ void lds_fence() {
    __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0), vmcnt/expcnt untouched
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void sched_fence() { __builtin_amdgcn_sched_barrier(0); }
