// convoy_kernels.h -- the kernel that couples the egos of one world in the closed-loop convoys
// (mpc_closed_loop_convoy): per step it ranks a world's egos by position and hands each its nearest leaders as
// slab entries after the script entries tr_fsm_kernel wrote.  Initialisation, the per-actor FSM step, the gather
// (with A + K for A), the compaction, the plant kernel and the solver launch are the traffic entry's, unchanged.
#pragma once
#include "traffic_kernels.h"

struct CvState {
    int W, K;                  // egos per world, leaders per ego at most
    double lead_range;
    // histories of the selected egos; either may be null.  tr_fsm_kernel runs with T.hist_slab null: its rows
    // are A wide, these A + K
    double* hist_slab;         // [n_hist][max_steps][A + K][2]
    int* hist_lead;            // [n_hist][max_steps][K]
};

#define CV_INACTIVE 0x10000    // added to the index of an ego that left the loop and of padding: sorts last

// key a = (sa, ia) sorts before key b: egos in the loop first, among them the one ahead (the larger s, on equal s
// the lower index), the rest by index.  The indices are distinct, so this is a strict total order
__device__ __forceinline__ bool cv_before(double sa, int ia, double sb, int ib) {
    if ((ia | ib) & CV_INACTIVE) return ia < ib;
    return sa > sb || (sa == sb && ia < ib);
}

// One workgroup per world, 64 * ceil(W / 64) threads, thread i for ego w * W + i.  LDS: the world's (s, v) by
// ego, the (s, index) keys being sorted, and each ego's rank: 256 * (8 + 8 + 8 + 4 + 4) = 8 KiB at most.
//   1. load (s, v, active); the key of an ego outside the loop, and of the padding up to the power of two P,
//      carries CV_INACTIVE
//   2. bitonic sort of the P keys, one compare-exchange per thread and stage (P / 2 < W <= blockDim.x),
//      log2(P) (log2(P) + 1) / 2 stages with a barrier each (36 at P = 256); then rank[ego] = position
//   3. an ego in the loop at rank r reads the egos at ranks r - 1, r - 2, ..: its leaders nearest first (every
//      position below r holds an ego in the loop), at most K, until the range cut
// Every thread reaches every barrier: no early return before step 3.
__global__ void __launch_bounds__(MPC_MAX_WORLD) cv_lead_kernel(int B, int A, ClState C, SwState S, TrState T,
                                                                CvState V, int step, int max_steps) {
    __shared__ double s0[MPC_MAX_WORLD], v0[MPC_MAX_WORLD], ks[MPC_MAX_WORLD];
    __shared__ int ki[MPC_MAX_WORLD], rank[MPC_MAX_WORLD];
    const int W = V.W, K = V.K, i = threadIdx.x;
    const int base = blockIdx.x * W, b = base + i;
    int P = 1;
    while (P < W) P <<= 1;
    bool act = false;
    double s = 0.0;
    for (int t = i; t < P; t += blockDim.x) {        // P <= 256 may exceed blockDim.x (W = 129 .. 192)
        bool a = false;
        double st = 0.0, vt = 0.0;
        if (t < W && base + t < B) {
            a = C.active[base + t] != 0;
            st = C.x[5 * (size_t)(base + t)];
            vt = C.x[5 * (size_t)(base + t) + 4];
        }
        s0[t] = st;
        v0[t] = vt;
        ks[t] = st;
        ki[t] = a ? t : (t | CV_INACTIVE);
        if (t == i) { act = a; s = st; }
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (i < (P >> 1)) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const double sl = ks[lo], sh = ks[hi];
                const int il = ki[lo], ih = ki[hi];
                const bool up = (lo & k) == 0;       // this run ends up in order; the next one reversed
                if (up ? cv_before(sh, ih, sl, il) : cv_before(sl, il, sh, ih)) {
                    ks[lo] = sh; ki[lo] = ih;
                    ks[hi] = sl; ki[hi] = il;
                }
            }
            __syncthreads();
        }
    }
    for (int t = i; t < P; t += blockDim.x) {
        const int e = ki[t];
        if (!(e & CV_INACTIVE)) rank[e] = t;
    }
    __syncthreads();
    if (i >= W || b >= B || !act) return;
    const int r = rank[i], n0 = C.nobs[b], AK = A + K;
    const int h = S.hslot[b];
    const size_t hrow = h >= 0 ? (size_t)h * max_steps + step : 0;
    double* hslab = h >= 0 && V.hist_slab ? V.hist_slab + hrow * AK * 2 : nullptr;
    int* hlead = h >= 0 && V.hist_lead ? V.hist_lead + hrow * K : nullptr;
    if (hslab)
        for (int j = 0; j < n0; ++j) {               // the script's entries, as tr_fsm_kernel left them
            hslab[2 * j] = T.slab[(size_t)(2 * j) * B + b];
            hslab[2 * j + 1] = T.slab[(size_t)(2 * j + 1) * B + b];
        }
    const EgoCols q{S.q, (size_t)B, (size_t)b}, ex{T.ex, (size_t)B, (size_t)b};
    int qf = S.qflags[b];
    const int qf0 = qf;
    double gmin = q[MPC_CLQ_MIN_OBS_DIST];
    double lmin = ex[MPC_CVX_MIN_LEAD_GAP];
    int lf = ex[MPC_CVX_MIN_LEAD_EGO] >= 0.0;        // bit 0: a leader gap was recorded
    int gset = 0, lego = -1, nl = 0;
    for (; nl < K && nl < r; ++nl) {
        const int j = ki[r - 1 - nl];
        const double sj = s0[j], g = sj - s;
        if (g >= V.lead_range) break;
        const int n = n0 + nl;                       // n < A + K: n0 <= A
        const double vj = v0[j];
        T.slab[(size_t)(2 * n) * B + b] = sj;
        T.slab[(size_t)(2 * n + 1) * B + b] = vj;
        if (hslab) { hslab[2 * n] = sj; hslab[2 * n + 1] = vj; }
        if (hlead) hlead[nl] = base + j;
        if (min_gap(gmin, qf, g)) gset = 1;          // the sweep's gap rule, a leader being a car
        if (min_gap(lmin, lf, g)) lego = base + j;
    }
    const int n = n0 + nl;
    if (nl) {
        C.nobs[b] = n;
        if ((double)n > ex[MPC_TRX_MAX_NOBS]) ex[MPC_TRX_MAX_NOBS] = (double)n;
        if ((double)nl > ex[MPC_CVX_MAX_LEADERS]) ex[MPC_CVX_MAX_LEADERS] = (double)nl;
        if (h >= 0 && T.hist_nobs) T.hist_nobs[hrow] = n;
    }
    if (gset) {
        q[MPC_CLQ_MIN_OBS_DIST] = gmin;
        ex[MPC_TRX_MIN_GAP_ACTOR] = -1.0;
    }
    if (qf != qf0) S.qflags[b] = qf;
    if (lego >= 0) {
        ex[MPC_CVX_MIN_LEAD_GAP] = lmin;
        ex[MPC_CVX_MIN_LEAD_EGO] = (double)lego;
    }
}

// the three convoy extras of every ego before the first step (tr_init_kernel seeds columns 0..2)
__global__ void __launch_bounds__(256) cv_init_kernel(int B, TrState T) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const EgoCols ex{T.ex, (size_t)B, (size_t)b};
    ex[MPC_CVX_MIN_LEAD_GAP] = NAN;
    ex[MPC_CVX_MIN_LEAD_EGO] = -1.0;
    ex[MPC_CVX_MAX_LEADERS] = 0.0;
}
