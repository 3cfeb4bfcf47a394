// noise_kernels.h -- the kernels of the closed-loop disturbance sweeps (mpc_closed_loop_noisy, mpc_noise_draw):
// the convoy loop with seeded noise between the world and the solver.  nz_measure_kernel takes tr_gather_kernel's
// place (the state and the slab copy the solver receives, perturbed on the way), nz_plant_kernel takes
// sw_plant_kernel's (the applied control perturbed and clamped, the process draw, the applied-control extras).
// The FSM step, the leader ranking, the compaction and the solver launch are the convoy entry's, unchanged, and
// they read the true states only.
#pragma once
#include "convoy_kernels.h"

// The noise source (include/mpcqp.h): stateless Philox4x32-10, one block per variate.  Integer arithmetic and
// single rounded FP64 operations only (the build has -ffp-contract=off), so a draw is the same bits on the device,
// on the host backend and in numpy.
#define NZ_M0 0xD2511F53u
#define NZ_M1 0xCD9E8D57u
#define NZ_W0 0x9E3779B9u
#define NZ_W1 0xBB67AE85u
#define NZ_C (1.7320508075688772 * 0x1p-32)    // the double nearest sqrt(3), scaled exactly

__device__ __forceinline__ void nz_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                          unsigned k1, unsigned w[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(NZ_M0, c0), lo0 = NZ_M0 * c0;
        const unsigned hi1 = __umulhi(NZ_M1, c2), lo1 = NZ_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += NZ_W0;
        k1 += NZ_W1;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// the variate of four words: the sum is an exact integer below 2^34, the subtraction is exact, one rounding
__device__ __forceinline__ double nz_variate(const unsigned w[4]) {
    const unsigned long long s = (unsigned long long)w[0] + w[1] + w[2] + w[3];
    return ((double)s - 8589934590.0) * NZ_C;
}

__device__ __forceinline__ double nz_z(unsigned k0, unsigned k1, unsigned long long g, int step, int channel) {
    unsigned w[4];
    nz_philox((unsigned)g, (unsigned)(g >> 32), (unsigned)step, (unsigned)channel, k0, k1, w);
    return nz_variate(w);
}

// rows of the per-ego sigma table: mpc_noise's fields in its order
#define NZ_MEAS 0
#define NZ_ACT 5
#define NZ_PROC 7
#define NZ_PERC 12
#define NZ_NSIG 14

struct NzState {
    const double* sig;         // [NZ_NSIG][B] per-ego sigmas, field-major like TrState::aval; null: `shared`
    mpc_noise shared;
    unsigned k0, k1;           // the key: the seed's halves
    unsigned long long g0;     // ego_offset: ego b draws as global ego g0 + b
    double u_min0, u_min1, u_max0, u_max1;
    // histories of the selected egos; either may be null
    double* hist_ua;           // [n_hist][max_steps][2]
    double* hist_xm;           // [n_hist][max_steps][5]
};

// sigma `f` (a compile-time row once the loops are unrolled) of ego b
__device__ __forceinline__ double nz_sigma(const NzState& Z, int f, int B, int b) {
    if (Z.sig) return Z.sig[(size_t)f * B + b];
    return f < NZ_ACT ? Z.shared.meas_sigma[f]
         : f < NZ_PROC ? Z.shared.act_sigma[f - NZ_ACT]
         : f < NZ_PERC ? Z.shared.proc_sigma[f - NZ_PROC] : Z.shared.perc_sigma[f - NZ_PERC];
}

// the noise extras of every ego before the first step (tr_init_kernel and cv_init_kernel seed columns 0..5;
// T.ex is [MPC_NZ_NX][B] here)
__global__ void __launch_bounds__(256) nz_init_kernel(int B, TrState T) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
#pragma unroll
    for (int k = MPC_NZX_U1A_MIN; k < MPC_NZ_NX; ++k) TR_X(T, k, B, b) = 0.0;
}

// tr_gather_kernel with the measurement and perception draws: slot i <- ego alist[i], its state plus
// meas_sigma * z per component, and of its n_obs slab entries (s + perc_sigma[0] * z, v + perc_sigma[1] * z'),
// zeros past them.  C.x and T.slab, the truth, are only read.  An ego that left the loop since the last
// compaction is still listed (its solve is dropped by the plant kernel): it is handed on as it is, draws nothing
// and records nothing
__global__ void __launch_bounds__(256) nz_measure_kernel(int nl, int B, int A, ClState C, SwState S, TrState T,
                                                         NzState Z, int step, int max_steps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nl) return;
    const int e = C.alist[i];
    const bool act = C.active[e] != 0;
    const unsigned long long g = Z.g0 + (unsigned long long)e;
    const int h = S.hslot[e];
    double* hxm = act && h >= 0 && Z.hist_xm ? Z.hist_xm + ((size_t)h * max_steps + step) * 5 : nullptr;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        double xv = C.x[5 * (size_t)e + j];
        const double sg = nz_sigma(Z, NZ_MEAS + j, B, e);
        if (act && sg != 0.0) xv = xv + sg * nz_z(Z.k0, Z.k1, g, step, MPC_NZ_CH_MEAS + j);
        C.xa[5 * (size_t)i + j] = xv;
        if (hxm) hxm[j] = xv;
    }
    const int n = C.nobs[e];
    const double sp = nz_sigma(Z, NZ_PERC, B, e), sv = nz_sigma(Z, NZ_PERC + 1, B, e);
    double* o = C.obsa + (size_t)i * A * 2;
    for (int j = 0; j < A; ++j) {                    // A <= MPC_MAX_ACTORS: channels 16 .. 47
        double os = 0.0, ov = 0.0;
        if (j < n) {
            os = T.slab[(size_t)(2 * j) * B + e];
            ov = T.slab[(size_t)(2 * j + 1) * B + e];
            if (act && sp != 0.0) os = os + sp * nz_z(Z.k0, Z.k1, g, step, MPC_NZ_CH_PERC + 2 * j);
            if (act && sv != 0.0) ov = ov + sv * nz_z(Z.k0, Z.k1, g, step, MPC_NZ_CH_PERC + 2 * j + 1);
        }
        o[2 * j] = os;
        o[2 * j + 1] = ov;
    }
    C.nobsa[i] = n;
}

// sw_plant_kernel with the actuation draw and clamp and the process draw.  The arithmetic and the quantity
// updates are that kernel's, restated: with every sigma 0 the two are the same bit for bit.  MPC_CLQ_U* and
// hist_u keep the commanded (u1, u2); the applied (ua1, ua2) go to the MPC_NZX_* extras and hist_ua
__global__ void __launch_bounds__(256) nz_plant_kernel(DevTable tab, int B, int nl, double dt, ClState C, SwState S,
                                                       TrState T, NzState Z, double s_stop, int step,
                                                       int max_steps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nl) return;
    const int b = C.alist[i];
    if (!C.active[b]) return;
    const int h = S.hslot[b];
    const unsigned long long g = Z.g0 + (unsigned long long)b;
    double x[5], st[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) x[j] = C.x[5 * (size_t)b + j];
    const double u1 = C.u0a[2 * (size_t)i], u2 = C.u0a[2 * (size_t)i + 1];
    double ua1 = u1, ua2 = u2;
    bool clamped = false;
    const double sa1 = nz_sigma(Z, NZ_ACT, B, b), sa2 = nz_sigma(Z, NZ_ACT + 1, B, b);
    if (sa1 != 0.0) {
        const double t = u1 + sa1 * nz_z(Z.k0, Z.k1, g, step, MPC_NZ_CH_ACT);
        ua1 = t < Z.u_min0 ? Z.u_min0 : (t > Z.u_max0 ? Z.u_max0 : t);
        clamped = clamped || t < Z.u_min0 || t > Z.u_max0;
    }
    if (sa2 != 0.0) {
        const double t = u2 + sa2 * nz_z(Z.k0, Z.k1, g, step, MPC_NZ_CH_ACT + 1);
        ua2 = t < Z.u_min1 ? Z.u_min1 : (t > Z.u_max1 ? Z.u_max1 : t);
        clamped = clamped || t < Z.u_min1 || t > Z.u_max1;
    }
    get_state(tab, x[0], st, nullptr);
    const double xd[5] = {x[4], x[4] * x[2], x[4] * (x[3] - st[3]), ua1, ua2};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        x[j] = x[j] + dt * xd[j];
        const double sp = nz_sigma(Z, NZ_PROC + j, B, b);
        if (sp != 0.0) x[j] = x[j] + (dt * sp) * nz_z(Z.k0, Z.k1, g, step, MPC_NZ_CH_PROC + j);
        C.x[5 * (size_t)b + j] = x[j];
        if (h >= 0 && S.hist_x) S.hist_x[((size_t)h * (max_steps + 1) + step + 1) * 5 + j] = x[j];
    }
    const int status = C.sta[i];
    if (h >= 0) {
        if (S.hist_u) {
            S.hist_u[((size_t)h * max_steps + step) * 2] = u1;
            S.hist_u[((size_t)h * max_steps + step) * 2 + 1] = u2;
        }
        if (Z.hist_ua) {
            Z.hist_ua[((size_t)h * max_steps + step) * 2] = ua1;
            Z.hist_ua[((size_t)h * max_steps + step) * 2 + 1] = ua2;
        }
        if (S.hist_status) S.hist_status[(size_t)h * max_steps + step] = status;
    }
    S.n_steps[b] = step + 1;
    SW_Q(S, MPC_CLQ_N_STEPS, B, b) = (double)(step + 1);
    SW_Q(S, MPC_CLQ_S_FINAL, B, b) = x[0];
    const double ad = fabs(x[1]), md = SW_Q(S, MPC_CLQ_MAX_DEV, B, b);
    if (ad > md || ad != ad) SW_Q(S, MPC_CLQ_MAX_DEV, B, b) = ad;
    if (step == 0) {
        SW_Q(S, MPC_CLQ_U1_MIN, B, b) = u1;
        SW_Q(S, MPC_CLQ_U1_MAX, B, b) = u1;
        SW_Q(S, MPC_CLQ_U2_MIN, B, b) = u2;
        SW_Q(S, MPC_CLQ_U2_MAX, B, b) = u2;
        TR_X(T, MPC_NZX_U1A_MIN, B, b) = ua1;
        TR_X(T, MPC_NZX_U1A_MAX, B, b) = ua1;
        TR_X(T, MPC_NZX_U2A_MIN, B, b) = ua2;
        TR_X(T, MPC_NZX_U2A_MAX, B, b) = ua2;
    } else {
        const double a0 = SW_Q(S, MPC_CLQ_U1_MIN, B, b), a1 = SW_Q(S, MPC_CLQ_U1_MAX, B, b);
        const double b0 = SW_Q(S, MPC_CLQ_U2_MIN, B, b), b1 = SW_Q(S, MPC_CLQ_U2_MAX, B, b);
        if (u1 < a0 || u1 != u1) SW_Q(S, MPC_CLQ_U1_MIN, B, b) = u1;
        if (u1 > a1 || u1 != u1) SW_Q(S, MPC_CLQ_U1_MAX, B, b) = u1;
        if (u2 < b0 || u2 != u2) SW_Q(S, MPC_CLQ_U2_MIN, B, b) = u2;
        if (u2 > b1 || u2 != u2) SW_Q(S, MPC_CLQ_U2_MAX, B, b) = u2;
        const double c0 = TR_X(T, MPC_NZX_U1A_MIN, B, b), c1 = TR_X(T, MPC_NZX_U1A_MAX, B, b);
        const double d0 = TR_X(T, MPC_NZX_U2A_MIN, B, b), d1 = TR_X(T, MPC_NZX_U2A_MAX, B, b);
        if (ua1 < c0 || ua1 != ua1) TR_X(T, MPC_NZX_U1A_MIN, B, b) = ua1;
        if (ua1 > c1 || ua1 != ua1) TR_X(T, MPC_NZX_U1A_MAX, B, b) = ua1;
        if (ua2 < d0 || ua2 != ua2) TR_X(T, MPC_NZX_U2A_MIN, B, b) = ua2;
        if (ua2 > d1 || ua2 != ua2) TR_X(T, MPC_NZX_U2A_MAX, B, b) = ua2;
    }
    if (clamped) TR_X(T, MPC_NZX_N_CLAMPED, B, b) += 1.0;
    const int code = status & MPC_STATUS_MASK;
    if (code == MPC_INFEASIBLE) SW_Q(S, MPC_CLQ_N_INFEASIBLE, B, b) += 1.0;
    if (code != MPC_OK) SW_Q(S, MPC_CLQ_N_NOT_OK, B, b) += 1.0;
    if (!(x[0] <= s_stop)) C.active[b] = 0;
    else atomicAdd(C.n_active, 1);
}

// mpc_noise_draw: draw i of (ego[i], step[i], channel[i]); words [n][4] and z [n], either may be null
__global__ void __launch_bounds__(256) nz_draw_kernel(int n, unsigned k0, unsigned k1,
                                                      const long long* __restrict__ ego,
                                                      const int* __restrict__ step, const int* __restrict__ channel,
                                                      unsigned* __restrict__ words, double* __restrict__ z) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long g = (unsigned long long)ego[i];
    unsigned w[4];
    nz_philox((unsigned)g, (unsigned)(g >> 32), (unsigned)step[i], (unsigned)channel[i], k0, k1, w);
    if (words) {
#pragma unroll
        for (int k = 0; k < 4; ++k) words[4 * (size_t)i + k] = w[k];
    }
    if (z) z[i] = nz_variate(w);
}
