// noise_kernels.h -- the kernels of the closed-loop disturbance sweeps (mpc_closed_loop_noisy, mpc_noise_draw):
// the convoy loop with seeded noise between the world and the solver.  nz_measure_kernel takes tr_gather_kernel's
// place (the state and the slab copy the solver receives, perturbed on the way), nz_plant_kernel takes
// sw_plant_kernel's (the applied control perturbed and clamped, the process draw, the applied-control extras).
// The FSM step, the leader ranking, the compaction and the solver launch are the convoy entry's, unchanged, and
// they read the true states only.
#pragma once
#include "convoy_kernels.h"

// The noise source (Philox4x32-10, the variate, the sigma application and the actuation clamp) is loop_steps.h's,
// so a draw is the same bits on the device, on the host backend and in numpy.

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
    const EgoCols ex{T.ex, (size_t)B, (size_t)b};
#pragma unroll
    for (int k = MPC_NZX_U1A_MIN; k < MPC_NZ_NX; ++k) ex[k] = 0.0;
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
    const NoiseAt at = {Z.k0, Z.k1, Z.g0 + (unsigned long long)e, step};
    const int h = S.hslot[e];
    double* hxm = act && h >= 0 && Z.hist_xm ? Z.hist_xm + ((size_t)h * max_steps + step) * 5 : nullptr;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        double xv = C.x[5 * (size_t)e + j];
        if (act) xv = noise_add(xv, nz_sigma(Z, NZ_MEAS + j, B, e), at, MPC_NZ_CH_MEAS + j);
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
            if (act) {
                os = noise_add(os, sp, at, MPC_NZ_CH_PERC + 2 * j);
                ov = noise_add(ov, sv, at, MPC_NZ_CH_PERC + 2 * j + 1);
            }
        }
        o[2 * j] = os;
        o[2 * j + 1] = ov;
    }
    C.nobsa[i] = n;
}

// sw_plant_kernel with the actuation draw and clamp and the process draw: the same plant_step, plant_quant and
// sw_plant_store, so with every sigma 0 the two are the same bit for bit.  MPC_CLQ_U* and hist_u keep the
// commanded (u1, u2); the applied (ua1, ua2) go to the MPC_NZX_* extras and hist_ua
__global__ void __launch_bounds__(256) nz_plant_kernel(DevTable tab, int B, int nl, double dt, ClState C, SwState S,
                                                       TrState T, NzState Z, double s_stop, int step,
                                                       int max_steps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nl) return;
    const int b = C.alist[i];
    if (!C.active[b]) return;
    const int h = S.hslot[b];
    const NoiseAt at = {Z.k0, Z.k1, Z.g0 + (unsigned long long)b, step};
    double x[5], st[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) x[j] = C.x[5 * (size_t)b + j];
    const double u1 = C.u0a[2 * (size_t)i], u2 = C.u0a[2 * (size_t)i + 1];
    bool clamped = false;
    const double ua1 = apply_actuation(u1, nz_sigma(Z, NZ_ACT, B, b), at, MPC_NZ_CH_ACT, Z.u_min0, Z.u_max0, clamped);
    const double ua2 = apply_actuation(u2, nz_sigma(Z, NZ_ACT + 1, B, b), at, MPC_NZ_CH_ACT + 1, Z.u_min1, Z.u_max1,
                                       clamped);
    get_state(tab, x[0], st, nullptr);
    plant_step(x, dt, ua1, ua2, st[3]);
#pragma unroll
    for (int j = 0; j < 5; ++j) x[j] = noise_add(x[j], nz_sigma(Z, NZ_PROC + j, B, b), at, MPC_NZ_CH_PROC + j, dt);
    const int status = C.sta[i];
    const EgoCols ex{T.ex, (size_t)B, (size_t)b};
    plant_quant(EgoCols{S.q, (size_t)B, (size_t)b}, step, x, u1, u2, status);
    extremes4(ex, MPC_NZX_U1A_MIN, step, ua1, ua2);
    if (clamped) ex[MPC_NZX_N_CLAMPED] += 1.0;
    if (h >= 0 && Z.hist_ua) {
        Z.hist_ua[((size_t)h * max_steps + step) * 2] = ua1;
        Z.hist_ua[((size_t)h * max_steps + step) * 2 + 1] = ua2;
    }
    sw_plant_store(C, S, b, h, x, u1, u2, status, s_stop, step, max_steps);
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
    noise_words((unsigned)g, (unsigned)(g >> 32), (unsigned)step[i], (unsigned)channel[i], k0, k1, w);
    if (words) {
#pragma unroll
        for (int k = 0; k < 4; ++k) words[4 * (size_t)i + k] = w[k];
    }
    if (z) z[i] = noise_variate(w);
}
