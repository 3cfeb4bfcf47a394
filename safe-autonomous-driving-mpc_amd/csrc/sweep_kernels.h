// sweep_kernels.h -- the kernels around the solve in the closed-loop scenario sweep (mpc_closed_loop_sweep):
// closed_loop_kernels.h's initialisation, FSM and plant step with a scenario per ego, the acceptance-check
// quantities (include/mpcqp.h, MPC_CLQ_*) accumulated in place, and history rows for the selected egos only.
// The steps and the quantity rules themselves are loop_steps.h's, shared with the host backend.
// The compaction and gather kernels and the solver launch are those of the closed loop, unchanged.
#pragma once
#include "closed_loop_kernels.h"

// One thread per ego like the closed loop's kernels.  Every quantity is a running min, max, count or a single
// subtraction of values the loop already forms, so a row equals shard.closed_loop_quantities on the ego's
// full histories bit for bit (the extremes keep a NaN like numpy's max / min: loop_steps.h, keep_min).
struct SwState {
    double* q;          // [MPC_CL_NQ][B] quantities, one coalesced row per column (transposed on the way out)
    int* qflags;        // [B] bit 0: a car gap was recorded; bit 1: the red-pass question is decided
    const int* hslot;   // [B] row of this ego in the history arrays, -1: not kept
    int* n_steps;       // [B]
    // histories of the selected egos, mpc_closed_loop's per-ego layout ([n_hist][max_steps (+1)][..]); any may
    // be null
    double* hist_x;
    double* hist_u;
    double* hist_obs_s;
    int* hist_tl;
    int* hist_status;
};

// ego b's columns of a field-major array [cols][B]: the accessor loop_steps.h's quantity functions take
struct EgoCols {
    double* p;
    size_t B, b;
    __device__ __forceinline__ double& operator[](int col) const { return p[(size_t)col * B + b]; }
};

// cl_init_kernel with ego b's scenario (PER_EGO: Fs[b], else the shared F) and the initial quantity row
template <bool PER_EGO>
__global__ void __launch_bounds__(256) sw_init_kernel(int B, mpc_fsm F, const mpc_fsm* __restrict__ Fs, ClState C,
                                                      SwState S, const double* __restrict__ x_init, double s_stop,
                                                      int max_steps) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int h = S.hslot[b];
    for (int j = 0; j < 5; ++j) {
        C.x[5 * (size_t)b + j] = x_init[5 * (size_t)b + j];
        if (h >= 0 && S.hist_x) S.hist_x[(size_t)h * (max_steps + 1) * 5 + j] = x_init[5 * (size_t)b + j];
    }
    C.active[b] = x_init[5 * (size_t)b] <= s_stop ? 1 : 0;
    C.obs_s[b] = PER_EGO ? Fs[b].obs_start_s : F.obs_start_s;
    C.tl_timer[b] = 0.0;
    for (int j = 0; j < 4; ++j) C.fsm_flags[4 * (size_t)b + j] = 0;
    for (int j = 0; j < 4; ++j) C.obs[4 * (size_t)b + j] = 0.0;
    C.nobs[b] = 0;
    S.n_steps[b] = 0;
    S.qflags[b] = 0;
    quant_init(EgoCols{S.q, (size_t)B, (size_t)b}, b, x_init[5 * (size_t)b], x_init[5 * (size_t)b + 1]);
}

// cl_fsm_kernel on ego b's own scenario, plus the two quantities that need this step's FSM outputs together with
// the state before the step: the gap to the car (hist_obs_s[i] - hist_x[i, 0]) and the red-light pass (the light
// at the first step that starts past tl_pos)
template <bool PER_EGO>
__global__ void __launch_bounds__(256) sw_fsm_kernel(int B, mpc_fsm F, const mpc_fsm* __restrict__ Fs, double dt,
                                                     ClState C, SwState S, int step, int max_steps) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (!C.active[b]) { C.nobs[b] = 0; return; }
    if (PER_EGO) F = Fs[b];
    const double s = C.x[5 * (size_t)b], v = C.x[5 * (size_t)b + 4];
    int* fl = C.fsm_flags + 4 * (size_t)b;
    double car_s;
    C.nobs[b] = fsm_step(F, dt, s, v, fl, C.obs_s[b], C.tl_timer[b], C.obs + 4 * (size_t)b, car_s);
    const int green = fl[2];
    const EgoCols q{S.q, (size_t)B, (size_t)b};
    int qf = S.qflags[b];
    const int qf0 = qf;
    if (car_s == car_s) min_gap(q[MPC_CLQ_MIN_OBS_DIST], qf, car_s - s);   // NaN: no car this step
    red_pass_step(F, s, green, q, qf);
    if (qf != qf0) S.qflags[b] = qf;
    const int h = S.hslot[b];
    if (h >= 0) {
        if (S.hist_obs_s) S.hist_obs_s[(size_t)h * max_steps + step] = car_s;
        if (S.hist_tl) S.hist_tl[(size_t)h * max_steps + step] = green;
    }
}

// what a plant step leaves of ego b besides its quantities: the new state x, the kept history rows (slot h) with
// the commanded control, n_steps, and whether the ego stays in the loop
__device__ __forceinline__ void sw_plant_store(const ClState& C, const SwState& S, int b, int h, const double* x,
                                               double u1, double u2, int status, double s_stop, int step,
                                               int max_steps) {
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        C.x[5 * (size_t)b + j] = x[j];
        if (h >= 0 && S.hist_x) S.hist_x[((size_t)h * (max_steps + 1) + step + 1) * 5 + j] = x[j];
    }
    if (h >= 0) {
        if (S.hist_u) {
            S.hist_u[((size_t)h * max_steps + step) * 2] = u1;
            S.hist_u[((size_t)h * max_steps + step) * 2 + 1] = u2;
        }
        if (S.hist_status) S.hist_status[(size_t)h * max_steps + step] = status;
    }
    S.n_steps[b] = step + 1;
    if (!(x[0] <= s_stop)) C.active[b] = 0;
    else atomicAdd(C.n_active, 1);
}

// cl_plant_kernel's step for the listed egos, with the plant-side quantities
__global__ void __launch_bounds__(256) sw_plant_kernel(DevTable tab, int B, int nl, double dt, ClState C, SwState S,
                                                       double s_stop, int step, int max_steps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nl) return;
    const int b = C.alist[i];
    if (!C.active[b]) return;
    const int h = S.hslot[b];
    double x[5], st[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) x[j] = C.x[5 * (size_t)b + j];
    const double u1 = C.u0a[2 * (size_t)i], u2 = C.u0a[2 * (size_t)i + 1];
    get_state(tab, x[0], st, nullptr);
    plant_step(x, dt, u1, u2, st[3]);
    const int status = C.sta[i];
    plant_quant(EgoCols{S.q, (size_t)B, (size_t)b}, step, x, u1, u2, status);
    sw_plant_store(C, S, b, h, x, u1, u2, status, s_stop, step, max_steps);
}
