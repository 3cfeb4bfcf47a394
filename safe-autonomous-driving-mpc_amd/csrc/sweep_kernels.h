// sweep_kernels.h -- the kernels around the solve in the closed-loop scenario sweep (mpc_closed_loop_sweep):
// closed_loop_kernels.h's initialisation, FSM and plant step with a scenario per ego, the acceptance-check
// quantities (include/mpcqp.h, MPC_CLQ_*) accumulated in place, and history rows for the selected egos only.
// The compaction and gather kernels and the solver launch are those of the closed loop, unchanged.
#pragma once
#include "closed_loop_kernels.h"

// One thread per ego like the kernels they restate.  Every quantity is a running min, max, count or a single
// subtraction of values the loop already forms, so a row equals shard.closed_loop_quantities on the ego's
// full histories bit for bit.  The comparisons are written so that a NaN operand enters the extreme and then
// stays (numpy's max / min): `a > m || a != a` takes a NaN a, and a NaN m fails both tests for every later a.
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

#define SW_Q(S, col, B, b) (S).q[(size_t)(col) * (size_t)(B) + (size_t)(b)]

// cl_init_kernel with ego b's scenario (PER_EGO: Fs[b], else the shared F) and the accumulators: an ego that
// never runs keeps this row (its initial s and |d|, zeros, a NaN gap: closed_loop_quantities' n_steps == 0 row)
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
    for (int k = 0; k < MPC_CL_NQ; ++k) SW_Q(S, k, B, b) = 0.0;
    SW_Q(S, MPC_CLQ_EGO, B, b) = (double)b;
    SW_Q(S, MPC_CLQ_S_FINAL, B, b) = x_init[5 * (size_t)b];
    SW_Q(S, MPC_CLQ_MAX_DEV, B, b) = fabs(x_init[5 * (size_t)b + 1]);
    SW_Q(S, MPC_CLQ_MIN_OBS_DIST, B, b) = NAN;
}

// cl_fsm_kernel's transitions on ego b's own scenario, plus the two quantities that need this step's FSM
// outputs together with the state before the step: the gap to the car (hist_obs_s[i] - hist_x[i, 0]) and the
// red-light pass (the light at the first step that starts past tl_pos)
template <bool PER_EGO>
__global__ void __launch_bounds__(256) sw_fsm_kernel(int B, mpc_fsm F, const mpc_fsm* __restrict__ Fs, double dt,
                                                     ClState C, SwState S, int step, int max_steps) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (!C.active[b]) { C.nobs[b] = 0; return; }
    if (PER_EGO) F = Fs[b];
    const double s = C.x[5 * (size_t)b], v = C.x[5 * (size_t)b + 4];
    int* fl = C.fsm_flags + 4 * (size_t)b;
    double* o = C.obs + 4 * (size_t)b;
    int n = 0;
    double car_s = NAN;
    if (F.dynamic_obstacle) {
        if (!fl[1] && s >= F.obs_trigger_s) { fl[1] = 1; fl[0] = 1; }
        if (fl[0]) {
            const double os = C.obs_s[b] + F.obs_v * dt;
            C.obs_s[b] = os;
            if (os > F.obs_end_s) {
                fl[0] = 0;
            } else {
                o[0] = os;
                o[1] = F.obs_v;
                n = 1;
                car_s = os;
            }
        }
    }
    if (F.traffic_light && !fl[2]) {
        const double dist = F.tl_pos - s;
        if (0.0 < dist && dist < F.tl_trigger_s) {
            o[2 * n] = F.tl_pos;
            o[2 * n + 1] = 0.0;
            ++n;
            if (v < 0.1 && dist < 10.0) fl[3] = 1;
        }
        if (fl[3]) {
            C.tl_timer[b] += dt;
            if (C.tl_timer[b] >= F.tl_stop_duration) { fl[2] = 1; fl[3] = 0; }
        }
    }
    C.nobs[b] = n;
    const int green = fl[2];
    int qf = S.qflags[b];
    const int qf0 = qf;
    if (car_s == car_s) {                       // a recorded car position (NaN: none this step)
        const double g = car_s - s;
        if (!(qf & 1)) {
            SW_Q(S, MPC_CLQ_MIN_OBS_DIST, B, b) = g;
            qf |= 1;
        } else {
            const double m = SW_Q(S, MPC_CLQ_MIN_OBS_DIST, B, b);
            if (g < m || g != g) SW_Q(S, MPC_CLQ_MIN_OBS_DIST, B, b) = g;
        }
    }
    if (F.traffic_light && !(qf & 2) && s > F.tl_pos) {
        qf |= 2;
        if (!green) SW_Q(S, MPC_CLQ_RED_PASS, B, b) = 1.0;
    }
    if (qf != qf0) S.qflags[b] = qf;
    const int h = S.hslot[b];
    if (h >= 0) {
        if (S.hist_obs_s) S.hist_obs_s[(size_t)h * max_steps + step] = car_s;
        if (S.hist_tl) S.hist_tl[(size_t)h * max_steps + step] = green;
    }
}

// cl_plant_kernel's step for the listed egos, with the running extremes of the state and the control and the
// status counters.  Every ego that runs at all runs step 0, which seeds the control extremes
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
    const double xd[5] = {x[4], x[4] * x[2], x[4] * (x[3] - st[3]), u1, u2};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        x[j] = x[j] + dt * xd[j];
        C.x[5 * (size_t)b + j] = x[j];
        if (h >= 0 && S.hist_x) S.hist_x[((size_t)h * (max_steps + 1) + step + 1) * 5 + j] = x[j];
    }
    const int status = C.sta[i];
    if (h >= 0) {
        if (S.hist_u) {
            S.hist_u[((size_t)h * max_steps + step) * 2] = u1;
            S.hist_u[((size_t)h * max_steps + step) * 2 + 1] = u2;
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
    } else {
        const double a0 = SW_Q(S, MPC_CLQ_U1_MIN, B, b), a1 = SW_Q(S, MPC_CLQ_U1_MAX, B, b);
        const double b0 = SW_Q(S, MPC_CLQ_U2_MIN, B, b), b1 = SW_Q(S, MPC_CLQ_U2_MAX, B, b);
        if (u1 < a0 || u1 != u1) SW_Q(S, MPC_CLQ_U1_MIN, B, b) = u1;
        if (u1 > a1 || u1 != u1) SW_Q(S, MPC_CLQ_U1_MAX, B, b) = u1;
        if (u2 < b0 || u2 != u2) SW_Q(S, MPC_CLQ_U2_MIN, B, b) = u2;
        if (u2 > b1 || u2 != u2) SW_Q(S, MPC_CLQ_U2_MAX, B, b) = u2;
    }
    const int code = status & MPC_STATUS_MASK;
    if (code == MPC_INFEASIBLE) SW_Q(S, MPC_CLQ_N_INFEASIBLE, B, b) += 1.0;
    if (code != MPC_OK) SW_Q(S, MPC_CLQ_N_NOT_OK, B, b) += 1.0;
    if (!(x[0] <= s_stop)) C.active[b] = 0;
    else atomicAdd(C.n_active, 1);
}
