// traffic_kernels.h -- the kernels around the solve in the closed-loop traffic scripts (mpc_closed_loop_traffic):
// sweep_kernels.h's initialisation and FSM step with a script of A actors per ego instead of one car and one
// light, and a gather that packs the A-wide obstacle slab.  Each actor runs the per-obstacle state machine of
// ObstaclesFSM.update on its own state (loop_steps.h, actor_step).  The compaction kernel, the plant kernel (with the
// plant-side quantities and the kept hist_x / hist_u / hist_status) and the solver launch are the sweep's,
// unchanged.
#pragma once
#include "sweep_kernels.h"

// One thread per ego; the per-actor state is actor-major ([A][B]) so that the threads of a wave touch
// neighbouring addresses for every actor, and so are the slab the FSM step writes and the extras.
struct TrState {
    const mpc_actor* actors;   // [B][A] (per_ego) or [A] (one shared script)
    int per_ego;
    double* aval;              // [A][B] car: position; light: timer
    int* aflags;               // [A][B] ACT_* bits (loop_steps.h)
    double* slab;              // [A][2][B] this step's slab of every ego (entry j: rows 2j, 2j + 1)
    double* ex;                // [MPC_TR_NX][B] extras (an EgoCols like SwState::q)
    // histories of the selected egos beyond SwState's; either may be null
    int* hist_nobs;            // [n_hist][max_steps]
    double* hist_slab;         // [n_hist][max_steps][A][2]
};

// sw_init_kernel with ego b's script: a car starts at its pos_s, a light at timer 0, every flag clear
__global__ void __launch_bounds__(256) tr_init_kernel(int B, int A, ClState C, SwState S, TrState T,
                                                      const double* __restrict__ x_init, double s_stop,
                                                      int max_steps) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int h = S.hslot[b];
    for (int j = 0; j < 5; ++j) {
        C.x[5 * (size_t)b + j] = x_init[5 * (size_t)b + j];
        if (h >= 0 && S.hist_x) S.hist_x[(size_t)h * (max_steps + 1) * 5 + j] = x_init[5 * (size_t)b + j];
    }
    C.active[b] = x_init[5 * (size_t)b] <= s_stop ? 1 : 0;
    const mpc_actor* sc = T.actors + (T.per_ego ? (size_t)b * A : 0);
    for (int a = 0; a < A; ++a) {
        T.aval[(size_t)a * B + b] = sc[a].kind == MPC_ACTOR_CAR ? sc[a].pos_s : 0.0;
        T.aflags[(size_t)a * B + b] = 0;
    }
    C.nobs[b] = 0;
    S.n_steps[b] = 0;
    S.qflags[b] = 0;
    quant_init(EgoCols{S.q, (size_t)B, (size_t)b}, b, x_init[5 * (size_t)b], x_init[5 * (size_t)b + 1]);
    const EgoCols ex{T.ex, (size_t)B, (size_t)b};
    ex[MPC_TRX_MAX_NOBS] = 0.0;
    ex[MPC_TRX_N_RED_PASS] = 0.0;
    ex[MPC_TRX_MIN_GAP_ACTOR] = -1.0;
}

// actor_step per actor, in index order, on the state before the step; the slab takes what the actors emit in that
// order.  The gap and red-pass quantities are the sweep's, over every car / every light
__global__ void __launch_bounds__(256) tr_fsm_kernel(int B, int A, double dt, ClState C, SwState S, TrState T,
                                                     int step, int max_steps) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (!C.active[b]) { C.nobs[b] = 0; return; }
    const double s = C.x[5 * (size_t)b], v = C.x[5 * (size_t)b + 4];
    const mpc_actor* sc = T.actors + (T.per_ego ? (size_t)b * A : 0);
    const int h = S.hslot[b];
    double* hslab = h >= 0 && T.hist_slab ? T.hist_slab + ((size_t)h * max_steps + step) * A * 2 : nullptr;
    const EgoCols q{S.q, (size_t)B, (size_t)b}, ex{T.ex, (size_t)B, (size_t)b};
    int n = 0, green = 0, n_red = 0, have_car = 0;
    double car_s = NAN;
    int qf = S.qflags[b];
    const int qf0 = qf;
    double gmin = q[MPC_CLQ_MIN_OBS_DIST];
    int gact = -1;                                   // the actor that replaced the minimum at this step
    for (int a = 0; a < A; ++a) {
        const int kind = sc[a].kind;
        if (kind == MPC_ACTOR_NONE) continue;
        const size_t ia = (size_t)a * B + b;
        int fl = T.aflags[ia];
        const int fl0 = fl;
        double os, ov;
        const int r = actor_step(sc[a], dt, s, v, fl, T.aval[ia], os, ov);
        if (fl != fl0) T.aflags[ia] = fl;
        if (r & ACTOR_GREEN) green |= 1 << a;
        if (r & ACTOR_RAN_RED) ++n_red;
        if (!(r & ACTOR_EMITS)) continue;
        T.slab[(size_t)(2 * n) * B + b] = os;        // n < A: every actor emits at most once
        T.slab[(size_t)(2 * n + 1) * B + b] = ov;
        if (hslab) { hslab[2 * n] = os; hslab[2 * n + 1] = ov; }
        ++n;
        if (kind != MPC_ACTOR_CAR) continue;
        if (!have_car) { have_car = 1; car_s = os; }
        if (os == os && min_gap(gmin, qf, os - s)) gact = a;   // a recorded car position
    }
    C.nobs[b] = n;
    if (gact >= 0) {
        q[MPC_CLQ_MIN_OBS_DIST] = gmin;
        ex[MPC_TRX_MIN_GAP_ACTOR] = (double)gact;
    }
    if (qf != qf0) S.qflags[b] = qf;
    if (n_red) {
        q[MPC_CLQ_RED_PASS] = 1.0;
        ex[MPC_TRX_N_RED_PASS] += (double)n_red;
    }
    if ((double)n > ex[MPC_TRX_MAX_NOBS]) ex[MPC_TRX_MAX_NOBS] = (double)n;
    if (h >= 0) {
        if (S.hist_obs_s) S.hist_obs_s[(size_t)h * max_steps + step] = car_s;
        if (S.hist_tl) S.hist_tl[(size_t)h * max_steps + step] = green;
        if (T.hist_nobs) T.hist_nobs[(size_t)h * max_steps + step] = n;
    }
}

// cl_gather_kernel for an A-wide slab: slot i <- ego alist[i], its state and its n_obs slab entries (zeros past
// them).  C.obsa is [nl][A][2], the solver's obs + i * max_obs * 2 with max_obs = A
__global__ void __launch_bounds__(256) tr_gather_kernel(int nl, int B, int A, ClState C, TrState T) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nl) return;
    const int e = C.alist[i];
    for (int j = 0; j < 5; ++j) C.xa[5 * (size_t)i + j] = C.x[5 * (size_t)e + j];
    const int n = C.nobs[e];
    double* o = C.obsa + (size_t)i * A * 2;
    for (int j = 0; j < A; ++j) {
        o[2 * j] = j < n ? T.slab[(size_t)(2 * j) * B + e] : 0.0;
        o[2 * j + 1] = j < n ? T.slab[(size_t)(2 * j + 1) * B + e] : 0.0;
    }
    C.nobsa[i] = n;
}
