// trace_kernels.h -- the kernels of the closed-loop plan traces (mpc_closed_loop_traced): the noisy loop with the
// solver's U and Xpred of every step kept for the listed egos.  tg_gap_kernel, after the plant kernel, accumulates
// the plan-vs-outcome gaps of every ego (include/mpcqp.h, MPC_TG_*); tg_hist_kernel scatters the plans of the
// named egos into hist_pred / hist_plan.  Every other kernel of the loop is the noisy entry's, unchanged.  The ring
// slot, the pair test and the gap rules are loop_steps.h's, shared with the host backend.
#pragma once
#include "noise_kernels.h"

struct TgState {
    int N;                      // the horizon: Xpa rows are N + 1 stages, Ua rows N controls
    int n_look;
    int look[MPC_MAX_LOOK];     // the lookaheads j, each 1 .. N
    int ring0[MPC_MAX_LOOK];    // slots before lookahead i's ring: look[0] + .. + look[i - 1]
    // the solver's outputs of this step, by list position
    const double* Ua;           // [B][N][2]
    const double* Xpa;          // [B][N+1][5]
    // per ego id, so that the list compaction cannot move them; field-major like NzState::sig
    double* ring;               // [sum(look)][3][B]: (s, d, v) of stage j of the last j predictions
    double* gq;                 // [n_look][MPC_TG_NQ][B] (transposed on the way out)
    // histories of the selected egos; either may be null
    double* hist_pred;          // [n_hist][max_steps][N+1][5]
    double* hist_plan;          // [n_hist][max_steps][N][2]
};

// the gap rows of every ego before the first step (the histories are pre-filled like the other histories, and a
// ring slot is written before it is read)
__global__ void __launch_bounds__(256) tg_init_kernel(int B, TgState G) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    for (int i = 0; i < G.n_look; ++i) trace_init(EgoCols{G.gq + (size_t)i * MPC_TG_NQ * B, (size_t)B, (size_t)b});
}

// After the plant kernel of step `step`, one thread per listed ego.  An ego that ran this step (n_steps says so: one
// that left at this step is still listed, and its final state is compared; one that left earlier is skipped) stores
// stage j of this step's prediction in its ring for j and compares its new true state with the prediction made
// j - 1 steps before, for every lookahead j.  With j == 1 the two are the same slot: the prediction made at this
// step is the one compared
__global__ void __launch_bounds__(256) tg_gap_kernel(int nl, int B, ClState C, SwState S, TgState G, int step) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nl) return;
    const int b = C.alist[i];
    if (S.n_steps[b] != step + 1) return;
    const double xs = C.x[5 * (size_t)b], xd = C.x[5 * (size_t)b + 1], xv = C.x[5 * (size_t)b + 4];
    const double* P = G.Xpa + (size_t)i * (G.N + 1) * 5;
    for (int li = 0; li < G.n_look; ++li) {
        const int j = G.look[li];
        double* ring = G.ring + (size_t)G.ring0[li] * 3 * B + b;
        const int ws = trace_slot(step, j);
        double ps = P[5 * j], pd = P[5 * j + 1], pv = P[5 * j + 4];
        ring[(size_t)(3 * ws) * B] = ps;
        ring[(size_t)(3 * ws + 1) * B] = pd;
        ring[(size_t)(3 * ws + 2) * B] = pv;
        if (!trace_pair(step, j)) continue;
        const int t0 = step + 1 - j, rs = trace_slot(t0, j);
        if (rs != ws) {
            ps = ring[(size_t)(3 * rs) * B];
            pd = ring[(size_t)(3 * rs + 1) * B];
            pv = ring[(size_t)(3 * rs + 2) * B];
        }
        trace_gap(EgoCols{G.gq + (size_t)li * MPC_TG_NQ * B, (size_t)B, (size_t)b}, t0, ps, pd, pv, xs, xd, xv);
    }
}

// After the plant kernel of step `step`, one thread per (listed ego, element) of the 5 (N + 1) + 2 N elements of a
// plan, so the copies of a named ego coalesce and an ego without a history slot costs its threads the two index
// loads and an exit.  Rows of an ego that did not run this step stay NaN
__global__ void __launch_bounds__(256) tg_hist_kernel(int nl, ClState C, SwState S, TgState G, int step,
                                                      int max_steps) {
    const int nx = 5 * (G.N + 1), ne = nx + 2 * G.N;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)nl * ne) return;
    const int i = (int)(t / ne), e = (int)(t % ne);
    const int b = C.alist[i];
    const int h = S.hslot[b];
    if (h < 0 || S.n_steps[b] != step + 1) return;
    const size_t row = (size_t)h * max_steps + step;
    if (e < nx) {
        if (G.hist_pred) G.hist_pred[row * nx + e] = G.Xpa[(size_t)i * nx + e];
    } else if (G.hist_plan) {
        G.hist_plan[row * 2 * G.N + (e - nx)] = G.Ua[(size_t)i * 2 * G.N + (e - nx)];
    }
}
