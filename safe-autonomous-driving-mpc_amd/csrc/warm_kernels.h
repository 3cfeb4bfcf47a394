// warm_kernels.h -- the kernels of the closed-loop warm starts (mpc_closed_loop_warm): the traced loop whose solver
// is handed an explicit ubar, the ego's previous plan shifted by one stage or the reference warm start restated.
// ws_carry_kernel, between the measure kernel and the solve, builds the packed ubar of the listed egos;
// ws_keep_kernel, after the plant kernel, keeps what the solver returned and accumulates the MPC_WQ_* columns.
// Every other kernel of the loop is the traced entry's, unchanged.  One thread per listed ego: the reference warm
// start is sequential in the stage.  The warm start, the reset test, the carry rule and the move accumulation are
// loop_steps.h's, shared with the host backend.
#pragma once
#include "trace_kernels.h"

struct WsState {
    mpc_warm warm;
    int N, max_obs;             // the horizon; the slab width the solver runs with (0: without a slab)
    double dt, brake_distance, brake_accel;
    double u_min0, u_min1, u_max0, u_max1;
    // by list position
    double* ubara;              // [B][N][2] the ubar the solver is handed
    const double* Ua;           // [B][N][2] the solver's U of this step
    // per ego id, so that the list compaction cannot move them; field-major so the loads of a wave coalesce
    double* plan;               // [2 N][B] the kept plan
    int* status;                // [B] the kept status, -1 before the ego's first solve
    int* nobs;                  // [B] the n_obs of the kept step
    double* wq;                 // [MPC_WQ_NQ][B] (transposed on the way out)
    double* hist_ubar;          // [n_hist][max_steps][N][2], may be null
};

// get_control on the device table, as loop_steps.h's warm_ref_control takes it
struct DevControl {
    const DevTable& tab;
    __device__ __forceinline__ void operator()(double s, double* ur) const { get_control(tab, s, ur); }
};

// the warm rows and the kept status of every ego before the first step (the kept plan and n_obs are written before
// they are read)
__global__ void __launch_bounds__(256) ws_init_kernel(int B, WsState Ws) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    warm_init(EgoCols{Ws.wq, (size_t)B, (size_t)b});
    Ws.status[b] = -1;
}

// After the measure kernel of step `step`: ubar of slot i (ego alist[i]) from the state and the slab the solver is
// about to read.  An ego that left the loop since the last compaction is still listed (its solve is dropped by the
// plant kernel): it gets the reference warm start, what the solver would have used, and records nothing
__global__ void __launch_bounds__(256) ws_carry_kernel(DevTable tab, int nl, int B, ClState C, SwState S, WsState Ws,
                                                       int step, int max_steps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nl) return;
    const int b = C.alist[i];
    const bool act = C.active[b] != 0;
    const int N = Ws.N;
    int nobs = Ws.max_obs > 0 ? C.nobsa[i] : 0;
    nobs = nobs < 0 ? 0 : (nobs > Ws.max_obs ? Ws.max_obs : nobs);
    const double* obs = C.obsa + (size_t)i * Ws.max_obs * 2;
    const int kept = act ? Ws.status[b] : -1;
    bool finite = true;
    if (kept >= 0 && Ws.warm.mode == MPC_WARM_CARRY)
        for (int e = 0; e < 2 * N; ++e) finite = finite && warm_finite(Ws.plan[(size_t)e * B + b]);
    const bool reset = warm_reset(Ws.warm, kept, finite, kept >= 0 ? Ws.nobs[b] : 0, nobs);
    const int h = S.hslot[b];
    double* hub = act && h >= 0 && Ws.hist_ubar ? Ws.hist_ubar + ((size_t)h * max_steps + step) * 2 * N : nullptr;
    double* ub = Ws.ubara + (size_t)i * 2 * N;
    WarmRef w = warm_ref_begin(C.xa + 5 * (size_t)i);
    // a carried ubar takes the reference's last stage only, and that one only under MPC_WTAIL_REFERENCE
    const bool walk = reset || Ws.warm.tail == MPC_WTAIL_REFERENCE;
    for (int k = 0; k < N; ++k) {
        const int src = reset ? -1 : warm_source(k, N, Ws.warm.tail);
        if (walk) warm_ref_advance(w, k, Ws.dt, obs, nobs, Ws.brake_distance);
        double u1, u2;
        if (src < 0) {
            warm_ref_control(w, Ws.brake_accel, DevControl{tab}, u1, u2);
        } else {
            u1 = clamp_control(Ws.plan[(size_t)(2 * src) * B + b], Ws.u_min0, Ws.u_max0);
            u2 = clamp_control(Ws.plan[(size_t)(2 * src + 1) * B + b], Ws.u_min1, Ws.u_max1);
        }
        ub[2 * k] = u1;
        ub[2 * k + 1] = u2;
        if (hub) {
            hub[2 * k] = u1;
            hub[2 * k + 1] = u2;
        }
    }
    if (act && reset) {
        const EgoCols wq{Ws.wq, (size_t)B, (size_t)b};
        wq[MPC_WQ_N_RESET] += 1.0;
    }
}

// After the plant kernel of step `step`, one thread per listed ego.  An ego that ran this step (n_steps says so, as
// in tg_gap_kernel) keeps the solver's U exactly as returned, its status and the n_obs the solver was handed, and
// its move from the ubar of this step enters its warm row
__global__ void __launch_bounds__(256) ws_keep_kernel(int nl, int B, ClState C, SwState S, WsState Ws, int step) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nl) return;
    const int b = C.alist[i];
    if (S.n_steps[b] != step + 1) return;
    const int N = Ws.N;
    const double* U = Ws.Ua + (size_t)i * 2 * N;
    const double* ub = Ws.ubara + (size_t)i * 2 * N;
    double move = 0.0;
    for (int e = 0; e < 2 * N; ++e) {
        const double u = U[e];
        Ws.plan[(size_t)e * B + b] = u;
        warm_move_element(move, u, ub[e]);
    }
    Ws.status[b] = C.sta[i];
    int nobs = Ws.max_obs > 0 ? C.nobsa[i] : 0;
    Ws.nobs[b] = nobs < 0 ? 0 : (nobs > Ws.max_obs ? Ws.max_obs : nobs);
    warm_move(EgoCols{Ws.wq, (size_t)B, (size_t)b}, step, move);
}
