// closed_loop_kernels.h -- the kernels around the solve in the batched closed loop (FSM, plant, compaction,
// gather, initialisation) and the global pose kernel.
#pragma once
#include "../../include/mpcqp.h"
#include "device_common.h"
#include "loop_steps.h"

// ------------------------------------------------------------------------------------------
// batched closed loop: run_simulation, trajectory_tracking.py:377-443, per ego,
// with the ObstaclesFSM of :266-374.  One thread per ego for the FSM and the plant; the solve in
// between is the batched solver kernel.  Same arithmetic order as the reference (numpy), so a
// closed loop on the device reproduces the host loop bit for bit.
// ------------------------------------------------------------------------------------------
struct ClState {
    double* x;          // [B][5]    current state
    double* obs;        // [B][2][2] obstacle slab of this step (car first, then the light: :341-358)
    int* nobs;          // [B]
    int* active;        // [B]       still inside the loop condition s <= s_stop (:395)
    double* obs_s;      // [B]       dynamic obstacle position
    double* tl_timer;   // [B]
    int* fsm_flags;     // [B][4]    obs_active, obs_has_triggered, tl_green, tl_waiting
    int* n_active;      // [1]
    // the solver runs on the egos still in the loop only: alist [B] holds their ids (increasing, rebuilt by
    // cl_compact_kernel whenever egos have left), and the solve reads / writes the packed slabs below
    int* alist;         // [B]
    int* n_list;        // [1]
    double* xa;         // [B][5]
    double* obsa;       // [B][2][2]
    int* nobsa;         // [B]
    double* u0a;        // [B][2]
    int* sta;           // [B]
};

// ids of the egos still in the loop, in increasing order (deterministic): one workgroup of 1024 lanes,
// wave ballots and a scan of the 16 wave counts per chunk
__global__ void __launch_bounds__(1024) cl_compact_kernel(int B, ClState C) {
    __shared__ int wsum[16];
    __shared__ int base;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c0 = 0; c0 < B; c0 += 1024) {
        const int e = c0 + threadIdx.x;
        const bool f = e < B && C.active[e];
        const unsigned long long m = __ballot(f);
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int i = 0; i < w; ++i) off += wsum[i];
        if (f) C.alist[off + pre] = e;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int i = 0; i < 16; ++i) t += wsum[i];
            base += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *C.n_list = base;
}

// packs the listed egos' state and obstacle slab for the solve (slot i <- ego alist[i])
__global__ void cl_gather_kernel(int nl, ClState C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nl) return;
    const int e = C.alist[i];
    for (int j = 0; j < 5; ++j) C.xa[5 * (size_t)i + j] = C.x[5 * (size_t)e + j];
    for (int j = 0; j < 4; ++j) C.obsa[4 * (size_t)i + j] = C.obs[4 * (size_t)e + j];
    C.nobsa[i] = C.nobs[e];
}

// ObstaclesFSM.update(dt, s, v) (trajectory_tracking.py:330-374, loop_steps.h's fsm_step) for every active ego
__global__ void cl_fsm_kernel(int B, mpc_fsm F, double dt, ClState C, double* hist_obs_s, int* hist_tl, int step,
                              int max_steps) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (!C.active[b]) { C.nobs[b] = 0; return; }
    const double s = C.x[5 * (size_t)b], v = C.x[5 * (size_t)b + 4];
    int* fl = C.fsm_flags + 4 * (size_t)b;
    double car_s;
    const int n = fsm_step(F, dt, s, v, fl, C.obs_s[b], C.tl_timer[b], C.obs + 4 * (size_t)b, car_s);
    C.nobs[b] = n;
    if (hist_obs_s) hist_obs_s[(size_t)b * max_steps + step] = car_s;
    if (hist_tl) hist_tl[(size_t)b * max_steps + step] = fl[2];
}

// plant step x <- x + dt * dynamics(x, u0, k_ref(x_s)) (:403-406) and the histories (:412-421), for the
// listed egos (slot i: ego alist[i], its control at u0a[i])
__global__ void cl_plant_kernel(DevTable tab, int nl, double dt, ClState C, double s_stop, double* hist_x,
                                double* hist_u, int* hist_status, int* n_steps, int step, int max_steps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nl) return;
    const int b = C.alist[i];
    if (!C.active[b]) return;
    double x[5], st[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) x[j] = C.x[5 * (size_t)b + j];
    const double u1 = C.u0a[2 * (size_t)i], u2 = C.u0a[2 * (size_t)i + 1];
    get_state(tab, x[0], st, nullptr);
    plant_step(x, dt, u1, u2, st[3]);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        C.x[5 * (size_t)b + j] = x[j];
        if (hist_x) hist_x[((size_t)b * (max_steps + 1) + step + 1) * 5 + j] = x[j];
    }
    if (hist_u) {
        hist_u[((size_t)b * max_steps + step) * 2] = u1;
        hist_u[((size_t)b * max_steps + step) * 2 + 1] = u2;
    }
    if (hist_status) hist_status[(size_t)b * max_steps + step] = C.sta[i];
    n_steps[b] = step + 1;
    if (!(x[0] <= s_stop)) C.active[b] = 0;
    else atomicAdd(C.n_active, 1);
}

__global__ void cl_init_kernel(int B, mpc_fsm F, ClState C, const double* x_init, double s_stop, double* hist_x,
                               int* n_steps, int max_steps) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    for (int j = 0; j < 5; ++j) {
        C.x[5 * (size_t)b + j] = x_init[5 * (size_t)b + j];
        if (hist_x) hist_x[(size_t)b * (max_steps + 1) * 5 + j] = x_init[5 * (size_t)b + j];
    }
    C.active[b] = x_init[5 * (size_t)b] <= s_stop ? 1 : 0;
    C.obs_s[b] = F.obs_start_s;
    C.tl_timer[b] = 0.0;
    for (int j = 0; j < 4; ++j) C.fsm_flags[4 * (size_t)b + j] = 0;
    for (int j = 0; j < 4; ++j) C.obs[4 * (size_t)b + j] = 0.0;
    C.nobs[b] = 0;
    n_steps[b] = 0;
}

// TrajectoryLoader.get_global_pose(s, d) (trajectory_loader.py:104-116), batched
__global__ void mpc_pose_kernel(DevTable tab, int n, const double* __restrict__ s, const double* __restrict__ d,
                                double* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    global_pose(tab, s[i], d[i], out + 3 * (size_t)i);
}
