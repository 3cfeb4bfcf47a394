// mpcqp.hip — MI355X (gfx950) batched tracking-MPC solver + its C ABI (include/mpcqp.h).
//
// Hot path replaced: TrajectoryTracker.solve(x0, obstacles)
//   medinammartin3/Safe-Autonomous-Driving-MPC trajectory_tracking.py:213-263
// with TrajectoryLoader.get_state/get_control (trajectory_loader.py:86-102) on a device table.
//
// One 64-lane wavefront (= one workgroup) per MPC instance:
//   K1  warm start (trajectory_tracking.py:224-246), lane j = control step j
//   K1  nominal rollout == predict(x0, ubar) (:87-114), lookups lane-parallel, bit-exact
//   K2  Gauss-Newton QP(ubar) stage data, lane k = stage k
//   K4  Mehrotra primal-dual interior point: row/stage-parallel residuals, barrier weights,
//       step lengths on lanes; the Newton systems solved by a stage-wise (Riccati) recursion
//       executed wave-uniformly from LDS (FP64; the dense condensed Cholesky loses ~5 digits
//       on these problems)
//   K5  predict(x0, U*) (:261) and outputs
// Compiled with -ffp-contract=off: the interp / rollout / warm-start arithmetic is bit-exact to
// the reference's numpy arithmetic; the solver uses explicit fma() where it wants fusion.
//
// This file is the library's one translation unit.  The device code lives in the headers it includes:
//   device_common.h        table, parameters, lookups, LDS layout, cross-lane helpers, rollout, fences
//   riccati_lanes.h        the lane-distributed Riccati recursions (inline-asm DPP chains)
//   solve_kernel.h         mpc_solve_kernel and mpc_lookup_kernel
//   closed_loop_kernels.h  closed-loop FSM / plant / compaction kernels, pose kernel
//   sweep_kernels.h        the scenario sweep's FSM / plant kernels (a scenario per ego, check quantities)
//   traffic_kernels.h      the traffic scripts' FSM / gather kernels (up to 16 actors per ego)
//   convoy_kernels.h       the convoys' leader-ranking kernel (a workgroup per world)
//   noise_kernels.h        the disturbance sweeps' Philox source, measure / plant / draw kernels
//   evaluate_kernel.h      the batched evaluator of the reference's cost and constraint rows
// Below them: the host side (error plumbing, mpc_ctx, mpc_create, launch_solve, the batch, closed-loop, pose
// and lookup entry points) and, last, the comm layer (comm.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "../../include/mpcqp.h"
#include "host_table.h"
#include "cpu_backend.h"
#include "solve_kernel.h"
#include "closed_loop_kernels.h"
#include "sweep_kernels.h"
#include "traffic_kernels.h"
#include "convoy_kernels.h"
#include "noise_kernels.h"
#include "evaluate_kernel.h"

// ------------------------------------------------------------------------------------------
// host side: C ABI
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err = "";

static int fail(int code, const std::string& msg);

// a host-backend call behind an extern "C" entry: no C++ exception crosses the ABI (worker threads that
// cannot start, or allocations that fail, become MPC_E_ALLOC)
template <typename F>
static int host_call(F&& f) {
    try {
        f();
        return MPC_SUCCESS;
    } catch (const std::bad_alloc&) {
        return fail(MPC_E_ALLOC, "host backend: out of memory");
    } catch (const std::exception& e) {
        return fail(MPC_E_ALLOC, std::string("host backend: ") + e.what());
    } catch (...) {
        return fail(MPC_E_ALLOC, "host backend: unexpected exception");
    }
}

static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr, code)                                                                           \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return fail(code, std::string(#expr ": ") + hipGetErrorString(e_));    \
    } while (0)

struct mpc_ctx {
    int device;
    mpcqp_cpu::Backend* cpu;    // device = -1: the host backend (cpu_backend.h); no HIP state is created
    mpc_params p;
    DevTable tab;
    double* table_buf;
    // host-API staging buffers
    size_t cap_B;
    int cap_N, cap_obs;
    double *x0, *obs, *ub, *u0, *U, *X;
    int *nobs, *status, *iters;
    double *ls, *lst, *lct;
    size_t cap_lookup;
    // mpc_evaluate_batch's output staging (summary, terms, rows), grown on demand
    double* ev;
    size_t cap_ev;      // doubles
    hipStream_t stream;
    // work list of the two-phase launch: wl[0], wl[1] = counts of the eager calls (alternating), wl[2] = count
    // of a call captured into a graph, wl[3..cap_wl + 2] = deferred instance ids
#define MPC_WORKLIST_CAP (1 << 20)
#define MPC_WL_HEAD 3
    int* wl;
    int wl_epoch;       // counter wl[wl_epoch] serves the next eager call; wl[wl_epoch ^ 1] is zeroed by it
    bool wl_memset;     // MPC_WL_MEMSET=1: reset the count by a memset launch before every call (A/B switch)
    size_t cap_wl;
    bool two_phase;     // MPC_TWO_PHASE=0 in the environment selects the single MODE_FULL launch
    // the work list is reused by every call: a call on a different stream than the previous one
    // first waits for the previous call's last kernel (wl_done, recorded after each split launch)
    hipEvent_t wl_done;
    hipStream_t wl_stream;
    bool wl_pending;
    // stage cache of the split launch (same ordering as the work list): per deferred instance, the
    // linearisation point and nominal rollout that MODE_XO computed, read back by MODE_IPM.  Off by
    // default (MPC_STAGE_CACHE=1 enables it): the repeated setup is ~1% of the slowest instance, and the
    // A/B is within noise (C2 0.4288 vs 0.4288 ms, C3 0.4977 vs 0.5004, C4 0.6078 vs 0.6107, two runs
    // each) while the cache moves 2.9 MB more per C2 step.  Grown on demand by eager calls; a captured
    // call that finds it too small runs without it (same results)
    double* stc;
    size_t cap_stc;     // doubles
    bool use_stc;
    // MPC_IPM_GL64=1: the N = 20 interior-point launch of the split path with one deferred instance per
    // wavefront (GL = 64) instead of two (A/B switch)
    bool ipm_gl64;
};

extern "C" void mpc_default_params(mpc_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->N = 5;
    p->max_obs = 0;
    p->dt = 0.2;
    p->u_min[0] = -0.6; p->u_min[1] = -5.0;
    p->u_max[0] = 0.6;  p->u_max[1] = 4.0;
    p->vehicle_radius = 1.0;
    p->w_d = 10.0; p->w_o = 10.0; p->w_v = 5.0; p->w_u1 = 0.5; p->w_u2 = 0.5;
    p->obstacle_safety_distance = 5.0;
    p->max_time_2_obs = 1.5;
    p->wheelbase = 2.8;
    p->lane_width = 3.0;
    p->safe_lane_margin = 0.1;
    p->brake_distance = 40.0;
    p->brake_accel = -2.0;
    p->linearization = 1;
    p->sqp_iters = 1;
    p->max_iter = 80;
    p->tol = 1e-9;
    p->tol_mu = 1e-10;
    p->elastic_rho = 1e5;
    p->polish = 2;
    p->sqp_tol = 1e-10;
}

extern "C" const char* mpc_last_error(void) { return g_err.c_str(); }

#ifdef MPC_PROF
// diagnostic build only: accumulated shader cycles per kernel phase (lane 0 of every instance)
extern "C" int mpc_debug_prof(unsigned long long* out, int reset) {
    if (out) HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(unsigned long long) * 16), MPC_E_DEVICE);
    if (reset) {
        unsigned long long z[16] = {0};
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof(z)), MPC_E_DEVICE);
    }
    return MPC_SUCCESS;
}
#endif
extern "C" int mpc_version(void) { return MPCQP_VERSION; }

static int check_params(const mpc_params* p) {
    if (!p) return fail(MPC_E_ARG, "params is NULL");
    if (p->N < 1 || p->N > MPC_MAX_N) return fail(MPC_E_ARG, "N out of range [1, 63]");
    if (p->max_obs < 0 || p->max_obs > MPC_MAX_OBS) return fail(MPC_E_ARG, "max_obs out of range [0, 64]");
    if (!(p->dt > 0)) return fail(MPC_E_ARG, "dt must be > 0");
    if (p->max_iter < 1) return fail(MPC_E_ARG, "max_iter must be >= 1");
    if (p->sqp_iters < 0 || p->sqp_iters > 100) return fail(MPC_E_ARG, "sqp_iters out of range [0, 100]");
    if (!(p->elastic_rho > 1.0)) return fail(MPC_E_ARG, "elastic_rho must be > 1");
    if (!(p->sqp_tol >= 0.0)) return fail(MPC_E_ARG, "sqp_tol must be >= 0");
    return MPC_SUCCESS;
}

static KParams kparams(const mpc_params* p) {
    KParams k;
    k.N = p->N;
    k.max_obs = p->max_obs;
    k.linearization = p->linearization;
    k.sqp_iters = p->sqp_iters;
    k.max_iter = p->max_iter;
    k.dt = p->dt;
    k.u_min0 = p->u_min[0]; k.u_min1 = p->u_min[1];
    k.u_max0 = p->u_max[0]; k.u_max1 = p->u_max[1];
    k.w_d = p->w_d; k.w_o = p->w_o; k.w_v = p->w_v; k.w_u1 = p->w_u1; k.w_u2 = p->w_u2;
    k.osd = p->obstacle_safety_distance;
    k.tgap = p->max_time_2_obs;
    k.L = p->wheelbase;
    k.sl = p->lane_width / 2.0 - p->vehicle_radius - p->safe_lane_margin;   // trajectory_tracking.py:169
    k.brake_distance = p->brake_distance;
    k.brake_accel = p->brake_accel;
    k.tol = p->tol;
    k.tol_mu = p->tol_mu;
    k.rho = p->elastic_rho;
    k.polish = p->polish;
    k.sqp_tol = p->sqp_tol;
    const char* dbg = std::getenv("MPC_DBG");
    k.dbg = dbg ? std::atoi(dbg) : 0;
    k.mu_check = mpcqp_cpu::checkpoint_on() ? MU_CHECK : -1.0;
    return k;
}

extern "C" int mpc_create(const double* X, int T, const double* U, int Tu, const mpc_params* p, int device,
                          mpc_ctx** out) {
    if (!out) return fail(MPC_E_ARG, "out is NULL");
    *out = nullptr;
    if (!X || !U || T < 2 || Tu < 2) return fail(MPC_E_ARG, "trajectory table needs T >= 2, Tu >= 2");
    int rc = check_params(p);
    if (rc) return rc;
    if (device < -1) return fail(MPC_E_DEVICE, "device index out of range (-1 = CPU backend)");
    if (device == -1) {
        // host backend: the same table build, the solver on host threads (cpu_backend.h)
        mpcqp_host::HostTable ht;
        if (!mpcqp_host::build_host_table(X, T, U, Tu, ht)) return fail(MPC_E_ARG, "bad trajectory table");
        mpc_ctx* c = (mpc_ctx*)std::calloc(1, sizeof(mpc_ctx));
        if (!c) return fail(MPC_E_ALLOC, "calloc");
        c->device = -1;
        c->p = *p;
        c->cpu = new (std::nothrow) mpcqp_cpu::Backend(std::move(ht));
        if (!c->cpu) {
            std::free(c);
            return fail(MPC_E_ALLOC, "host backend");
        }
        *out = c;
        return MPC_SUCCESS;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(MPC_E_DEVICE, "no HIP device available (device = -1 selects the CPU backend)");
    if (device < 0 || device >= ndev) return fail(MPC_E_DEVICE, "device index out of range (-1 = CPU backend)");
    HIPCHK(hipSetDevice(device), MPC_E_DEVICE);
    mpcqp_host::HostTable ht;      // monotone s fix, interp columns, global line, bucket index (host_table.h)
    if (!mpcqp_host::build_host_table(X, T, U, Tu, ht)) return fail(MPC_E_ARG, "bad trajectory table");
    const std::vector<double>& h = ht.buf;
    const int tu = ht.tu;
    mpc_ctx* c = (mpc_ctx*)std::calloc(1, sizeof(mpc_ctx));
    if (!c) return fail(MPC_E_ALLOC, "calloc");
    c->device = device;
    c->p = *p;
    {
        const char* e = std::getenv("MPC_TWO_PHASE");
        c->two_phase = !(e && e[0] == '0');
        const char* e2 = std::getenv("MPC_STAGE_CACHE");
        c->use_stc = !(e2 && e2[0] == '0');     // on by default since round 6 (it carries the interior point's start)
        const char* e3 = std::getenv("MPC_WL_MEMSET");
        c->wl_memset = e3 && e3[0] == '1';
        const char* e4 = std::getenv("MPC_IPM_GL64");
        c->ipm_gl64 = e4 && e4[0] == '1';
    }
    if (hipMalloc(&c->table_buf, h.size() * sizeof(double)) != hipSuccess) {
        std::free(c);
        return fail(MPC_E_ALLOC, "hipMalloc table");
    }
    if (hipMemcpy(c->table_buf, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(c->table_buf);
        std::free(c);
        return fail(MPC_E_DEVICE, "hipMemcpy table");
    }
    c->tab.s = c->table_buf;
    c->tab.d = c->table_buf + T;
    c->tab.o = c->table_buf + 2 * T;
    c->tab.k = c->table_buf + 3 * T;
    c->tab.v = c->table_buf + 4 * T;
    c->tab.u1 = c->table_buf + 5 * T;
    c->tab.u2 = c->table_buf + 5 * T + tu;
    c->tab.gx = c->table_buf + 5 * T + 2 * tu;
    c->tab.gy = c->tab.gx + T;
    c->tab.gpsi = c->tab.gy + T;
    c->tab.T = T;
    c->tab.Tu = tu;
    c->tab.smax = ht.smax;
    c->tab.bidx = reinterpret_cast<const int*>(c->table_buf + ht.off_bidx);
    c->tab.nb = ht.nb;
    c->tab.s0 = ht.s0;
    c->tab.ibh = ht.ibh;
    for (int j = 0; j < 5; ++j) c->tab.last[j] = ht.last[j];
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        hipFree(c->table_buf);
        std::free(c);
        return fail(MPC_E_DEVICE, "hipStreamCreate");
    }
    // work list of the two-phase launch (count + ids), allocated here once so that no solve call
    // allocates; without it every batch runs the single-kernel path
    if (hipMalloc(&c->wl, sizeof(int) * ((size_t)MPC_WORKLIST_CAP + MPC_WL_HEAD)) == hipSuccess &&
        hipMemset(c->wl, 0, sizeof(int) * MPC_WL_HEAD) == hipSuccess &&
        hipEventCreateWithFlags(&c->wl_done, hipEventDisableTiming) == hipSuccess) {
        c->cap_wl = MPC_WORKLIST_CAP;
    } else {
        hipFree(c->wl);
        c->wl = nullptr;
        c->cap_wl = 0;
        (void)hipGetLastError();
    }
    *out = c;
    return MPC_SUCCESS;
}

extern "C" int mpc_set_params(mpc_ctx* c, const mpc_params* p) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    c->p = *p;
    return MPC_SUCCESS;
}

extern "C" int mpc_get_params(const mpc_ctx* c, mpc_params* p) {
    if (!c || !p) return fail(MPC_E_ARG, "NULL argument");
    *p = c->p;
    return MPC_SUCCESS;
}

static void free_staging(mpc_ctx* c) {
    hipFree(c->x0); hipFree(c->obs); hipFree(c->ub); hipFree(c->u0); hipFree(c->U); hipFree(c->X);
    hipFree(c->nobs); hipFree(c->status); hipFree(c->iters);
    c->x0 = c->obs = c->ub = c->u0 = c->U = c->X = nullptr;
    c->nobs = c->status = c->iters = nullptr;
    c->cap_B = 0;
}

extern "C" void mpc_destroy(mpc_ctx* c) {
    if (!c) return;
    if (c->cpu) {
        delete c->cpu;
        std::free(c);
        return;
    }
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    free_staging(c);
    hipFree(c->ls); hipFree(c->lst); hipFree(c->lct);
    hipFree(c->ev);
    if (c->wl) hipEventDestroy(c->wl_done);
    hipFree(c->wl);
    hipFree(c->stc);
    hipFree(c->table_buf);
    hipStreamDestroy(c->stream);
    std::free(c);
}

// launch of the solver kernel for an already validated parameter set
#define MPC_STAGE_CACHE_CAP ((size_t)1 << 27)
static int launch_solve(mpc_ctx* c, const KParams& kp, int B, const double* x0, const double* obs, const int* n_obs,
                        const double* ubar, double* u0, double* U, double* Xpred, int* status, int* iters,
                        hipStream_t st) {
    // G = 64 / GL instances per wavefront: the smallest lane group holding the N + 1 stages
    const int* nob = obs ? n_obs : nullptr;
    const int GL = kp.N + 1 <= 16 ? 16 : (kp.N + 1 <= 32 ? 32 : 64);
    const int G = WAVE / GL;
    // horizon of the specialised kernel that serves N (0: the runtime-horizon kernels)
    const int ntv = kp.N == 20 || kp.N == 30 || kp.N == 40 ? kp.N : 0;
    const size_t lds_wave = sizeof(double) * (size_t)lds_doubles(kp.N, acl_on(GL, ntv)) * G;
    if (lds_wave > 160 * 1024) return fail(MPC_E_ARG, "horizon too long for LDS");
    const size_t lds_lite = sizeof(double) * (size_t)lds_doubles(kp.N, false, true) * G;   // MODE_XO
    const dim3 grid((B + G - 1) / G);
    // Two-phase launch (MODE_XO then MODE_IPM) for single-QP solves with the crossover on; the work
    // list lives in the context (one list per context: a context is not re-entrant, include/mpcqp.h).
    // With one instance per wavefront (G = 1, N > 31) nothing is stranded behind a slower partner, and
    // the crossover rarely certifies at those horizons (C5: 9%), so the split only repeats the setup.
    // The list is allocated once by mpc_create (MPC_WORKLIST_CAP ids), so this path allocates nothing
    // and stays graph-capturable; a larger batch runs the single-kernel path (same results).
    const bool split = kp.polish >= 2 && kp.sqp_iters == 1 && c->two_phase && G >= 2 && (size_t)B <= c->cap_wl;
    int* wl = split ? c->wl + MPC_WL_HEAD : nullptr;
    int* wcnt = nullptr;
    int* wnext = nullptr;
    // Under stream capture (a HIP graph being recorded) the cross-call ordering below is left out: waiting
    // on wl_done, recorded outside the capture, would be a cross-capture dependency that invalidates the
    // capture, and an event recorded inside it belongs to the graph.  Replays of a captured graph are
    // therefore ordered against eager calls on the same context only by the caller (include/mpcqp.h).
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (split) HIPCHK(hipStreamIsCapturing(st, &cap), MPC_E_DEVICE);
    const bool capturing = cap != hipStreamCaptureStatusNone;
    double* stc = nullptr;
    if (split) {
        // the previous split launch may still be reading the list on another stream: order after it
        if (!capturing && c->wl_pending && c->wl_stream != st)
            HIPCHK(hipStreamWaitEvent(st, c->wl_done, 0), MPC_E_DEVICE);
        const size_t need = (size_t)B * stage_cache_doubles(kp.N);
        // the cache is sized for B records (only the deferred instances write one); above MPC_STAGE_CACHE_CAP
        // doubles (1 GiB) the call runs without it (the same results: the start is recomputed bit for bit)
        if (c->use_stc && need > c->cap_stc && need <= MPC_STAGE_CACHE_CAP && !capturing) {
            // hipFree waits for the device, so no launch still reads the old buffer
            hipFree(c->stc);
            c->stc = nullptr;
            c->cap_stc = 0;
            if (hipMalloc(&c->stc, need * sizeof(double)) == hipSuccess) c->cap_stc = need;
            else { c->stc = nullptr; (void)hipGetLastError(); }
        }
        // a captured call runs without the stage cache: a later eager call may grow (free and reallocate) it,
        // and a graph holding the old pointer would then replay into freed memory
        if (c->use_stc && need <= c->cap_stc && !capturing) stc = c->stc;
        if (capturing || c->wl_memset) {
            // a captured call resets its own count by a memset inside the graph, so every replay starts
            // from zero (an eager call's reset would not be replayed)
            wcnt = capturing ? c->wl + 2 : c->wl + c->wl_epoch;
            HIPCHK(hipMemsetAsync(wcnt, 0, sizeof(int), st), MPC_E_DEVICE);
        } else {
            // eager calls alternate between two counts: this call's MODE_XO zeroes the other one, which the
            // next call (same stream, or ordered after this one by wl_done) uses; no memset launch
            wcnt = c->wl + c->wl_epoch;
            wnext = c->wl + (c->wl_epoch ^ 1);
        }
    }
    // obstacle rows exist only when obstacles are passed
#define MPC_LAUNCH(GLV, OBSV, MODEV, NTV)                                                                   \
    hipLaunchKernelGGL((mpc_solve_kernel<GLV, OBSV, MODEV, NTV>), grid, dim3(WAVE),                    \
                       MODEV == MODE_XO ? lds_lite : lds_wave, st, c->tab, kp, B,                           \
                       x0, obs, nob, ubar, u0, U, Xpred, status, iters, wl, wcnt, stc,                 \
                       MODEV == MODE_XO ? wnext : nullptr)
    // horizon-specialised kernels for the BASELINE horizons (N = 20: C2, C3; N = 30: C4; N = 40: C5), whose
    // unrolled recursions pay for their code size (C4 0.89 -> 0.66 ms, C5 5.67 -> 4.16 ms)
#define MPC_LAUNCH_GL(MODEV)                                                                   \
    do {                                                                                       \
        if (ntv == 20) { if (with_obs) MPC_LAUNCH(32, true, MODEV, 20); else MPC_LAUNCH(32, false, MODEV, 20); } \
        else if (ntv == 30) { if (with_obs) MPC_LAUNCH(32, true, MODEV, 30); else MPC_LAUNCH(32, false, MODEV, 30); } \
        else if (ntv == 40) { if (with_obs) MPC_LAUNCH(64, true, MODEV, 40); else MPC_LAUNCH(64, false, MODEV, 40); } \
        else if (GL == 16) { if (with_obs) MPC_LAUNCH(16, true, MODEV, 0); else MPC_LAUNCH(16, false, MODEV, 0); } \
        else if (GL == 32) { if (with_obs) MPC_LAUNCH(32, true, MODEV, 0); else MPC_LAUNCH(32, false, MODEV, 0); } \
        else { if (with_obs) MPC_LAUNCH(64, true, MODEV, 0); else MPC_LAUNCH(64, false, MODEV, 0); } \
    } while (0)
    const bool with_obs = obs != nullptr && kp.max_obs > 0;
    if (split) {
        MPC_LAUNCH_GL(MODE_XO);
        HIPCHK(hipGetLastError(), MPC_E_LAUNCH);
        // the launched MODE_XO zeroed wl[epoch ^ 1] and uses wl[epoch]: the next eager call takes the other
        if (wnext) c->wl_epoch ^= 1;
        if (ntv == 20 && c->ipm_gl64) {
            // one deferred instance per wavefront: B waves at most, the wave's LDS for one group
            const size_t lds_one = sizeof(double) * (size_t)lds_doubles(kp.N, true);
            if (with_obs)
                hipLaunchKernelGGL((mpc_solve_kernel<64, true, MODE_IPM, 20>), dim3(B), dim3(WAVE), lds_one, st,
                                   c->tab, kp, B, x0, obs, nob, ubar, u0, U, Xpred, status, iters, wl, wcnt, stc,
                                   nullptr);
            else
                hipLaunchKernelGGL((mpc_solve_kernel<64, false, MODE_IPM, 20>), dim3(B), dim3(WAVE), lds_one, st,
                                   c->tab, kp, B, x0, obs, nob, ubar, u0, U, Xpred, status, iters, wl, wcnt, stc,
                                   nullptr);
        } else {
            MPC_LAUNCH_GL(MODE_IPM);
        }
        HIPCHK(hipGetLastError(), MPC_E_LAUNCH);
        if (!capturing) {
            HIPCHK(hipEventRecord(c->wl_done, st), MPC_E_DEVICE);
            c->wl_stream = st;
            c->wl_pending = true;
        }
    } else if (kp.sqp_iters == 1) {
        MPC_LAUNCH_GL(MODE_ONE);
    } else {
        MPC_LAUNCH_GL(MODE_FULL);
    }
#undef MPC_LAUNCH_GL
#undef MPC_LAUNCH
    HIPCHK(hipGetLastError(), MPC_E_LAUNCH);
    return MPC_SUCCESS;
}

extern "C" int mpc_solve_batch_device(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                                      const double* ubar, double* u0, double* U, double* Xpred, int* status,
                                      int* iters, void* stream) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0) return fail(MPC_E_ARG, "B < 0");
    if (B == 0) return MPC_SUCCESS;
    if (!x0) return fail(MPC_E_ARG, "x0 is NULL");
    if (c->p.max_obs > 0 && n_obs && !obs) return fail(MPC_E_ARG, "n_obs given but obs is NULL");
    if (obs && c->p.max_obs == 0)
        return fail(MPC_E_ARG, "obs given but params.max_obs == 0 (the obstacles would be ignored)");
    int rc = check_params(&c->p);
    if (rc) return rc;
    if (((uintptr_t)u0 | (uintptr_t)U | (uintptr_t)x0 | (uintptr_t)Xpred | (uintptr_t)obs | (uintptr_t)ubar) & 7)
        return fail(MPC_E_ARG, "double arrays must be 8-byte aligned");
    if (c->cpu) {
        // host context: the pointers are host memory and the call is synchronous (stream ignored)
        return host_call([&] { c->cpu->solve_batch(c->p, B, x0, obs, n_obs, ubar, u0, U, Xpred, status, iters); });
    }
    KParams kp = kparams(&c->p);
    if (!obs) kp.max_obs = 0;
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    return launch_solve(c, kp, B, x0, obs, n_obs, ubar, u0, U, Xpred, status, iters, (hipStream_t)stream);
}

template <typename T>
static int grow(T** ptr, size_t n) {
    hipFree(*ptr);
    *ptr = nullptr;
    if (n == 0) return 0;
    return hipMalloc(ptr, n * sizeof(T)) == hipSuccess ? 0 : -1;
}

// the host entries' staging buffers for a batch of B instances, horizon N and slab width mo (grow only)
static int ensure_staging(mpc_ctx* c, int B, int N, int mo) {
    if ((size_t)B > c->cap_B || N > c->cap_N || mo > c->cap_obs) {
        size_t nb = (size_t)B > c->cap_B ? (size_t)B : c->cap_B;
        int nn = N > c->cap_N ? N : c->cap_N;
        int no = mo > c->cap_obs ? mo : c->cap_obs;
        free_staging(c);
        if (grow(&c->x0, nb * 5) || grow(&c->obs, nb * (no > 0 ? no : 1) * 2) || grow(&c->ub, nb * 2 * nn) ||
            grow(&c->u0, nb * 2) || grow(&c->U, nb * 2 * nn) || grow(&c->X, nb * 5 * (nn + 1)) ||
            grow(&c->nobs, nb) || grow(&c->status, nb) || grow(&c->iters, nb))
            return fail(MPC_E_ALLOC, "hipMalloc staging");
        c->cap_B = nb;
        c->cap_N = nn;
        c->cap_obs = no;
    }
    return MPC_SUCCESS;
}

extern "C" int mpc_solve_batch(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                               const double* ubar, double* u0, double* U, double* Xpred, int* status, int* iters) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0) return fail(MPC_E_ARG, "B < 0");
    if (B == 0) return MPC_SUCCESS;
    if (!x0) return fail(MPC_E_ARG, "x0 is NULL");
    int rc = check_params(&c->p);
    if (rc) return rc;
    const int N = c->p.N, mo = c->p.max_obs;
    if (obs && mo == 0) return fail(MPC_E_ARG, "obs given but params.max_obs == 0 (the obstacles would be ignored)");
    if (c->cpu)
        return host_call([&] {
            c->cpu->solve_batch(c->p, B, x0, mo > 0 ? obs : nullptr, n_obs, ubar, u0, U, Xpred, status, iters);
        });
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    rc = ensure_staging(c, B, N, mo);
    if (rc) return rc;
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpyAsync(c->x0, x0, sizeof(double) * 5 * B, hipMemcpyHostToDevice, s), MPC_E_DEVICE);
    const bool use_obs = mo > 0 && obs;
    if (use_obs) {
        HIPCHK(hipMemcpyAsync(c->obs, obs, sizeof(double) * 2 * mo * B, hipMemcpyHostToDevice, s), MPC_E_DEVICE);
        if (n_obs) HIPCHK(hipMemcpyAsync(c->nobs, n_obs, sizeof(int) * B, hipMemcpyHostToDevice, s), MPC_E_DEVICE);
    }
    if (ubar) HIPCHK(hipMemcpyAsync(c->ub, ubar, sizeof(double) * 2 * N * B, hipMemcpyHostToDevice, s), MPC_E_DEVICE);
    rc = mpc_solve_batch_device(c, B, c->x0, use_obs ? c->obs : nullptr, use_obs && n_obs ? c->nobs : nullptr,
                                ubar ? c->ub : nullptr, c->u0, c->U, c->X, c->status, c->iters, (void*)s);
    if (rc) return rc;
    if (u0) HIPCHK(hipMemcpyAsync(u0, c->u0, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, s), MPC_E_DEVICE);
    if (U) HIPCHK(hipMemcpyAsync(U, c->U, sizeof(double) * 2 * N * B, hipMemcpyDeviceToHost, s), MPC_E_DEVICE);
    if (Xpred)
        HIPCHK(hipMemcpyAsync(Xpred, c->X, sizeof(double) * 5 * (N + 1) * B, hipMemcpyDeviceToHost, s), MPC_E_DEVICE);
    if (status) HIPCHK(hipMemcpyAsync(status, c->status, sizeof(int) * B, hipMemcpyDeviceToHost, s), MPC_E_DEVICE);
    if (iters) HIPCHK(hipMemcpyAsync(iters, c->iters, sizeof(int) * B, hipMemcpyDeviceToHost, s), MPC_E_DEVICE);
    HIPCHK(hipStreamSynchronize(s), MPC_E_DEVICE);
    return MPC_SUCCESS;
}

// ------------------------------------------------------------------------------------------
// batched evaluator (evaluate_kernel.h)
// ------------------------------------------------------------------------------------------
extern "C" int mpc_evaluate_batch_device(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                                         const double* U, double* Xpred, double* summary, double* terms,
                                         double* rows, void* stream) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0) return fail(MPC_E_ARG, "B < 0");
    if (B == 0) return MPC_SUCCESS;
    if (!x0) return fail(MPC_E_ARG, "x0 is NULL");
    if (!U) return fail(MPC_E_ARG, "U is NULL (the evaluator needs the control sequence to evaluate)");
    if (c->p.max_obs > 0 && n_obs && !obs) return fail(MPC_E_ARG, "n_obs given but obs is NULL");
    if (obs && c->p.max_obs == 0)
        return fail(MPC_E_ARG, "obs given but params.max_obs == 0 (the obstacles would be ignored)");
    int rc = check_params(&c->p);
    if (rc) return rc;
    if (((uintptr_t)x0 | (uintptr_t)obs | (uintptr_t)U | (uintptr_t)Xpred | (uintptr_t)summary | (uintptr_t)terms |
         (uintptr_t)rows) & 7)
        return fail(MPC_E_ARG, "double arrays must be 8-byte aligned");
    if (!Xpred && !summary && !terms && !rows) return MPC_SUCCESS;
    if (c->cpu)
        return host_call([&] { c->cpu->evaluate_batch(c->p, B, x0, obs, n_obs, U, Xpred, summary, terms, rows); });
    KParams kp = kparams(&c->p);
    const int rw = 7 + c->p.max_obs;       // the row width keeps the context's slab width without obstacles too
    if (!obs) kp.max_obs = 0;
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    const int GL = kp.N + 1 <= 16 ? 16 : (kp.N + 1 <= 32 ? 32 : 64);     // launch_solve's rule
    const dim3 grid((B + WAVE / GL - 1) / (WAVE / GL));
    hipStream_t st = (hipStream_t)stream;
#define MPC_EV_LAUNCH(GLV, OBSV)                                                                              \
    hipLaunchKernelGGL((mpc_evaluate_kernel<GLV, OBSV>), grid, dim3(WAVE), 0, st, c->tab, kp, B, rw, x0, obs, \
                       obs ? n_obs : nullptr, U, Xpred, summary, terms, rows)
    if (GL == 16) { if (obs) MPC_EV_LAUNCH(16, true); else MPC_EV_LAUNCH(16, false); }
    else if (GL == 32) { if (obs) MPC_EV_LAUNCH(32, true); else MPC_EV_LAUNCH(32, false); }
    else { if (obs) MPC_EV_LAUNCH(64, true); else MPC_EV_LAUNCH(64, false); }
#undef MPC_EV_LAUNCH
    HIPCHK(hipGetLastError(), MPC_E_LAUNCH);
    return MPC_SUCCESS;
}

extern "C" int mpc_evaluate_batch(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                                  const double* U, double* Xpred, double* summary, double* terms, double* rows) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0) return fail(MPC_E_ARG, "B < 0");
    if (B == 0) return MPC_SUCCESS;
    if (!x0) return fail(MPC_E_ARG, "x0 is NULL");
    if (!U) return fail(MPC_E_ARG, "U is NULL (the evaluator needs the control sequence to evaluate)");
    int rc = check_params(&c->p);
    if (rc) return rc;
    const int N = c->p.N, mo = c->p.max_obs, rw = 7 + mo;
    if (obs && mo == 0) return fail(MPC_E_ARG, "obs given but params.max_obs == 0 (the obstacles would be ignored)");
    if (!Xpred && !summary && !terms && !rows) return MPC_SUCCESS;
    if (c->cpu)
        return host_call([&] {
            c->cpu->evaluate_batch(c->p, B, x0, mo > 0 ? obs : nullptr, n_obs, U, Xpred, summary, terms, rows);
        });
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    rc = ensure_staging(c, B, N, mo);
    if (rc) return rc;
    const size_t n_sum = (size_t)B * MPC_EV_NQ, n_terms = (size_t)B * 5, n_rows = (size_t)B * N * rw;
    if (n_sum + n_terms + n_rows > c->cap_ev) {
        c->cap_ev = 0;
        if (grow(&c->ev, n_sum + n_terms + n_rows)) return fail(MPC_E_ALLOC, "hipMalloc evaluator staging");
        c->cap_ev = n_sum + n_terms + n_rows;
    }
    double *d_sum = c->ev, *d_terms = c->ev + n_sum, *d_rows = c->ev + n_sum + n_terms;
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpyAsync(c->x0, x0, sizeof(double) * 5 * B, hipMemcpyHostToDevice, s), MPC_E_DEVICE);
    const bool use_obs = obs != nullptr;
    if (use_obs) {
        HIPCHK(hipMemcpyAsync(c->obs, obs, sizeof(double) * 2 * mo * B, hipMemcpyHostToDevice, s), MPC_E_DEVICE);
        if (n_obs) HIPCHK(hipMemcpyAsync(c->nobs, n_obs, sizeof(int) * B, hipMemcpyHostToDevice, s), MPC_E_DEVICE);
    }
    HIPCHK(hipMemcpyAsync(c->ub, U, sizeof(double) * 2 * N * B, hipMemcpyHostToDevice, s), MPC_E_DEVICE);
    rc = mpc_evaluate_batch_device(c, B, c->x0, use_obs ? c->obs : nullptr, use_obs && n_obs ? c->nobs : nullptr,
                                   c->ub, Xpred ? c->X : nullptr, summary ? d_sum : nullptr,
                                   terms ? d_terms : nullptr, rows ? d_rows : nullptr, (void*)s);
    if (rc) return rc;
    if (Xpred)
        HIPCHK(hipMemcpyAsync(Xpred, c->X, sizeof(double) * 5 * (N + 1) * B, hipMemcpyDeviceToHost, s), MPC_E_DEVICE);
    if (summary) HIPCHK(hipMemcpyAsync(summary, d_sum, sizeof(double) * n_sum, hipMemcpyDeviceToHost, s), MPC_E_DEVICE);
    if (terms) HIPCHK(hipMemcpyAsync(terms, d_terms, sizeof(double) * n_terms, hipMemcpyDeviceToHost, s), MPC_E_DEVICE);
    if (rows) HIPCHK(hipMemcpyAsync(rows, d_rows, sizeof(double) * n_rows, hipMemcpyDeviceToHost, s), MPC_E_DEVICE);
    HIPCHK(hipStreamSynchronize(s), MPC_E_DEVICE);
    return MPC_SUCCESS;
}

extern "C" void mpc_default_fsm(mpc_fsm* f) {
    std::memset(f, 0, sizeof(*f));
    // the trajectory2.json preset, active in the reference (trajectory_tracking.py:292-308)
    f->obs_trigger_s = 710.0;
    f->obs_start_s = 780.0;
    f->obs_v = 4.0;
    f->obs_end_s = 1050.0;
    f->tl_pos = 550.0;
    f->tl_trigger_s = 100.0;
    f->tl_stop_duration = 20.0;
}

extern "C" int mpc_closed_loop(mpc_ctx* c, int B, const double* x_init, const mpc_fsm* fsm, int max_steps,
                               double s_stop, double* hist_x, double* hist_u, double* hist_obs_s, int* hist_tl,
                               int* hist_status, int* n_steps, double* step_ms) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0 || max_steps < 1) return fail(MPC_E_ARG, "B < 0 or max_steps < 1");
    if (B == 0) return MPC_SUCCESS;
    if (!x_init || !n_steps) return fail(MPC_E_ARG, "x_init and n_steps are required");
    int rc = check_params(&c->p);
    if (rc) return rc;
    mpc_fsm F;
    if (fsm) F = *fsm; else mpc_default_fsm(&F);     // NULL: both scenarios off
    const bool with_fsm = fsm && (F.dynamic_obstacle || F.traffic_light);
    if (c->cpu) {
        int hrc = MPC_SUCCESS;
        const int erc = host_call([&] {
            hrc = c->cpu->closed_loop(c->p, B, x_init, F, with_fsm, max_steps, s_stop, hist_x, hist_u, hist_obs_s,
                                      hist_tl, hist_status, n_steps, step_ms);
        });
        return erc != MPC_SUCCESS ? erc : hrc;
    }
    KParams kp = kparams(&c->p);
    kp.max_obs = with_fsm ? 2 : 0;          // the FSM yields at most the car and the light
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    const size_t nb = (size_t)B, ns = (size_t)max_steps;
    std::vector<void*> bufs;
    auto dalloc = [&](size_t bytes) -> void* {
        void* ptr = nullptr;
        if (hipMalloc(&ptr, bytes) != hipSuccess) return nullptr;
        bufs.push_back(ptr);
        return ptr;
    };
    auto release = [&]() { for (void* q : bufs) hipFree(q); };
    ClState C;
    C.x = (double*)dalloc(nb * 5 * 8);
    C.obs = (double*)dalloc(nb * 4 * 8);
    C.nobs = (int*)dalloc(nb * 4);
    C.active = (int*)dalloc(nb * 4);
    C.obs_s = (double*)dalloc(nb * 8);
    C.tl_timer = (double*)dalloc(nb * 8);
    C.fsm_flags = (int*)dalloc(nb * 4 * 4);
    C.n_active = (int*)dalloc(4);
    C.alist = (int*)dalloc(nb * 4);
    C.n_list = (int*)dalloc(4);
    C.xa = (double*)dalloc(nb * 5 * 8);
    C.obsa = (double*)dalloc(nb * 4 * 8);
    C.nobsa = (int*)dalloc(nb * 4);
    C.u0a = (double*)dalloc(nb * 2 * 8);
    C.sta = (int*)dalloc(nb * 4);
    double* d_xinit = (double*)dalloc(nb * 5 * 8);
    double* d_hx = hist_x ? (double*)dalloc(nb * (ns + 1) * 5 * 8) : nullptr;
    double* d_hu = hist_u ? (double*)dalloc(nb * ns * 2 * 8) : nullptr;
    double* d_ho = hist_obs_s ? (double*)dalloc(nb * ns * 8) : nullptr;
    int* d_ht = hist_tl ? (int*)dalloc(nb * ns * 4) : nullptr;
    int* d_hs = hist_status ? (int*)dalloc(nb * ns * 4) : nullptr;
    int* d_ns = (int*)dalloc(nb * 4);
    for (void* q : bufs)
        if (!q) { release(); return fail(MPC_E_ALLOC, "hipMalloc closed-loop buffers"); }
    if ((hist_x && !d_hx) || (hist_u && !d_hu) || (hist_obs_s && !d_ho) || (hist_tl && !d_ht) || (hist_status && !d_hs)) {
        release();
        return fail(MPC_E_ALLOC, "hipMalloc closed-loop histories");
    }
    hipStream_t st = c->stream;
    std::vector<hipEvent_t> ev;
    auto cleanup = [&]() {
        hipStreamSynchronize(st);
        for (auto& e : ev)
            if (e) hipEventDestroy(e);
        release();
    };
    // steps that never run stay NaN / -1 (all-ones bytes)
    bool ok0 = true;
    if (d_hx) ok0 = ok0 && hipMemsetAsync(d_hx, 0xff, nb * (ns + 1) * 5 * 8, st) == hipSuccess;
    if (d_hu) ok0 = ok0 && hipMemsetAsync(d_hu, 0xff, nb * ns * 2 * 8, st) == hipSuccess;
    if (d_ho) ok0 = ok0 && hipMemsetAsync(d_ho, 0xff, nb * ns * 8, st) == hipSuccess;
    if (d_ht) ok0 = ok0 && hipMemsetAsync(d_ht, 0xff, nb * ns * 4, st) == hipSuccess;
    if (d_hs) ok0 = ok0 && hipMemsetAsync(d_hs, 0xff, nb * ns * 4, st) == hipSuccess;
    ok0 = ok0 && hipMemcpyAsync(d_xinit, x_init, nb * 5 * 8, hipMemcpyHostToDevice, st) == hipSuccess;
    if (!ok0) {
        cleanup();
        return fail(MPC_E_DEVICE, "closed-loop buffer initialisation");
    }
    const dim3 tb(256), tg((B + 255) / 256);
    hipLaunchKernelGGL(cl_init_kernel, tg, tb, 0, st, B, F, C, d_xinit, s_stop, d_hx, d_ns, max_steps);
    if (step_ms) {
        ev.assign(ns + 1, nullptr);
        for (auto& e : ev)
            if (hipEventCreate(&e) != hipSuccess) {
                e = nullptr;
                cleanup();
                return fail(MPC_E_DEVICE, "hipEventCreate (step timing)");
            }
        if (hipEventRecord(ev[0], st) != hipSuccess) {
            cleanup();
            return fail(MPC_E_DEVICE, "hipEventRecord (step timing)");
        }
    }
    int steps_run = 0;
    rc = MPC_SUCCESS;
    // the solve runs on the egos still in the loop: the list is rebuilt at the host syncs below whenever
    // egos have left, so retired egos stop costing solver work (results are per ego, unchanged)
    hipLaunchKernelGGL(cl_compact_kernel, dim3(1), dim3(1024), 0, st, B, C);
    int nl = 0;
    if (hipMemcpyAsync(&nl, C.n_list, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        cleanup();
        return fail(MPC_E_DEVICE, "closed-loop initial ego list");
    }
    for (int step = 0; step < max_steps && nl > 0; ++step) {
        // runs without scenarios too: records the RED light / no-car histories like the reference
        hipLaunchKernelGGL(cl_fsm_kernel, tg, tb, 0, st, B, F, kp.dt, C, d_ho, d_ht, step, max_steps);
        const dim3 lg((nl + 255) / 256);
        hipLaunchKernelGGL(cl_gather_kernel, lg, tb, 0, st, nl, C);
        rc = launch_solve(c, kp, nl, C.xa, with_fsm ? C.obsa : nullptr, with_fsm ? C.nobsa : nullptr, nullptr, C.u0a,
                          nullptr, nullptr, C.sta, nullptr, st);
        if (rc) break;
        if (hipMemsetAsync(C.n_active, 0, 4, st) != hipSuccess) {
            rc = fail(MPC_E_DEVICE, "closed-loop active-count reset");
            break;
        }
        hipLaunchKernelGGL(cl_plant_kernel, lg, tb, 0, st, c->tab, nl, kp.dt, C, s_stop, d_hx, d_hu, d_hs, d_ns, step,
                           max_steps);
        if (step_ms && hipEventRecord(ev[step + 1], st) != hipSuccess) {
            rc = fail(MPC_E_DEVICE, "hipEventRecord (step timing)");
            break;
        }
        steps_run = step + 1;
        if ((step & 7) == 7 || step == max_steps - 1) {     // every 8 steps: has every ego left the loop?
            int na = 0;
            if (hipMemcpyAsync(&na, C.n_active, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) {
                rc = fail(MPC_E_DEVICE, "closed-loop step sync");
                break;
            }
            if (na == 0) break;
            if (na < nl) {                                  // egos left: shrink the solver's list
                hipLaunchKernelGGL(cl_compact_kernel, dim3(1), dim3(1024), 0, st, B, C);
                if (hipMemcpyAsync(&nl, C.n_list, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                    hipStreamSynchronize(st) != hipSuccess) {
                    rc = fail(MPC_E_DEVICE, "closed-loop ego list");
                    break;
                }
            }
        }
    }
    if (rc == MPC_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(MPC_E_LAUNCH, "closed-loop kernel launch");
    if (rc == MPC_SUCCESS) {
        bool ok = hipMemcpyAsync(n_steps, d_ns, nb * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (hist_x) ok = ok && hipMemcpyAsync(hist_x, d_hx, nb * (ns + 1) * 5 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (hist_u) ok = ok && hipMemcpyAsync(hist_u, d_hu, nb * ns * 2 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (hist_obs_s) ok = ok && hipMemcpyAsync(hist_obs_s, d_ho, nb * ns * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (hist_tl) ok = ok && hipMemcpyAsync(hist_tl, d_ht, nb * ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (hist_status) ok = ok && hipMemcpyAsync(hist_status, d_hs, nb * ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = ok && hipStreamSynchronize(st) == hipSuccess;
        if (!ok) rc = fail(MPC_E_DEVICE, "closed-loop copy-back");
    }
    if (step_ms) {
        for (size_t i = 0; i < ns; ++i) {
            float ms = NAN;
            if ((int)i < steps_run && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) != hipSuccess) ms = NAN;
            step_ms[i] = ms;
        }
    }
    cleanup();
    return rc;
}

// mpc_closed_loop with a scenario per ego, the check quantities accumulated on the device and histories for
// the named egos only (include/mpcqp.h).  Device allocations: the closed loop's per-ego state (ClState), the
// scenarios [B] when they differ, the quantities [MPC_CL_NQ][B], two int arrays [B] (flags, history slots),
// n_steps [B] and the kept histories [n_hist][max_steps ..]: O(B) + O(n_hist * max_steps).  Step times come
// from a ring of SW_EVENTS events read at the every-8-steps host sync
#define SW_EVENTS 9
extern "C" int mpc_closed_loop_sweep(mpc_ctx* c, int B, const double* x_init, const mpc_fsm* fsm, int n_fsm,
                                     int max_steps, double s_stop, double* quant, int n_hist, const int* hist_egos,
                                     double* hist_x, double* hist_u, double* hist_obs_s, int* hist_tl,
                                     int* hist_status, int* n_steps, double* step_ms) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0 || max_steps < 1) return fail(MPC_E_ARG, "B < 0 or max_steps < 1");
    if (fsm ? !(n_fsm == 1 || n_fsm == B) : n_fsm != 0)
        return fail(MPC_E_ARG, "n_fsm must be B (a scenario per ego), 1 (shared) or 0 with fsm NULL");
    if (!quant) return fail(MPC_E_ARG, "quant is required");
    if (n_hist < 0) return fail(MPC_E_ARG, "n_hist < 0");
    if (n_hist == 0 && (hist_x || hist_u || hist_obs_s || hist_tl || hist_status))
        return fail(MPC_E_ARG, "a history array is given but n_hist == 0");
    if (n_hist > 0 && !hist_egos) return fail(MPC_E_ARG, "hist_egos is NULL but n_hist > 0");
    std::vector<int> slot;
    try {
        slot.assign((size_t)B, -1);
    } catch (const std::bad_alloc&) {
        return fail(MPC_E_ALLOC, "history slot map");
    }
    for (int k = 0; k < n_hist; ++k) {
        const int e = hist_egos[k];
        if (e < 0 || e >= B) return fail(MPC_E_ARG, "hist_egos: ego index out of range [0, B)");
        if (slot[e] >= 0) return fail(MPC_E_ARG, "hist_egos: ego index repeated");
        slot[e] = k;
    }
    if (B == 0) return MPC_SUCCESS;
    if (!x_init) return fail(MPC_E_ARG, "x_init is required");
    int rc = check_params(&c->p);
    if (rc) return rc;
    mpc_fsm F;
    mpc_default_fsm(&F);                             // no scenario: both switches off
    if (fsm && n_fsm == 1) F = fsm[0];
    const bool per_ego = fsm && n_fsm != 1;          // n_fsm == B > 1
    bool with_fsm = F.dynamic_obstacle || F.traffic_light;
    if (per_ego)
        for (int b = 0; b < B && !with_fsm; ++b) with_fsm = fsm[b].dynamic_obstacle || fsm[b].traffic_light;
    if (c->cpu) {
        int hrc = MPC_SUCCESS;
        const int erc = host_call([&] {
            hrc = c->cpu->closed_loop_sweep(c->p, B, x_init, per_ego ? fsm : &F, per_ego ? B : 1, with_fsm, max_steps,
                                            s_stop, quant, n_hist, slot.data(), hist_x, hist_u, hist_obs_s, hist_tl,
                                            hist_status, n_steps, step_ms);
        });
        return erc != MPC_SUCCESS ? erc : hrc;
    }
    KParams kp = kparams(&c->p);
    kp.max_obs = with_fsm ? 2 : 0;          // the FSM yields at most the car and the light
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    const size_t nb = (size_t)B, ns = (size_t)max_steps, nh = (size_t)n_hist;
    std::vector<void*> bufs;
    auto dalloc = [&](size_t bytes) -> void* {
        void* ptr = nullptr;
        if (hipMalloc(&ptr, bytes) != hipSuccess) return nullptr;
        bufs.push_back(ptr);
        return ptr;
    };
    auto release = [&]() { for (void* q : bufs) hipFree(q); };
    ClState C;
    C.x = (double*)dalloc(nb * 5 * 8);
    C.obs = (double*)dalloc(nb * 4 * 8);
    C.nobs = (int*)dalloc(nb * 4);
    C.active = (int*)dalloc(nb * 4);
    C.obs_s = (double*)dalloc(nb * 8);
    C.tl_timer = (double*)dalloc(nb * 8);
    C.fsm_flags = (int*)dalloc(nb * 4 * 4);
    C.n_active = (int*)dalloc(4);
    C.alist = (int*)dalloc(nb * 4);
    C.n_list = (int*)dalloc(4);
    C.xa = (double*)dalloc(nb * 5 * 8);
    C.obsa = (double*)dalloc(nb * 4 * 8);
    C.nobsa = (int*)dalloc(nb * 4);
    C.u0a = (double*)dalloc(nb * 2 * 8);
    C.sta = (int*)dalloc(nb * 4);
    double* d_xinit = (double*)dalloc(nb * 5 * 8);
    SwState S;
    S.q = (double*)dalloc(nb * MPC_CL_NQ * 8);
    S.qflags = (int*)dalloc(nb * 4);
    int* d_hslot = (int*)dalloc(nb * 4);
    S.hslot = d_hslot;
    S.n_steps = (int*)dalloc(nb * 4);
    mpc_fsm* d_fsm = per_ego ? (mpc_fsm*)dalloc(nb * sizeof(mpc_fsm)) : nullptr;
    S.hist_x = hist_x ? (double*)dalloc(nh * (ns + 1) * 5 * 8) : nullptr;
    S.hist_u = hist_u ? (double*)dalloc(nh * ns * 2 * 8) : nullptr;
    S.hist_obs_s = hist_obs_s ? (double*)dalloc(nh * ns * 8) : nullptr;
    S.hist_tl = hist_tl ? (int*)dalloc(nh * ns * 4) : nullptr;
    S.hist_status = hist_status ? (int*)dalloc(nh * ns * 4) : nullptr;
    for (void* q : bufs)
        if (!q) { release(); return fail(MPC_E_ALLOC, "hipMalloc sweep buffers"); }
    if ((per_ego && !d_fsm) || (hist_x && !S.hist_x) || (hist_u && !S.hist_u) || (hist_obs_s && !S.hist_obs_s) ||
        (hist_tl && !S.hist_tl) || (hist_status && !S.hist_status)) {
        release();
        return fail(MPC_E_ALLOC, "hipMalloc sweep scenarios / histories");
    }
    hipStream_t st = c->stream;
    hipEvent_t ev[SW_EVENTS] = {};
    auto cleanup = [&]() {
        hipStreamSynchronize(st);
        for (auto& e : ev)
            if (e) hipEventDestroy(e);
        release();
    };
    // steps that never run stay NaN / -1 (all-ones bytes)
    bool ok0 = true;
    if (S.hist_x) ok0 = ok0 && hipMemsetAsync(S.hist_x, 0xff, nh * (ns + 1) * 5 * 8, st) == hipSuccess;
    if (S.hist_u) ok0 = ok0 && hipMemsetAsync(S.hist_u, 0xff, nh * ns * 2 * 8, st) == hipSuccess;
    if (S.hist_obs_s) ok0 = ok0 && hipMemsetAsync(S.hist_obs_s, 0xff, nh * ns * 8, st) == hipSuccess;
    if (S.hist_tl) ok0 = ok0 && hipMemsetAsync(S.hist_tl, 0xff, nh * ns * 4, st) == hipSuccess;
    if (S.hist_status) ok0 = ok0 && hipMemsetAsync(S.hist_status, 0xff, nh * ns * 4, st) == hipSuccess;
    ok0 = ok0 && hipMemcpyAsync(d_xinit, x_init, nb * 5 * 8, hipMemcpyHostToDevice, st) == hipSuccess;
    ok0 = ok0 && hipMemcpyAsync(d_hslot, slot.data(), nb * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    if (per_ego) ok0 = ok0 && hipMemcpyAsync(d_fsm, fsm, nb * sizeof(mpc_fsm), hipMemcpyHostToDevice, st) == hipSuccess;
    if (!ok0) {
        cleanup();
        return fail(MPC_E_DEVICE, "sweep buffer initialisation");
    }
    const dim3 tb(256), tg((B + 255) / 256);
    if (per_ego) hipLaunchKernelGGL(sw_init_kernel<true>, tg, tb, 0, st, B, F, d_fsm, C, S, d_xinit, s_stop, max_steps);
    else hipLaunchKernelGGL(sw_init_kernel<false>, tg, tb, 0, st, B, F, d_fsm, C, S, d_xinit, s_stop, max_steps);
    for (auto& e : ev)
        if (hipEventCreate(&e) != hipSuccess) {
            e = nullptr;
            cleanup();
            return fail(MPC_E_DEVICE, "hipEventCreate (step timing)");
        }
    if (hipEventRecord(ev[0], st) != hipSuccess) {
        cleanup();
        return fail(MPC_E_DEVICE, "hipEventRecord (step timing)");
    }
    // step i ran between events i and i + 1 of the ring; read at a host sync, at most 8 steps after the last
    // read, so no event is re-recorded before its interval has been taken
    std::vector<double> ms;
    auto read_times = [&](int upto) {
        for (int i = (int)ms.size(); i < upto; ++i) {
            float t = NAN;
            if (hipEventElapsedTime(&t, ev[i % SW_EVENTS], ev[(i + 1) % SW_EVENTS]) != hipSuccess) t = NAN;
            ms.push_back(t);
        }
    };
    rc = MPC_SUCCESS;
    hipLaunchKernelGGL(cl_compact_kernel, dim3(1), dim3(1024), 0, st, B, C);
    int nl = 0;
    if (hipMemcpyAsync(&nl, C.n_list, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        cleanup();
        return fail(MPC_E_DEVICE, "sweep initial ego list");
    }
    try {
        for (int step = 0; step < max_steps && nl > 0; ++step) {
            if (per_ego) hipLaunchKernelGGL(sw_fsm_kernel<true>, tg, tb, 0, st, B, F, d_fsm, kp.dt, C, S, step, max_steps);
            else hipLaunchKernelGGL(sw_fsm_kernel<false>, tg, tb, 0, st, B, F, d_fsm, kp.dt, C, S, step, max_steps);
            const dim3 lg((nl + 255) / 256);
            hipLaunchKernelGGL(cl_gather_kernel, lg, tb, 0, st, nl, C);
            rc = launch_solve(c, kp, nl, C.xa, with_fsm ? C.obsa : nullptr, with_fsm ? C.nobsa : nullptr, nullptr,
                              C.u0a, nullptr, nullptr, C.sta, nullptr, st);
            if (rc) break;
            if (hipMemsetAsync(C.n_active, 0, 4, st) != hipSuccess) {
                rc = fail(MPC_E_DEVICE, "sweep active-count reset");
                break;
            }
            hipLaunchKernelGGL(sw_plant_kernel, lg, tb, 0, st, c->tab, B, nl, kp.dt, C, S, s_stop, step, max_steps);
            if (hipEventRecord(ev[(step + 1) % SW_EVENTS], st) != hipSuccess) {
                rc = fail(MPC_E_DEVICE, "hipEventRecord (step timing)");
                break;
            }
            if ((step & 7) == 7 || step == max_steps - 1) {     // every 8 steps: has every ego left the loop?
                int na = 0;
                if (hipMemcpyAsync(&na, C.n_active, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                    hipStreamSynchronize(st) != hipSuccess) {
                    rc = fail(MPC_E_DEVICE, "sweep step sync");
                    break;
                }
                read_times(step + 1);
                if (na == 0) break;
                if (na < nl) {                                  // egos left: shrink the solver's list
                    hipLaunchKernelGGL(cl_compact_kernel, dim3(1), dim3(1024), 0, st, B, C);
                    if (hipMemcpyAsync(&nl, C.n_list, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                        hipStreamSynchronize(st) != hipSuccess) {
                        rc = fail(MPC_E_DEVICE, "sweep ego list");
                        break;
                    }
                }
            }
        }
        if (rc == MPC_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(MPC_E_LAUNCH, "sweep kernel launch");
        if (rc == MPC_SUCCESS) {
            std::vector<double> hq(nb * MPC_CL_NQ);
            std::vector<int> hn(nb);
            bool ok = hipMemcpyAsync(hn.data(), S.n_steps, nb * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(hq.data(), S.q, nb * MPC_CL_NQ * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_x) ok = ok && hipMemcpyAsync(hist_x, S.hist_x, nh * (ns + 1) * 5 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_u) ok = ok && hipMemcpyAsync(hist_u, S.hist_u, nh * ns * 2 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_obs_s) ok = ok && hipMemcpyAsync(hist_obs_s, S.hist_obs_s, nh * ns * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_tl) ok = ok && hipMemcpyAsync(hist_tl, S.hist_tl, nh * ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_status) ok = ok && hipMemcpyAsync(hist_status, S.hist_status, nh * ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && hipStreamSynchronize(st) == hipSuccess;
            if (!ok) {
                rc = fail(MPC_E_DEVICE, "sweep copy-back");
            } else {
                for (size_t b = 0; b < nb; ++b)               // [MPC_CL_NQ][B] on the device -> [B][MPC_CL_NQ]
                    for (int k = 0; k < MPC_CL_NQ; ++k) quant[b * MPC_CL_NQ + k] = hq[(size_t)k * nb + b];
                mpcqp_cpu::sweep_max_step_ms(B, hn.data(), ms, quant);
                if (n_steps) std::memcpy(n_steps, hn.data(), nb * 4);
                if (step_ms)
                    for (size_t i = 0; i < ns; ++i) step_ms[i] = i < ms.size() ? ms[i] : (double)NAN;
            }
        }
    } catch (const std::bad_alloc&) {
        rc = fail(MPC_E_ALLOC, "sweep host buffers");
    }
    cleanup();
    return rc;
}

extern "C" int mpc_cl_verdicts(const mpc_ctx* c, int B, const double* quant, double s_total, int* verdicts,
                               int counts[8]) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0 || (B > 0 && !quant)) return fail(MPC_E_ARG, "B < 0 or quant is NULL");
    mpcqp_cpu::cl_verdicts(c->p, B, quant, s_total, verdicts, counts);
    return MPC_SUCCESS;
}

extern "C" void mpc_actors_from_fsm(const mpc_fsm* f, mpc_actor out[2]) {
    std::memset(out, 0, 2 * sizeof(mpc_actor));
    if (f->dynamic_obstacle) {
        out[0].kind = MPC_ACTOR_CAR;
        out[0].trigger_s = f->obs_trigger_s;
        out[0].pos_s = f->obs_start_s;
        out[0].v = f->obs_v;
        out[0].end_s = f->obs_end_s;
    }
    if (f->traffic_light) {
        out[1].kind = MPC_ACTOR_LIGHT;
        out[1].trigger_s = f->tl_trigger_s;
        out[1].pos_s = f->tl_pos;
        out[1].stop_duration = f->tl_stop_duration;
    }
}

// mpc_closed_loop_sweep with a script of A actors per ego (include/mpcqp.h): the same loop, plant kernel,
// compaction and event ring around tr_fsm_kernel / tr_gather_kernel and an A-wide slab.  Device allocations: the
// per-ego state and packed solver buffers [B], the per-actor state and the slab [A][B], the scripts [B][A] (or
// [A] when shared), the quantities and extras, and the kept histories [n_hist][max_steps ..(A)]:
// O(B * A) + O(n_hist * max_steps * A)
extern "C" int mpc_closed_loop_traffic(mpc_ctx* c, int B, const double* x_init, const mpc_actor* actors, int A,
                                       int n_scripts, int max_steps, double s_stop, double* quant, double* extra,
                                       int n_hist, const int* hist_egos, double* hist_x, double* hist_u,
                                       double* hist_car_s, int* hist_tl, int* hist_status, int* hist_nobs,
                                       double* hist_slab, int* n_steps, double* step_ms) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0 || max_steps < 1) return fail(MPC_E_ARG, "B < 0 or max_steps < 1");
    if (A < 0 || A > MPC_MAX_ACTORS) return fail(MPC_E_ARG, "A out of range [0, 16]");
    if (actors ? !(n_scripts == 1 || n_scripts == B) : n_scripts != 0)
        return fail(MPC_E_ARG, "n_scripts must be B (a script per ego), 1 (shared) or 0 with actors NULL");
    if (!actors && A != 0) return fail(MPC_E_ARG, "actors is NULL but A > 0");
    if (!quant) return fail(MPC_E_ARG, "quant is required");
    if (n_hist < 0) return fail(MPC_E_ARG, "n_hist < 0");
    if (n_hist == 0 && (hist_x || hist_u || hist_car_s || hist_tl || hist_status || hist_nobs || hist_slab))
        return fail(MPC_E_ARG, "a history array is given but n_hist == 0");
    if (hist_slab && A == 0) return fail(MPC_E_ARG, "hist_slab is given but A == 0");
    if (n_hist > 0 && !hist_egos) return fail(MPC_E_ARG, "hist_egos is NULL but n_hist > 0");
    bool with_slab = false;
    for (size_t k = 0; k < (size_t)n_scripts * (size_t)A; ++k) {
        if (actors[k].kind < MPC_ACTOR_NONE || actors[k].kind > MPC_ACTOR_LIGHT)
            return fail(MPC_E_ARG, "actor kind outside MPC_ACTOR_NONE .. MPC_ACTOR_LIGHT");
        with_slab = with_slab || actors[k].kind != MPC_ACTOR_NONE;
    }
    std::vector<int> slot;
    try {
        slot.assign((size_t)B, -1);
    } catch (const std::bad_alloc&) {
        return fail(MPC_E_ALLOC, "history slot map");
    }
    for (int k = 0; k < n_hist; ++k) {
        const int e = hist_egos[k];
        if (e < 0 || e >= B) return fail(MPC_E_ARG, "hist_egos: ego index out of range [0, B)");
        if (slot[e] >= 0) return fail(MPC_E_ARG, "hist_egos: ego index repeated");
        slot[e] = k;
    }
    if (B == 0) return MPC_SUCCESS;
    if (!x_init) return fail(MPC_E_ARG, "x_init is required");
    int rc = check_params(&c->p);
    if (rc) return rc;
    const bool per_ego = n_scripts == B && B > 1;    // n_scripts == B == 1 is the shared case
    const int nsc = per_ego ? B : (actors ? 1 : 0);
    if (c->cpu) {
        int hrc = MPC_SUCCESS;
        const int erc = host_call([&] {
            hrc = c->cpu->closed_loop_traffic(c->p, B, x_init, actors, A, nsc == 0 ? 1 : nsc, with_slab, max_steps,
                                              s_stop, quant, extra, n_hist, slot.data(), hist_x, hist_u, hist_car_s,
                                              hist_tl, hist_status, hist_nobs, hist_slab, n_steps, step_ms);
        });
        return erc != MPC_SUCCESS ? erc : hrc;
    }
    KParams kp = kparams(&c->p);
    kp.max_obs = with_slab ? A : 0;          // every actor emits at most one entry
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    const size_t nb = (size_t)B, ns = (size_t)max_steps, nh = (size_t)n_hist, na = (size_t)A;
    const size_t na1 = na ? na : 1;          // no zero-sized allocation
    std::vector<void*> bufs;
    auto dalloc = [&](size_t bytes) -> void* {
        void* ptr = nullptr;
        if (hipMalloc(&ptr, bytes) != hipSuccess) return nullptr;
        bufs.push_back(ptr);
        return ptr;
    };
    auto release = [&]() { for (void* q : bufs) hipFree(q); };
    ClState C = {};                          // obs, obs_s, tl_timer, fsm_flags stay null: TrState holds them
    C.x = (double*)dalloc(nb * 5 * 8);
    C.nobs = (int*)dalloc(nb * 4);
    C.active = (int*)dalloc(nb * 4);
    C.n_active = (int*)dalloc(4);
    C.alist = (int*)dalloc(nb * 4);
    C.n_list = (int*)dalloc(4);
    C.xa = (double*)dalloc(nb * 5 * 8);
    C.obsa = (double*)dalloc(nb * na1 * 2 * 8);
    C.nobsa = (int*)dalloc(nb * 4);
    C.u0a = (double*)dalloc(nb * 2 * 8);
    C.sta = (int*)dalloc(nb * 4);
    double* d_xinit = (double*)dalloc(nb * 5 * 8);
    SwState S = {};
    S.q = (double*)dalloc(nb * MPC_CL_NQ * 8);
    S.qflags = (int*)dalloc(nb * 4);
    int* d_hslot = (int*)dalloc(nb * 4);
    S.hslot = d_hslot;
    S.n_steps = (int*)dalloc(nb * 4);
    TrState T = {};
    mpc_actor* d_actors = (mpc_actor*)dalloc((per_ego ? nb : 1) * na1 * sizeof(mpc_actor));
    T.actors = d_actors;
    T.per_ego = per_ego ? 1 : 0;
    T.aval = (double*)dalloc(nb * na1 * 8);
    T.aflags = (int*)dalloc(nb * na1 * 4);
    T.slab = (double*)dalloc(nb * na1 * 2 * 8);
    T.ex = (double*)dalloc(nb * MPC_TR_NX * 8);
    if (!C.x || !C.nobs || !C.active || !C.n_active || !C.alist || !C.n_list || !C.xa || !C.obsa || !C.nobsa ||
        !C.u0a || !C.sta || !d_xinit || !S.q || !S.qflags || !d_hslot || !S.n_steps || !d_actors || !T.aval ||
        !T.aflags || !T.slab || !T.ex) {
        release();
        return fail(MPC_E_ALLOC, "hipMalloc traffic buffers");
    }
    S.hist_x = hist_x ? (double*)dalloc(nh * (ns + 1) * 5 * 8) : nullptr;
    S.hist_u = hist_u ? (double*)dalloc(nh * ns * 2 * 8) : nullptr;
    S.hist_obs_s = hist_car_s ? (double*)dalloc(nh * ns * 8) : nullptr;
    S.hist_tl = hist_tl ? (int*)dalloc(nh * ns * 4) : nullptr;
    S.hist_status = hist_status ? (int*)dalloc(nh * ns * 4) : nullptr;
    T.hist_nobs = hist_nobs ? (int*)dalloc(nh * ns * 4) : nullptr;
    T.hist_slab = hist_slab ? (double*)dalloc(nh * ns * na * 2 * 8) : nullptr;
    if ((hist_x && !S.hist_x) || (hist_u && !S.hist_u) || (hist_car_s && !S.hist_obs_s) || (hist_tl && !S.hist_tl) ||
        (hist_status && !S.hist_status) || (hist_nobs && !T.hist_nobs) || (hist_slab && !T.hist_slab)) {
        release();
        return fail(MPC_E_ALLOC, "hipMalloc traffic histories");
    }
    hipStream_t st = c->stream;
    hipEvent_t ev[SW_EVENTS] = {};
    auto cleanup = [&]() {
        hipStreamSynchronize(st);
        for (auto& e : ev)
            if (e) hipEventDestroy(e);
        release();
    };
    // steps that never run stay NaN / -1 (all-ones bytes)
    bool ok0 = true;
    if (S.hist_x) ok0 = ok0 && hipMemsetAsync(S.hist_x, 0xff, nh * (ns + 1) * 5 * 8, st) == hipSuccess;
    if (S.hist_u) ok0 = ok0 && hipMemsetAsync(S.hist_u, 0xff, nh * ns * 2 * 8, st) == hipSuccess;
    if (S.hist_obs_s) ok0 = ok0 && hipMemsetAsync(S.hist_obs_s, 0xff, nh * ns * 8, st) == hipSuccess;
    if (S.hist_tl) ok0 = ok0 && hipMemsetAsync(S.hist_tl, 0xff, nh * ns * 4, st) == hipSuccess;
    if (S.hist_status) ok0 = ok0 && hipMemsetAsync(S.hist_status, 0xff, nh * ns * 4, st) == hipSuccess;
    if (T.hist_nobs) ok0 = ok0 && hipMemsetAsync(T.hist_nobs, 0xff, nh * ns * 4, st) == hipSuccess;
    if (T.hist_slab) ok0 = ok0 && hipMemsetAsync(T.hist_slab, 0xff, nh * ns * na * 2 * 8, st) == hipSuccess;
    ok0 = ok0 && hipMemcpyAsync(d_xinit, x_init, nb * 5 * 8, hipMemcpyHostToDevice, st) == hipSuccess;
    ok0 = ok0 && hipMemcpyAsync(d_hslot, slot.data(), nb * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    if (nsc > 0 && A > 0)
        ok0 = ok0 && hipMemcpyAsync(d_actors, actors, (size_t)nsc * na * sizeof(mpc_actor), hipMemcpyHostToDevice,
                                    st) == hipSuccess;
    if (!ok0) {
        cleanup();
        return fail(MPC_E_DEVICE, "traffic buffer initialisation");
    }
    const dim3 tb(256), tg((B + 255) / 256);
    hipLaunchKernelGGL(tr_init_kernel, tg, tb, 0, st, B, A, C, S, T, d_xinit, s_stop, max_steps);
    for (auto& e : ev)
        if (hipEventCreate(&e) != hipSuccess) {
            e = nullptr;
            cleanup();
            return fail(MPC_E_DEVICE, "hipEventCreate (step timing)");
        }
    if (hipEventRecord(ev[0], st) != hipSuccess) {
        cleanup();
        return fail(MPC_E_DEVICE, "hipEventRecord (step timing)");
    }
    // the sweep's ring: step i ran between events i and i + 1, read at a host sync at most 8 steps later
    std::vector<double> ms;
    auto read_times = [&](int upto) {
        for (int i = (int)ms.size(); i < upto; ++i) {
            float t = NAN;
            if (hipEventElapsedTime(&t, ev[i % SW_EVENTS], ev[(i + 1) % SW_EVENTS]) != hipSuccess) t = NAN;
            ms.push_back(t);
        }
    };
    rc = MPC_SUCCESS;
    hipLaunchKernelGGL(cl_compact_kernel, dim3(1), dim3(1024), 0, st, B, C);
    int nl = 0;
    if (hipMemcpyAsync(&nl, C.n_list, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        cleanup();
        return fail(MPC_E_DEVICE, "traffic initial ego list");
    }
    try {
        for (int step = 0; step < max_steps && nl > 0; ++step) {
            hipLaunchKernelGGL(tr_fsm_kernel, tg, tb, 0, st, B, A, kp.dt, C, S, T, step, max_steps);
            const dim3 lg((nl + 255) / 256);
            hipLaunchKernelGGL(tr_gather_kernel, lg, tb, 0, st, nl, B, A, C, T);
            rc = launch_solve(c, kp, nl, C.xa, with_slab ? C.obsa : nullptr, with_slab ? C.nobsa : nullptr, nullptr,
                              C.u0a, nullptr, nullptr, C.sta, nullptr, st);
            if (rc) break;
            if (hipMemsetAsync(C.n_active, 0, 4, st) != hipSuccess) {
                rc = fail(MPC_E_DEVICE, "traffic active-count reset");
                break;
            }
            hipLaunchKernelGGL(sw_plant_kernel, lg, tb, 0, st, c->tab, B, nl, kp.dt, C, S, s_stop, step, max_steps);
            if (hipEventRecord(ev[(step + 1) % SW_EVENTS], st) != hipSuccess) {
                rc = fail(MPC_E_DEVICE, "hipEventRecord (step timing)");
                break;
            }
            if ((step & 7) == 7 || step == max_steps - 1) {     // every 8 steps: has every ego left the loop?
                int nact = 0;
                if (hipMemcpyAsync(&nact, C.n_active, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                    hipStreamSynchronize(st) != hipSuccess) {
                    rc = fail(MPC_E_DEVICE, "traffic step sync");
                    break;
                }
                read_times(step + 1);
                if (nact == 0) break;
                if (nact < nl) {                                // egos left: shrink the solver's list
                    hipLaunchKernelGGL(cl_compact_kernel, dim3(1), dim3(1024), 0, st, B, C);
                    if (hipMemcpyAsync(&nl, C.n_list, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                        hipStreamSynchronize(st) != hipSuccess) {
                        rc = fail(MPC_E_DEVICE, "traffic ego list");
                        break;
                    }
                }
            }
        }
        if (rc == MPC_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(MPC_E_LAUNCH, "traffic kernel launch");
        if (rc == MPC_SUCCESS) {
            std::vector<double> hq(nb * MPC_CL_NQ), hx(extra ? nb * MPC_TR_NX : 0);
            std::vector<int> hn(nb);
            bool ok = hipMemcpyAsync(hn.data(), S.n_steps, nb * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(hq.data(), S.q, nb * MPC_CL_NQ * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (extra) ok = ok && hipMemcpyAsync(hx.data(), T.ex, nb * MPC_TR_NX * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_x) ok = ok && hipMemcpyAsync(hist_x, S.hist_x, nh * (ns + 1) * 5 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_u) ok = ok && hipMemcpyAsync(hist_u, S.hist_u, nh * ns * 2 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_car_s) ok = ok && hipMemcpyAsync(hist_car_s, S.hist_obs_s, nh * ns * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_tl) ok = ok && hipMemcpyAsync(hist_tl, S.hist_tl, nh * ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_status) ok = ok && hipMemcpyAsync(hist_status, S.hist_status, nh * ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_nobs) ok = ok && hipMemcpyAsync(hist_nobs, T.hist_nobs, nh * ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_slab) ok = ok && hipMemcpyAsync(hist_slab, T.hist_slab, nh * ns * na * 2 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && hipStreamSynchronize(st) == hipSuccess;
            if (!ok) {
                rc = fail(MPC_E_DEVICE, "traffic copy-back");
            } else {
                for (size_t b = 0; b < nb; ++b) {             // column-major on the device -> one row per ego
                    for (int k = 0; k < MPC_CL_NQ; ++k) quant[b * MPC_CL_NQ + k] = hq[(size_t)k * nb + b];
                    if (extra)
                        for (int k = 0; k < MPC_TR_NX; ++k) extra[b * MPC_TR_NX + k] = hx[(size_t)k * nb + b];
                }
                mpcqp_cpu::sweep_max_step_ms(B, hn.data(), ms, quant);
                if (n_steps) std::memcpy(n_steps, hn.data(), nb * 4);
                if (step_ms)
                    for (size_t i = 0; i < ns; ++i) step_ms[i] = i < ms.size() ? ms[i] : (double)NAN;
            }
        }
    } catch (const std::bad_alloc&) {
        rc = fail(MPC_E_ALLOC, "traffic host buffers");
    }
    cleanup();
    return rc;
}

// mpc_closed_loop_traffic with the egos of a world as each other's obstacles (include/mpcqp.h): the same loop,
// with cv_lead_kernel between tr_fsm_kernel and the gather and an (A + K)-wide slab.  Device allocations: the
// traffic entry's with A + K for the slab width, and hist_lead [n_hist][max_steps][K]:
// O(B * (A + K)) + O(n_hist * max_steps * (A + K))
extern "C" int mpc_closed_loop_convoy(mpc_ctx* c, int B, int W, int K, double lead_range, const double* x_init,
                                      const mpc_actor* actors, int A, int n_scripts, int max_steps, double s_stop,
                                      double* quant, double* extra, int n_hist, const int* hist_egos, double* hist_x,
                                      double* hist_u, double* hist_car_s, int* hist_tl, int* hist_status,
                                      int* hist_nobs, double* hist_slab, int* hist_lead, int* n_steps,
                                      double* step_ms) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0 || max_steps < 1) return fail(MPC_E_ARG, "B < 0 or max_steps < 1");
    if (W < 1 || W > MPC_MAX_WORLD) return fail(MPC_E_ARG, "W out of range [1, 256]");
    if (B % W != 0) return fail(MPC_E_ARG, "B is not a multiple of W");
    if (A < 0 || A > MPC_MAX_ACTORS) return fail(MPC_E_ARG, "A out of range [0, 16]");
    if (K < 0 || K > MPC_MAX_ACTORS) return fail(MPC_E_ARG, "K out of range [0, 16]");
    if (A + K > MPC_MAX_ACTORS) return fail(MPC_E_ARG, "A + K > 16");
    if (!(lead_range > 0.0)) return fail(MPC_E_ARG, "lead_range must be > 0 (+inf allowed)");
    if (actors ? !(n_scripts == 1 || n_scripts == B) : n_scripts != 0)
        return fail(MPC_E_ARG, "n_scripts must be B (a script per ego), 1 (shared) or 0 with actors NULL");
    if (!actors && A != 0) return fail(MPC_E_ARG, "actors is NULL but A > 0");
    if (!quant) return fail(MPC_E_ARG, "quant is required");
    if (n_hist < 0) return fail(MPC_E_ARG, "n_hist < 0");
    if (n_hist == 0 &&
        (hist_x || hist_u || hist_car_s || hist_tl || hist_status || hist_nobs || hist_slab || hist_lead))
        return fail(MPC_E_ARG, "a history array is given but n_hist == 0");
    if (hist_slab && A + K == 0) return fail(MPC_E_ARG, "hist_slab is given but A + K == 0");
    if (hist_lead && K == 0) return fail(MPC_E_ARG, "hist_lead is given but K == 0");
    if (n_hist > 0 && !hist_egos) return fail(MPC_E_ARG, "hist_egos is NULL but n_hist > 0");
    bool with_slab = K > 0 && W > 1;
    for (size_t k = 0; k < (size_t)n_scripts * (size_t)A; ++k) {
        if (actors[k].kind < MPC_ACTOR_NONE || actors[k].kind > MPC_ACTOR_LIGHT)
            return fail(MPC_E_ARG, "actor kind outside MPC_ACTOR_NONE .. MPC_ACTOR_LIGHT");
        with_slab = with_slab || actors[k].kind != MPC_ACTOR_NONE;
    }
    std::vector<int> slot;
    try {
        slot.assign((size_t)B, -1);
    } catch (const std::bad_alloc&) {
        return fail(MPC_E_ALLOC, "history slot map");
    }
    for (int k = 0; k < n_hist; ++k) {
        const int e = hist_egos[k];
        if (e < 0 || e >= B) return fail(MPC_E_ARG, "hist_egos: ego index out of range [0, B)");
        if (slot[e] >= 0) return fail(MPC_E_ARG, "hist_egos: ego index repeated");
        slot[e] = k;
    }
    if (B == 0) return MPC_SUCCESS;
    if (!x_init) return fail(MPC_E_ARG, "x_init is required");
    int rc = check_params(&c->p);
    if (rc) return rc;
    const bool per_ego = n_scripts == B && B > 1;    // n_scripts == B == 1 is the shared case
    const int nsc = per_ego ? B : (actors ? 1 : 0);
    const int AK = A + K;
    if (c->cpu) {
        int hrc = MPC_SUCCESS;
        const int erc = host_call([&] {
            hrc = c->cpu->closed_loop_convoy(c->p, B, W, K, lead_range, x_init, actors, A, nsc == 0 ? 1 : nsc,
                                             with_slab, max_steps, s_stop, quant, extra, n_hist, slot.data(), hist_x,
                                             hist_u, hist_car_s, hist_tl, hist_status, hist_nobs, hist_slab, hist_lead,
                                             n_steps, step_ms);
        });
        return erc != MPC_SUCCESS ? erc : hrc;
    }
    KParams kp = kparams(&c->p);
    kp.max_obs = with_slab ? AK : 0;         // every actor and every leader adds at most one entry
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    const size_t nb = (size_t)B, ns = (size_t)max_steps, nh = (size_t)n_hist, na = (size_t)A, nk = (size_t)K;
    const size_t nak = (size_t)AK;
    const size_t na1 = na ? na : 1, nak1 = nak ? nak : 1;    // no zero-sized allocation
    std::vector<void*> bufs;
    auto dalloc = [&](size_t bytes) -> void* {
        void* ptr = nullptr;
        if (hipMalloc(&ptr, bytes) != hipSuccess) return nullptr;
        bufs.push_back(ptr);
        return ptr;
    };
    auto release = [&]() { for (void* q : bufs) hipFree(q); };
    ClState C = {};                          // obs, obs_s, tl_timer, fsm_flags stay null: TrState holds them
    C.x = (double*)dalloc(nb * 5 * 8);
    C.nobs = (int*)dalloc(nb * 4);
    C.active = (int*)dalloc(nb * 4);
    C.n_active = (int*)dalloc(4);
    C.alist = (int*)dalloc(nb * 4);
    C.n_list = (int*)dalloc(4);
    C.xa = (double*)dalloc(nb * 5 * 8);
    C.obsa = (double*)dalloc(nb * nak1 * 2 * 8);
    C.nobsa = (int*)dalloc(nb * 4);
    C.u0a = (double*)dalloc(nb * 2 * 8);
    C.sta = (int*)dalloc(nb * 4);
    double* d_xinit = (double*)dalloc(nb * 5 * 8);
    SwState S = {};
    S.q = (double*)dalloc(nb * MPC_CL_NQ * 8);
    S.qflags = (int*)dalloc(nb * 4);
    int* d_hslot = (int*)dalloc(nb * 4);
    S.hslot = d_hslot;
    S.n_steps = (int*)dalloc(nb * 4);
    TrState T = {};
    mpc_actor* d_actors = (mpc_actor*)dalloc((per_ego ? nb : 1) * na1 * sizeof(mpc_actor));
    T.actors = d_actors;
    T.per_ego = per_ego ? 1 : 0;
    T.aval = (double*)dalloc(nb * na1 * 8);
    T.aflags = (int*)dalloc(nb * na1 * 4);
    T.slab = (double*)dalloc(nb * nak1 * 2 * 8);
    T.ex = (double*)dalloc(nb * MPC_CV_NX * 8);
    if (!C.x || !C.nobs || !C.active || !C.n_active || !C.alist || !C.n_list || !C.xa || !C.obsa || !C.nobsa ||
        !C.u0a || !C.sta || !d_xinit || !S.q || !S.qflags || !d_hslot || !S.n_steps || !d_actors || !T.aval ||
        !T.aflags || !T.slab || !T.ex) {
        release();
        return fail(MPC_E_ALLOC, "hipMalloc convoy buffers");
    }
    CvState V = {};
    V.W = W;
    V.K = K;
    V.lead_range = lead_range;
    S.hist_x = hist_x ? (double*)dalloc(nh * (ns + 1) * 5 * 8) : nullptr;
    S.hist_u = hist_u ? (double*)dalloc(nh * ns * 2 * 8) : nullptr;
    S.hist_obs_s = hist_car_s ? (double*)dalloc(nh * ns * 8) : nullptr;
    S.hist_tl = hist_tl ? (int*)dalloc(nh * ns * 4) : nullptr;
    S.hist_status = hist_status ? (int*)dalloc(nh * ns * 4) : nullptr;
    T.hist_nobs = hist_nobs ? (int*)dalloc(nh * ns * 4) : nullptr;
    T.hist_slab = nullptr;                   // tr_fsm_kernel's rows are A wide: cv_lead_kernel writes the rows
    V.hist_slab = hist_slab ? (double*)dalloc(nh * ns * nak * 2 * 8) : nullptr;
    V.hist_lead = hist_lead ? (int*)dalloc(nh * ns * nk * 4) : nullptr;
    if ((hist_x && !S.hist_x) || (hist_u && !S.hist_u) || (hist_car_s && !S.hist_obs_s) || (hist_tl && !S.hist_tl) ||
        (hist_status && !S.hist_status) || (hist_nobs && !T.hist_nobs) || (hist_slab && !V.hist_slab) ||
        (hist_lead && !V.hist_lead)) {
        release();
        return fail(MPC_E_ALLOC, "hipMalloc convoy histories");
    }
    hipStream_t st = c->stream;
    hipEvent_t ev[SW_EVENTS] = {};
    auto cleanup = [&]() {
        hipStreamSynchronize(st);
        for (auto& e : ev)
            if (e) hipEventDestroy(e);
        release();
    };
    // steps that never run stay NaN / -1 (all-ones bytes)
    bool ok0 = true;
    if (S.hist_x) ok0 = ok0 && hipMemsetAsync(S.hist_x, 0xff, nh * (ns + 1) * 5 * 8, st) == hipSuccess;
    if (S.hist_u) ok0 = ok0 && hipMemsetAsync(S.hist_u, 0xff, nh * ns * 2 * 8, st) == hipSuccess;
    if (S.hist_obs_s) ok0 = ok0 && hipMemsetAsync(S.hist_obs_s, 0xff, nh * ns * 8, st) == hipSuccess;
    if (S.hist_tl) ok0 = ok0 && hipMemsetAsync(S.hist_tl, 0xff, nh * ns * 4, st) == hipSuccess;
    if (S.hist_status) ok0 = ok0 && hipMemsetAsync(S.hist_status, 0xff, nh * ns * 4, st) == hipSuccess;
    if (T.hist_nobs) ok0 = ok0 && hipMemsetAsync(T.hist_nobs, 0xff, nh * ns * 4, st) == hipSuccess;
    if (V.hist_slab) ok0 = ok0 && hipMemsetAsync(V.hist_slab, 0xff, nh * ns * nak * 2 * 8, st) == hipSuccess;
    if (V.hist_lead) ok0 = ok0 && hipMemsetAsync(V.hist_lead, 0xff, nh * ns * nk * 4, st) == hipSuccess;
    ok0 = ok0 && hipMemcpyAsync(d_xinit, x_init, nb * 5 * 8, hipMemcpyHostToDevice, st) == hipSuccess;
    ok0 = ok0 && hipMemcpyAsync(d_hslot, slot.data(), nb * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    if (nsc > 0 && A > 0)
        ok0 = ok0 && hipMemcpyAsync(d_actors, actors, (size_t)nsc * na * sizeof(mpc_actor), hipMemcpyHostToDevice,
                                    st) == hipSuccess;
    if (!ok0) {
        cleanup();
        return fail(MPC_E_DEVICE, "convoy buffer initialisation");
    }
    const dim3 tb(256), tg((B + 255) / 256);
    const dim3 wb(64 * ((W + 63) / 64)), wg(B / W);          // a workgroup per world
    hipLaunchKernelGGL(tr_init_kernel, tg, tb, 0, st, B, A, C, S, T, d_xinit, s_stop, max_steps);
    hipLaunchKernelGGL(cv_init_kernel, tg, tb, 0, st, B, T);
    for (auto& e : ev)
        if (hipEventCreate(&e) != hipSuccess) {
            e = nullptr;
            cleanup();
            return fail(MPC_E_DEVICE, "hipEventCreate (step timing)");
        }
    if (hipEventRecord(ev[0], st) != hipSuccess) {
        cleanup();
        return fail(MPC_E_DEVICE, "hipEventRecord (step timing)");
    }
    // the sweep's ring: step i ran between events i and i + 1, read at a host sync at most 8 steps later
    std::vector<double> ms;
    auto read_times = [&](int upto) {
        for (int i = (int)ms.size(); i < upto; ++i) {
            float t = NAN;
            if (hipEventElapsedTime(&t, ev[i % SW_EVENTS], ev[(i + 1) % SW_EVENTS]) != hipSuccess) t = NAN;
            ms.push_back(t);
        }
    };
    rc = MPC_SUCCESS;
    hipLaunchKernelGGL(cl_compact_kernel, dim3(1), dim3(1024), 0, st, B, C);
    int nl = 0;
    if (hipMemcpyAsync(&nl, C.n_list, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        cleanup();
        return fail(MPC_E_DEVICE, "convoy initial ego list");
    }
    try {
        for (int step = 0; step < max_steps && nl > 0; ++step) {
            hipLaunchKernelGGL(tr_fsm_kernel, tg, tb, 0, st, B, A, kp.dt, C, S, T, step, max_steps);
            hipLaunchKernelGGL(cv_lead_kernel, wg, wb, 0, st, B, A, C, S, T, V, step, max_steps);
            const dim3 lg((nl + 255) / 256);
            hipLaunchKernelGGL(tr_gather_kernel, lg, tb, 0, st, nl, B, AK, C, T);
            rc = launch_solve(c, kp, nl, C.xa, with_slab ? C.obsa : nullptr, with_slab ? C.nobsa : nullptr, nullptr,
                              C.u0a, nullptr, nullptr, C.sta, nullptr, st);
            if (rc) break;
            if (hipMemsetAsync(C.n_active, 0, 4, st) != hipSuccess) {
                rc = fail(MPC_E_DEVICE, "convoy active-count reset");
                break;
            }
            hipLaunchKernelGGL(sw_plant_kernel, lg, tb, 0, st, c->tab, B, nl, kp.dt, C, S, s_stop, step, max_steps);
            if (hipEventRecord(ev[(step + 1) % SW_EVENTS], st) != hipSuccess) {
                rc = fail(MPC_E_DEVICE, "hipEventRecord (step timing)");
                break;
            }
            if ((step & 7) == 7 || step == max_steps - 1) {     // every 8 steps: has every ego left the loop?
                int nact = 0;
                if (hipMemcpyAsync(&nact, C.n_active, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                    hipStreamSynchronize(st) != hipSuccess) {
                    rc = fail(MPC_E_DEVICE, "convoy step sync");
                    break;
                }
                read_times(step + 1);
                if (nact == 0) break;
                if (nact < nl) {                                // egos left: shrink the solver's list
                    hipLaunchKernelGGL(cl_compact_kernel, dim3(1), dim3(1024), 0, st, B, C);
                    if (hipMemcpyAsync(&nl, C.n_list, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                        hipStreamSynchronize(st) != hipSuccess) {
                        rc = fail(MPC_E_DEVICE, "convoy ego list");
                        break;
                    }
                }
            }
        }
        if (rc == MPC_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(MPC_E_LAUNCH, "convoy kernel launch");
        if (rc == MPC_SUCCESS) {
            std::vector<double> hq(nb * MPC_CL_NQ), hx(extra ? nb * MPC_CV_NX : 0);
            std::vector<int> hn(nb);
            bool ok = hipMemcpyAsync(hn.data(), S.n_steps, nb * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(hq.data(), S.q, nb * MPC_CL_NQ * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (extra) ok = ok && hipMemcpyAsync(hx.data(), T.ex, nb * MPC_CV_NX * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_x) ok = ok && hipMemcpyAsync(hist_x, S.hist_x, nh * (ns + 1) * 5 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_u) ok = ok && hipMemcpyAsync(hist_u, S.hist_u, nh * ns * 2 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_car_s) ok = ok && hipMemcpyAsync(hist_car_s, S.hist_obs_s, nh * ns * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_tl) ok = ok && hipMemcpyAsync(hist_tl, S.hist_tl, nh * ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_status) ok = ok && hipMemcpyAsync(hist_status, S.hist_status, nh * ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_nobs) ok = ok && hipMemcpyAsync(hist_nobs, T.hist_nobs, nh * ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_slab) ok = ok && hipMemcpyAsync(hist_slab, V.hist_slab, nh * ns * nak * 2 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_lead) ok = ok && hipMemcpyAsync(hist_lead, V.hist_lead, nh * ns * nk * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && hipStreamSynchronize(st) == hipSuccess;
            if (!ok) {
                rc = fail(MPC_E_DEVICE, "convoy copy-back");
            } else {
                for (size_t b = 0; b < nb; ++b) {             // column-major on the device -> one row per ego
                    for (int k = 0; k < MPC_CL_NQ; ++k) quant[b * MPC_CL_NQ + k] = hq[(size_t)k * nb + b];
                    if (extra)
                        for (int k = 0; k < MPC_CV_NX; ++k) extra[b * MPC_CV_NX + k] = hx[(size_t)k * nb + b];
                }
                mpcqp_cpu::sweep_max_step_ms(B, hn.data(), ms, quant);
                if (n_steps) std::memcpy(n_steps, hn.data(), nb * 4);
                if (step_ms)
                    for (size_t i = 0; i < ns; ++i) step_ms[i] = i < ms.size() ? ms[i] : (double)NAN;
            }
        }
    } catch (const std::bad_alloc&) {
        rc = fail(MPC_E_ALLOC, "convoy host buffers");
    }
    cleanup();
    return rc;
}

extern "C" void mpc_default_noise(mpc_noise* n) { std::memset(n, 0, sizeof(*n)); }

// mpc_closed_loop_convoy with seeded noise between the world and the solver (include/mpcqp.h): the same loop with
// nz_measure_kernel for tr_gather_kernel and nz_plant_kernel for sw_plant_kernel; tr_fsm_kernel, cv_lead_kernel,
// cl_compact_kernel and launch_solve are reused untouched and see the true states.  noise == NULL runs the same
// kernels on an all-zero shared struct.  Device allocations: the convoy entry's, extras MPC_NZ_NX wide, the
// field-major sigma table [14][B] for per-ego noise, hist_ua and hist_xm:
// O(B * (A + K)) + O(n_hist * max_steps * (A + K))
extern "C" int mpc_closed_loop_noisy(mpc_ctx* c, int B, int W, int K, double lead_range, const double* x_init,
                                     const mpc_actor* actors, int A, int n_scripts, const mpc_noise* noise,
                                     int n_noise, unsigned long long seed, long long ego_offset, int max_steps,
                                     double s_stop, double* quant, double* extra, int n_hist, const int* hist_egos,
                                     double* hist_x, double* hist_u, double* hist_ua, double* hist_xm,
                                     double* hist_car_s, int* hist_tl, int* hist_status, int* hist_nobs,
                                     double* hist_slab, int* hist_lead, int* n_steps, double* step_ms) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0 || max_steps < 1) return fail(MPC_E_ARG, "B < 0 or max_steps < 1");
    if (W < 1 || W > MPC_MAX_WORLD) return fail(MPC_E_ARG, "W out of range [1, 256]");
    if (B % W != 0) return fail(MPC_E_ARG, "B is not a multiple of W");
    if (A < 0 || A > MPC_MAX_ACTORS) return fail(MPC_E_ARG, "A out of range [0, 16]");
    if (K < 0 || K > MPC_MAX_ACTORS) return fail(MPC_E_ARG, "K out of range [0, 16]");
    if (A + K > MPC_MAX_ACTORS) return fail(MPC_E_ARG, "A + K > 16");
    if (!(lead_range > 0.0)) return fail(MPC_E_ARG, "lead_range must be > 0 (+inf allowed)");
    if (actors ? !(n_scripts == 1 || n_scripts == B) : n_scripts != 0)
        return fail(MPC_E_ARG, "n_scripts must be B (a script per ego), 1 (shared) or 0 with actors NULL");
    if (!actors && A != 0) return fail(MPC_E_ARG, "actors is NULL but A > 0");
    if (noise ? !(n_noise == 1 || n_noise == B) : n_noise != 0)
        return fail(MPC_E_ARG, "n_noise must be B (a struct per ego), 1 (shared) or 0 with noise NULL");
    if (ego_offset < 0) return fail(MPC_E_ARG, "ego_offset < 0");
    if (!quant) return fail(MPC_E_ARG, "quant is required");
    if (n_hist < 0) return fail(MPC_E_ARG, "n_hist < 0");
    if (n_hist == 0 && (hist_x || hist_u || hist_ua || hist_xm || hist_car_s || hist_tl || hist_status || hist_nobs ||
                        hist_slab || hist_lead))
        return fail(MPC_E_ARG, "a history array is given but n_hist == 0");
    if (hist_slab && A + K == 0) return fail(MPC_E_ARG, "hist_slab is given but A + K == 0");
    if (hist_lead && K == 0) return fail(MPC_E_ARG, "hist_lead is given but K == 0");
    if (n_hist > 0 && !hist_egos) return fail(MPC_E_ARG, "hist_egos is NULL but n_hist > 0");
    bool with_slab = K > 0 && W > 1;
    for (size_t k = 0; k < (size_t)n_scripts * (size_t)A; ++k) {
        if (actors[k].kind < MPC_ACTOR_NONE || actors[k].kind > MPC_ACTOR_LIGHT)
            return fail(MPC_E_ARG, "actor kind outside MPC_ACTOR_NONE .. MPC_ACTOR_LIGHT");
        with_slab = with_slab || actors[k].kind != MPC_ACTOR_NONE;
    }
    for (size_t k = 0; k < (size_t)n_noise * NZ_NSIG; ++k)       // mpc_noise is NZ_NSIG doubles, no padding
        if (!(reinterpret_cast<const double*>(noise)[k] >= 0.0))
            return fail(MPC_E_ARG, "a noise sigma is negative or NaN");
    std::vector<int> slot;
    try {
        slot.assign((size_t)B, -1);
    } catch (const std::bad_alloc&) {
        return fail(MPC_E_ALLOC, "history slot map");
    }
    for (int k = 0; k < n_hist; ++k) {
        const int e = hist_egos[k];
        if (e < 0 || e >= B) return fail(MPC_E_ARG, "hist_egos: ego index out of range [0, B)");
        if (slot[e] >= 0) return fail(MPC_E_ARG, "hist_egos: ego index repeated");
        slot[e] = k;
    }
    if (B == 0) return MPC_SUCCESS;
    if (!x_init) return fail(MPC_E_ARG, "x_init is required");
    int rc = check_params(&c->p);
    if (rc) return rc;
    const bool per_ego = n_scripts == B && B > 1;    // n_scripts == B == 1 is the shared case
    const int nsc = per_ego ? B : (actors ? 1 : 0);
    const bool nz_per_ego = n_noise == B && B > 1;
    mpc_noise zero;
    mpc_default_noise(&zero);
    if (!noise) noise = &zero;
    const int AK = A + K;
    if (c->cpu) {
        int hrc = MPC_SUCCESS;
        const int erc = host_call([&] {
            hrc = c->cpu->closed_loop_noisy(c->p, B, W, K, lead_range, x_init, actors, A, nsc == 0 ? 1 : nsc, with_slab,
                                            noise, nz_per_ego ? B : 1, seed, ego_offset, max_steps, s_stop, quant,
                                            extra, n_hist, slot.data(), hist_x, hist_u, hist_ua, hist_xm, hist_car_s,
                                            hist_tl, hist_status, hist_nobs, hist_slab, hist_lead, n_steps, step_ms);
        });
        return erc != MPC_SUCCESS ? erc : hrc;
    }
    KParams kp = kparams(&c->p);
    kp.max_obs = with_slab ? AK : 0;         // every actor and every leader adds at most one entry
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    const size_t nb = (size_t)B, ns = (size_t)max_steps, nh = (size_t)n_hist, na = (size_t)A, nk = (size_t)K;
    const size_t nak = (size_t)AK;
    const size_t na1 = na ? na : 1, nak1 = nak ? nak : 1;    // no zero-sized allocation
    std::vector<double> hsig;                // per-ego sigmas, field-major: the loads of a wave coalesce
    if (nz_per_ego) {
        try {
            hsig.resize(nb * NZ_NSIG);
        } catch (const std::bad_alloc&) {
            return fail(MPC_E_ALLOC, "noise table");
        }
        for (size_t b = 0; b < nb; ++b)
            for (size_t f = 0; f < NZ_NSIG; ++f) hsig[f * nb + b] = reinterpret_cast<const double*>(noise + b)[f];
    }
    std::vector<void*> bufs;
    auto dalloc = [&](size_t bytes) -> void* {
        void* ptr = nullptr;
        if (hipMalloc(&ptr, bytes) != hipSuccess) return nullptr;
        bufs.push_back(ptr);
        return ptr;
    };
    auto release = [&]() { for (void* q : bufs) hipFree(q); };
    ClState C = {};                          // obs, obs_s, tl_timer, fsm_flags stay null: TrState holds them
    C.x = (double*)dalloc(nb * 5 * 8);
    C.nobs = (int*)dalloc(nb * 4);
    C.active = (int*)dalloc(nb * 4);
    C.n_active = (int*)dalloc(4);
    C.alist = (int*)dalloc(nb * 4);
    C.n_list = (int*)dalloc(4);
    C.xa = (double*)dalloc(nb * 5 * 8);
    C.obsa = (double*)dalloc(nb * nak1 * 2 * 8);
    C.nobsa = (int*)dalloc(nb * 4);
    C.u0a = (double*)dalloc(nb * 2 * 8);
    C.sta = (int*)dalloc(nb * 4);
    double* d_xinit = (double*)dalloc(nb * 5 * 8);
    SwState S = {};
    S.q = (double*)dalloc(nb * MPC_CL_NQ * 8);
    S.qflags = (int*)dalloc(nb * 4);
    int* d_hslot = (int*)dalloc(nb * 4);
    S.hslot = d_hslot;
    S.n_steps = (int*)dalloc(nb * 4);
    TrState T = {};
    mpc_actor* d_actors = (mpc_actor*)dalloc((per_ego ? nb : 1) * na1 * sizeof(mpc_actor));
    T.actors = d_actors;
    T.per_ego = per_ego ? 1 : 0;
    T.aval = (double*)dalloc(nb * na1 * 8);
    T.aflags = (int*)dalloc(nb * na1 * 4);
    T.slab = (double*)dalloc(nb * nak1 * 2 * 8);
    T.ex = (double*)dalloc(nb * MPC_NZ_NX * 8);
    double* d_sig = nz_per_ego ? (double*)dalloc(nb * NZ_NSIG * 8) : nullptr;
    if (!C.x || !C.nobs || !C.active || !C.n_active || !C.alist || !C.n_list || !C.xa || !C.obsa || !C.nobsa ||
        !C.u0a || !C.sta || !d_xinit || !S.q || !S.qflags || !d_hslot || !S.n_steps || !d_actors || !T.aval ||
        !T.aflags || !T.slab || !T.ex || (nz_per_ego && !d_sig)) {
        release();
        return fail(MPC_E_ALLOC, "hipMalloc noisy-loop buffers");
    }
    CvState V = {};
    V.W = W;
    V.K = K;
    V.lead_range = lead_range;
    NzState Z = {};
    Z.sig = d_sig;
    Z.shared = nz_per_ego ? zero : noise[0];
    Z.k0 = (unsigned)(seed & 0xffffffffull);
    Z.k1 = (unsigned)(seed >> 32);
    Z.g0 = (unsigned long long)ego_offset;
    Z.u_min0 = c->p.u_min[0];
    Z.u_min1 = c->p.u_min[1];
    Z.u_max0 = c->p.u_max[0];
    Z.u_max1 = c->p.u_max[1];
    S.hist_x = hist_x ? (double*)dalloc(nh * (ns + 1) * 5 * 8) : nullptr;
    S.hist_u = hist_u ? (double*)dalloc(nh * ns * 2 * 8) : nullptr;
    Z.hist_ua = hist_ua ? (double*)dalloc(nh * ns * 2 * 8) : nullptr;
    Z.hist_xm = hist_xm ? (double*)dalloc(nh * ns * 5 * 8) : nullptr;
    S.hist_obs_s = hist_car_s ? (double*)dalloc(nh * ns * 8) : nullptr;
    S.hist_tl = hist_tl ? (int*)dalloc(nh * ns * 4) : nullptr;
    S.hist_status = hist_status ? (int*)dalloc(nh * ns * 4) : nullptr;
    T.hist_nobs = hist_nobs ? (int*)dalloc(nh * ns * 4) : nullptr;
    T.hist_slab = nullptr;                   // tr_fsm_kernel's rows are A wide: cv_lead_kernel writes the rows
    V.hist_slab = hist_slab ? (double*)dalloc(nh * ns * nak * 2 * 8) : nullptr;
    V.hist_lead = hist_lead ? (int*)dalloc(nh * ns * nk * 4) : nullptr;
    if ((hist_x && !S.hist_x) || (hist_u && !S.hist_u) || (hist_ua && !Z.hist_ua) || (hist_xm && !Z.hist_xm) ||
        (hist_car_s && !S.hist_obs_s) || (hist_tl && !S.hist_tl) || (hist_status && !S.hist_status) ||
        (hist_nobs && !T.hist_nobs) || (hist_slab && !V.hist_slab) || (hist_lead && !V.hist_lead)) {
        release();
        return fail(MPC_E_ALLOC, "hipMalloc noisy-loop histories");
    }
    hipStream_t st = c->stream;
    hipEvent_t ev[SW_EVENTS] = {};
    auto cleanup = [&]() {
        hipStreamSynchronize(st);
        for (auto& e : ev)
            if (e) hipEventDestroy(e);
        release();
    };
    // steps that never run stay NaN / -1 (all-ones bytes)
    bool ok0 = true;
    if (S.hist_x) ok0 = ok0 && hipMemsetAsync(S.hist_x, 0xff, nh * (ns + 1) * 5 * 8, st) == hipSuccess;
    if (S.hist_u) ok0 = ok0 && hipMemsetAsync(S.hist_u, 0xff, nh * ns * 2 * 8, st) == hipSuccess;
    if (Z.hist_ua) ok0 = ok0 && hipMemsetAsync(Z.hist_ua, 0xff, nh * ns * 2 * 8, st) == hipSuccess;
    if (Z.hist_xm) ok0 = ok0 && hipMemsetAsync(Z.hist_xm, 0xff, nh * ns * 5 * 8, st) == hipSuccess;
    if (S.hist_obs_s) ok0 = ok0 && hipMemsetAsync(S.hist_obs_s, 0xff, nh * ns * 8, st) == hipSuccess;
    if (S.hist_tl) ok0 = ok0 && hipMemsetAsync(S.hist_tl, 0xff, nh * ns * 4, st) == hipSuccess;
    if (S.hist_status) ok0 = ok0 && hipMemsetAsync(S.hist_status, 0xff, nh * ns * 4, st) == hipSuccess;
    if (T.hist_nobs) ok0 = ok0 && hipMemsetAsync(T.hist_nobs, 0xff, nh * ns * 4, st) == hipSuccess;
    if (V.hist_slab) ok0 = ok0 && hipMemsetAsync(V.hist_slab, 0xff, nh * ns * nak * 2 * 8, st) == hipSuccess;
    if (V.hist_lead) ok0 = ok0 && hipMemsetAsync(V.hist_lead, 0xff, nh * ns * nk * 4, st) == hipSuccess;
    ok0 = ok0 && hipMemcpyAsync(d_xinit, x_init, nb * 5 * 8, hipMemcpyHostToDevice, st) == hipSuccess;
    ok0 = ok0 && hipMemcpyAsync(d_hslot, slot.data(), nb * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    if (nsc > 0 && A > 0)
        ok0 = ok0 && hipMemcpyAsync(d_actors, actors, (size_t)nsc * na * sizeof(mpc_actor), hipMemcpyHostToDevice,
                                    st) == hipSuccess;
    if (nz_per_ego)
        ok0 = ok0 && hipMemcpyAsync(d_sig, hsig.data(), nb * NZ_NSIG * 8, hipMemcpyHostToDevice, st) == hipSuccess;
    if (!ok0) {
        cleanup();
        return fail(MPC_E_DEVICE, "noisy-loop buffer initialisation");
    }
    const dim3 tb(256), tg((B + 255) / 256);
    const dim3 wb(64 * ((W + 63) / 64)), wg(B / W);          // a workgroup per world
    hipLaunchKernelGGL(tr_init_kernel, tg, tb, 0, st, B, A, C, S, T, d_xinit, s_stop, max_steps);
    hipLaunchKernelGGL(cv_init_kernel, tg, tb, 0, st, B, T);
    hipLaunchKernelGGL(nz_init_kernel, tg, tb, 0, st, B, T);
    for (auto& e : ev)
        if (hipEventCreate(&e) != hipSuccess) {
            e = nullptr;
            cleanup();
            return fail(MPC_E_DEVICE, "hipEventCreate (step timing)");
        }
    if (hipEventRecord(ev[0], st) != hipSuccess) {
        cleanup();
        return fail(MPC_E_DEVICE, "hipEventRecord (step timing)");
    }
    // the sweep's ring: step i ran between events i and i + 1, read at a host sync at most 8 steps later
    std::vector<double> ms;
    auto read_times = [&](int upto) {
        for (int i = (int)ms.size(); i < upto; ++i) {
            float t = NAN;
            if (hipEventElapsedTime(&t, ev[i % SW_EVENTS], ev[(i + 1) % SW_EVENTS]) != hipSuccess) t = NAN;
            ms.push_back(t);
        }
    };
    rc = MPC_SUCCESS;
    hipLaunchKernelGGL(cl_compact_kernel, dim3(1), dim3(1024), 0, st, B, C);
    int nl = 0;
    if (hipMemcpyAsync(&nl, C.n_list, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        cleanup();
        return fail(MPC_E_DEVICE, "noisy-loop initial ego list");
    }
    try {
        for (int step = 0; step < max_steps && nl > 0; ++step) {
            hipLaunchKernelGGL(tr_fsm_kernel, tg, tb, 0, st, B, A, kp.dt, C, S, T, step, max_steps);
            hipLaunchKernelGGL(cv_lead_kernel, wg, wb, 0, st, B, A, C, S, T, V, step, max_steps);
            const dim3 lg((nl + 255) / 256);
            hipLaunchKernelGGL(nz_measure_kernel, lg, tb, 0, st, nl, B, AK, C, S, T, Z, step, max_steps);
            rc = launch_solve(c, kp, nl, C.xa, with_slab ? C.obsa : nullptr, with_slab ? C.nobsa : nullptr, nullptr,
                              C.u0a, nullptr, nullptr, C.sta, nullptr, st);
            if (rc) break;
            if (hipMemsetAsync(C.n_active, 0, 4, st) != hipSuccess) {
                rc = fail(MPC_E_DEVICE, "noisy-loop active-count reset");
                break;
            }
            hipLaunchKernelGGL(nz_plant_kernel, lg, tb, 0, st, c->tab, B, nl, kp.dt, C, S, T, Z, s_stop, step,
                               max_steps);
            if (hipEventRecord(ev[(step + 1) % SW_EVENTS], st) != hipSuccess) {
                rc = fail(MPC_E_DEVICE, "hipEventRecord (step timing)");
                break;
            }
            if ((step & 7) == 7 || step == max_steps - 1) {     // every 8 steps: has every ego left the loop?
                int nact = 0;
                if (hipMemcpyAsync(&nact, C.n_active, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                    hipStreamSynchronize(st) != hipSuccess) {
                    rc = fail(MPC_E_DEVICE, "noisy-loop step sync");
                    break;
                }
                read_times(step + 1);
                if (nact == 0) break;
                if (nact < nl) {                                // egos left: shrink the solver's list
                    hipLaunchKernelGGL(cl_compact_kernel, dim3(1), dim3(1024), 0, st, B, C);
                    if (hipMemcpyAsync(&nl, C.n_list, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                        hipStreamSynchronize(st) != hipSuccess) {
                        rc = fail(MPC_E_DEVICE, "noisy-loop ego list");
                        break;
                    }
                }
            }
        }
        if (rc == MPC_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(MPC_E_LAUNCH, "noisy-loop kernel launch");
        if (rc == MPC_SUCCESS) {
            std::vector<double> hq(nb * MPC_CL_NQ), hx(extra ? nb * MPC_NZ_NX : 0);
            std::vector<int> hn(nb);
            bool ok = hipMemcpyAsync(hn.data(), S.n_steps, nb * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(hq.data(), S.q, nb * MPC_CL_NQ * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (extra) ok = ok && hipMemcpyAsync(hx.data(), T.ex, nb * MPC_NZ_NX * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_x) ok = ok && hipMemcpyAsync(hist_x, S.hist_x, nh * (ns + 1) * 5 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_u) ok = ok && hipMemcpyAsync(hist_u, S.hist_u, nh * ns * 2 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_ua) ok = ok && hipMemcpyAsync(hist_ua, Z.hist_ua, nh * ns * 2 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_xm) ok = ok && hipMemcpyAsync(hist_xm, Z.hist_xm, nh * ns * 5 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_car_s) ok = ok && hipMemcpyAsync(hist_car_s, S.hist_obs_s, nh * ns * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_tl) ok = ok && hipMemcpyAsync(hist_tl, S.hist_tl, nh * ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_status) ok = ok && hipMemcpyAsync(hist_status, S.hist_status, nh * ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_nobs) ok = ok && hipMemcpyAsync(hist_nobs, T.hist_nobs, nh * ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_slab) ok = ok && hipMemcpyAsync(hist_slab, V.hist_slab, nh * ns * nak * 2 * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (hist_lead) ok = ok && hipMemcpyAsync(hist_lead, V.hist_lead, nh * ns * nk * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && hipStreamSynchronize(st) == hipSuccess;
            if (!ok) {
                rc = fail(MPC_E_DEVICE, "noisy-loop copy-back");
            } else {
                for (size_t b = 0; b < nb; ++b) {             // column-major on the device -> one row per ego
                    for (int k = 0; k < MPC_CL_NQ; ++k) quant[b * MPC_CL_NQ + k] = hq[(size_t)k * nb + b];
                    if (extra)
                        for (int k = 0; k < MPC_NZ_NX; ++k) extra[b * MPC_NZ_NX + k] = hx[(size_t)k * nb + b];
                }
                mpcqp_cpu::sweep_max_step_ms(B, hn.data(), ms, quant);
                if (n_steps) std::memcpy(n_steps, hn.data(), nb * 4);
                if (step_ms)
                    for (size_t i = 0; i < ns; ++i) step_ms[i] = i < ms.size() ? ms[i] : (double)NAN;
            }
        }
    } catch (const std::bad_alloc&) {
        rc = fail(MPC_E_ALLOC, "noisy-loop host buffers");
    }
    cleanup();
    return rc;
}

// the draws of mpc_closed_loop_noisy on their own (include/mpcqp.h), on the context's backend
extern "C" int mpc_noise_draw(mpc_ctx* c, unsigned long long seed, int n, const long long* ego, const int* step,
                              const int* channel, unsigned* words, double* z) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!ego || !step || !channel))) return fail(MPC_E_ARG, "bad noise-draw arguments");
    for (int i = 0; i < n; ++i) {
        if (ego[i] < 0) return fail(MPC_E_ARG, "noise draw: ego index < 0");
        if (channel[i] < 0 || channel[i] >= MPC_NZ_CHANNELS) return fail(MPC_E_ARG, "noise draw: channel outside 0 .. 47");
    }
    if (n == 0 || (!words && !z)) return MPC_SUCCESS;
    if (c->cpu) {
        mpcqp_cpu::noise_draw(seed, n, ego, step, channel, words, z);
        return MPC_SUCCESS;
    }
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    const size_t nn = (size_t)n;
    std::vector<void*> bufs;
    auto dalloc = [&](size_t bytes) -> void* {
        void* ptr = nullptr;
        if (hipMalloc(&ptr, bytes) != hipSuccess) return nullptr;
        bufs.push_back(ptr);
        return ptr;
    };
    auto release = [&]() { for (void* q : bufs) hipFree(q); };
    long long* d_ego = (long long*)dalloc(nn * 8);
    int* d_step = (int*)dalloc(nn * 4);
    int* d_ch = (int*)dalloc(nn * 4);
    unsigned* d_w = words ? (unsigned*)dalloc(nn * 16) : nullptr;
    double* d_z = z ? (double*)dalloc(nn * 8) : nullptr;
    if (!d_ego || !d_step || !d_ch || (words && !d_w) || (z && !d_z)) {
        release();
        return fail(MPC_E_ALLOC, "hipMalloc noise-draw buffers");
    }
    hipStream_t st = c->stream;
    bool ok = hipMemcpyAsync(d_ego, ego, nn * 8, hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(d_step, step, nn * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(d_ch, channel, nn * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(nz_draw_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, (unsigned)(seed & 0xffffffffull),
                           (unsigned)(seed >> 32), d_ego, d_step, d_ch, d_w, d_z);
        ok = hipGetLastError() == hipSuccess;
    }
    if (words) ok = ok && hipMemcpyAsync(words, d_w, nn * 16, hipMemcpyDeviceToHost, st) == hipSuccess;
    if (z) ok = ok && hipMemcpyAsync(z, d_z, nn * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = hipStreamSynchronize(st) == hipSuccess && ok;
    release();
    return ok ? MPC_SUCCESS : fail(MPC_E_DEVICE, "noise draw");
}

extern "C" int mpc_global_pose(mpc_ctx* c, int n, const double* s, const double* d, double* out) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!s || !d || !out))) return fail(MPC_E_ARG, "bad global-pose arguments");
    if (n == 0) return MPC_SUCCESS;
    if (c->cpu) {
        c->cpu->pose(n, s, d, out);
        return MPC_SUCCESS;
    }
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    double* buf = nullptr;
    HIPCHK(hipMalloc(&buf, sizeof(double) * 5 * (size_t)n), MPC_E_ALLOC);
    hipStream_t st = c->stream;
    int rc = MPC_SUCCESS;
    if (hipMemcpyAsync(buf, s, sizeof(double) * n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(buf + n, d, sizeof(double) * n, hipMemcpyHostToDevice, st) != hipSuccess) {
        rc = fail(MPC_E_DEVICE, "hipMemcpy global pose inputs");
    } else {
        hipLaunchKernelGGL(mpc_pose_kernel, dim3((n + 255) / 256), dim3(256), 0, st, c->tab, n, buf, buf + n, buf + 2 * n);
        if (hipGetLastError() != hipSuccess) rc = fail(MPC_E_LAUNCH, "global pose kernel");
        else if (hipMemcpyAsync(out, buf + 2 * n, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
                 hipStreamSynchronize(st) != hipSuccess)
            rc = fail(MPC_E_DEVICE, "hipMemcpy global pose");
    }
    hipStreamSynchronize(st);
    hipFree(buf);
    return rc;
}

extern "C" int mpc_read_trajectory_json(const char* path, double* X, int maxT, double* U, int maxTu, int* T,
                                        int* Tu) {
    if (!path || !T || !Tu) return fail(MPC_E_ARG, "path, T and Tu are required");
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(MPC_E_ARG, std::string("File not found : ") + path + ".");   // trajectory_loader.py:18
    std::string text;
    char chunk[65536];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) text.append(chunk, got);
    std::fclose(f);
    // host_table.h: json.load semantics (last duplicate key wins, bounded nesting, no trailing data)
    std::vector<double> xs, us;
    int tx = 0, tu = 0;
    std::string err;
    if (!mpcqp_host::read_trajectory_json_text(text, xs, tx, us, tu, err)) return fail(MPC_E_ARG, err);
    *T = tx;
    *Tu = tu;
    if (X) {
        if (maxT < tx) return fail(MPC_E_ARG, "X buffer too small");
        std::memcpy(X, xs.data(), sizeof(double) * 5 * (size_t)tx);
    }
    if (U) {
        if (maxTu < tu) return fail(MPC_E_ARG, "U buffer too small");
        std::memcpy(U, us.data(), sizeof(double) * 2 * (size_t)tu);
    }
    return MPC_SUCCESS;
}

extern "C" int mpc_create_from_json(const char* path, const mpc_params* p, int device, mpc_ctx** out) {
    int T = 0, Tu = 0;
    int rc = mpc_read_trajectory_json(path, nullptr, 0, nullptr, 0, &T, &Tu);
    if (rc) return rc;
    std::vector<double> X((size_t)5 * T), U((size_t)2 * Tu);
    rc = mpc_read_trajectory_json(path, X.data(), T, U.data(), Tu, &T, &Tu);
    if (rc) return rc;
    return mpc_create(X.data(), T, U.data(), Tu, p, device, out);
}

extern "C" int mpc_lookup(mpc_ctx* c, int n, const double* s, double* out_state, double* out_control) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && !s)) return fail(MPC_E_ARG, "bad lookup arguments");
    if (n == 0) return MPC_SUCCESS;
    if (c->cpu) {
        c->cpu->lookup(n, s, out_state, out_control);
        return MPC_SUCCESS;
    }
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    if ((size_t)n > c->cap_lookup) {
        if (grow(&c->ls, n) || grow(&c->lst, (size_t)n * 5) || grow(&c->lct, (size_t)n * 2))
            return fail(MPC_E_ALLOC, "hipMalloc lookup");
        c->cap_lookup = n;
    }
    hipStream_t st = c->stream;
    HIPCHK(hipMemcpyAsync(c->ls, s, sizeof(double) * n, hipMemcpyHostToDevice, st), MPC_E_DEVICE);
    hipLaunchKernelGGL(mpc_lookup_kernel, dim3((n + 255) / 256), dim3(256), 0, st, c->tab, n, c->ls, c->lst, c->lct);
    HIPCHK(hipGetLastError(), MPC_E_LAUNCH);
    if (out_state)
        HIPCHK(hipMemcpyAsync(out_state, c->lst, sizeof(double) * 5 * n, hipMemcpyDeviceToHost, st), MPC_E_DEVICE);
    if (out_control)
        HIPCHK(hipMemcpyAsync(out_control, c->lct, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, st), MPC_E_DEVICE);
    HIPCHK(hipStreamSynchronize(st), MPC_E_DEVICE);
    return MPC_SUCCESS;
}

// multi-GPU: the ego-shard communicator (RCCL gather behind the C ABI)
#include "comm.h"
