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
//   tracker_model.h        table, parameters, lookups, constants, row model, evaluator and gradient steps (shared with the host)
//   device_common.h        LDS layout, cross-lane helpers, rollout, fences
//   riccati_lanes.h        the lane-distributed Riccati recursions (inline-asm DPP chains)
//   solve_kernel.h         mpc_solve_kernel and mpc_lookup_kernel
//   closed_loop_kernels.h  closed-loop FSM / plant / compaction kernels, pose kernel
//   sweep_kernels.h        the scenario sweep's FSM / plant kernels (a scenario per ego, check quantities)
//   traffic_kernels.h      the traffic scripts' FSM / gather kernels (up to 16 actors per ego)
//   convoy_kernels.h       the convoys' leader-ranking kernel (a workgroup per world)
//   noise_kernels.h        the disturbance sweeps' Philox source, measure / plant / draw kernels
//   trace_kernels.h        the plan traces' gap and history kernels (the solver's U / Xpred of every step)
//   warm_kernels.h         the warm starts' carry and keep kernels (the previous plan as the next ubar)
//   evaluator_common.h     the phase the four batched evaluators below share: instance, rollout, linearisation
//   evaluate_kernel.h      the batched evaluator of the reference's cost and constraint rows
//   gradient_kernel.h      the batched gradients of that cost and of those rows (reverse sweeps)
//   hessvec_kernel.h       the batched Hessian-vector products and row tangents (a lane per direction)
//   multiplier_kernel.h    the batched multiplier estimates of those rows (least squares over the active rows)
// Below them: the host side (error plumbing, mpc_ctx, mpc_create, launch_solve, the batch, closed-loop, pose
// and lookup entry points; the host entries stage their arrays through staging.h, the driver the closed-loop
// entries share is closed_loop_host.h) and, last, the comm layer (comm.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <initializer_list>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mpcqp.h"
#include "staging.h"
#include "host_table.h"
#include "cpu_backend.h"
#include "solve_kernel.h"
#include "closed_loop_kernels.h"
#include "sweep_kernels.h"
#include "traffic_kernels.h"
#include "convoy_kernels.h"
#include "noise_kernels.h"
#include "trace_kernels.h"
#include "warm_kernels.h"
#include "evaluate_kernel.h"
#include "gradient_kernel.h"
#include "multiplier_kernel.h"
#include "hessvec_kernel.h"

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
    staging::Arena arena;       // what the host entries stage their arrays through (staging.h)
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

// the kernels' parameters: the model's (tracker_model.h) and the environment's switches
static KParams kparams(const mpc_params* p) {
    KParams k = model_params(*p);
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
    c->tab = ht.view(c->table_buf);
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
    // mpc_hessvec_kernel's dynamic LDS goes beyond 64 KB: declare the most a launch may ask for (here, so that no
    // hessvec call does anything but launch).  A runtime that needs no such declaration may refuse it: ignored
    {
        const int n64 = (int)sizeof(double) * hv_lds_doubles(MPC_HV_N64_MAX, 64);
        const int n32 = (int)sizeof(double) * hv_lds_doubles(MPC_MAX_N, 32);
        (void)hipFuncSetAttribute((const void*)mpc_hessvec_kernel<64, true>, hipFuncAttributeMaxDynamicSharedMemorySize, n64);
        (void)hipFuncSetAttribute((const void*)mpc_hessvec_kernel<64, false>, hipFuncAttributeMaxDynamicSharedMemorySize, n64);
        (void)hipFuncSetAttribute((const void*)mpc_hessvec_kernel<32, true>, hipFuncAttributeMaxDynamicSharedMemorySize, n32);
        (void)hipFuncSetAttribute((const void*)mpc_hessvec_kernel<32, false>, hipFuncAttributeMaxDynamicSharedMemorySize, n32);
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

extern "C" void mpc_destroy(mpc_ctx* c) {
    if (!c) return;
    if (c->cpu) {
        delete c->cpu;
        std::free(c);
        return;
    }
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    c->arena.release();
    if (c->wl) hipEventDestroy(c->wl_done);
    hipFree(c->wl);
    hipFree(c->stc);
    hipFree(c->table_buf);
    hipStreamDestroy(c->stream);
    std::free(c);
}

// The runtime-horizon launches' choice of kernel: f(GL, obs) with the lane group (lane_group) and whether obstacle
// rows exist as std::integral_constants, so f names the instantiation <decltype(gl)::value, decltype(ob)::value>
template <typename F>
static void for_gl_obs(int GL, bool obs, F&& f) {
    auto with_gl = [&](auto gl) { obs ? f(gl, std::true_type{}) : f(gl, std::false_type{}); };
    if (GL == 16) with_gl(std::integral_constant<int, 16>{});
    else if (GL == 32) with_gl(std::integral_constant<int, 32>{});
    else with_gl(std::integral_constant<int, 64>{});
}

// one lane group per instance, WAVE / GL instances per wavefront
static dim3 group_grid(int B, int GL) { return dim3((B + WAVE / GL - 1) / (WAVE / GL)); }

// launch of the solver kernel for an already validated parameter set
#define MPC_STAGE_CACHE_CAP ((size_t)1 << 27)
static int launch_solve(mpc_ctx* c, const KParams& kp, int B, const double* x0, const double* obs, const int* n_obs,
                        const double* ubar, double* u0, double* U, double* Xpred, int* status, int* iters,
                        hipStream_t st) {
    // G = 64 / GL instances per wavefront: the smallest lane group holding the N + 1 stages
    const int* nob = obs ? n_obs : nullptr;
    const int GL = lane_group(kp.N);
    const int G = WAVE / GL;
    // horizon of the specialised kernel that serves N (0: the runtime-horizon kernels)
    const int ntv = kp.N == 20 || kp.N == 30 || kp.N == 40 ? kp.N : 0;
    const size_t lds_wave = sizeof(double) * (size_t)lds_doubles(kp.N, acl_on(GL, ntv)) * G;
    if (lds_wave > 160 * 1024) return fail(MPC_E_ARG, "horizon too long for LDS");
    const size_t lds_lite = sizeof(double) * (size_t)lds_doubles(kp.N, false, true) * G;   // MODE_XO
    const dim3 grid = group_grid(B, GL);
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
        else for_gl_obs(GL, with_obs, [&](auto gl, auto ob) { MPC_LAUNCH(decltype(gl)::value, decltype(ob)::value, MODEV, 0); }); \
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

// ------------------------------------------------------------------------------------------
// the batch entries.  Each host / device pair shares one *_args: the checks that hold for both, B == 0 included (it
// passes, and the entry returns success on it).  What only the device side can be asked is device_args: n_obs without
// obs (a host entry stages n_obs only together with obs) and the alignment of raw addresses (staging.h aligns).
// ------------------------------------------------------------------------------------------
// the checks of all three pairs in the order they fire; u_missing: the refusal of a NULL U that the entry needs
static int batch_args(mpc_ctx* c, int B, const double* x0, const double* obs, const char* u_missing = nullptr,
                      bool jtl_without_lam = false) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0) return fail(MPC_E_ARG, "B < 0");
    if (B == 0) return MPC_SUCCESS;
    if (!x0) return fail(MPC_E_ARG, "x0 is NULL");
    if (u_missing) return fail(MPC_E_ARG, u_missing);
    if (obs && c->p.max_obs == 0)
        return fail(MPC_E_ARG, "obs given but params.max_obs == 0 (the obstacles would be ignored)");
    if (jtl_without_lam) return fail(MPC_E_ARG, "jtl asked for but lam is NULL (J' lam needs the row weights)");
    return check_params(&c->p);
}

static int solve_args(mpc_ctx* c, int B, const double* x0, const double* obs) { return batch_args(c, B, x0, obs); }
static int evaluate_args(mpc_ctx* c, int B, const double* x0, const double* obs, const double* U) {
    return batch_args(c, B, x0, obs, U ? nullptr : "U is NULL (the evaluator needs the control sequence to evaluate)");
}

static int gradient_args(mpc_ctx* c, int B, const double* x0, const double* obs, const double* U, const double* lam,
                         const double* jtl) {
    return batch_args(c, B, x0, obs, U ? nullptr : "U is NULL (the gradient needs the control sequence to differentiate at)",
                      jtl && !lam);
}

static int multipliers_args(mpc_ctx* c, int B, const double* x0, const double* obs, const double* U, double active_tol,
                            double bound_tol, double rank_tol) {
    int rc = batch_args(c, B, x0, obs, U ? nullptr : "U is NULL (the multiplier estimate needs the control sequence to estimate at)");
    if (rc || B == 0) return rc;
    if (active_tol != active_tol) return fail(MPC_E_ARG, "active_tol is NaN");
    if (!(bound_tol >= 0.0)) return fail(MPC_E_ARG, "bound_tol is negative or NaN");
    if (!(rank_tol >= 0.0)) return fail(MPC_E_ARG, "rank_tol is negative or NaN");
    return MPC_SUCCESS;
}

static int device_args(const mpc_ctx* c, const double* obs, const int* n_obs, std::initializer_list<const double*> arrays) {
    if (c->p.max_obs > 0 && n_obs && !obs) return fail(MPC_E_ARG, "n_obs given but obs is NULL");
    for (const double* a : arrays)
        if ((uintptr_t)a & 7) return fail(MPC_E_ARG, "double arrays must be 8-byte aligned");
    return MPC_SUCCESS;
}

extern "C" int mpc_solve_batch_device(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                                      const double* ubar, double* u0, double* U, double* Xpred, int* status,
                                      int* iters, void* stream) {
    int rc = solve_args(c, B, x0, obs);
    if (rc || B == 0) return rc;
    if ((rc = device_args(c, obs, n_obs, {u0, U, x0, Xpred, obs, ubar}))) return rc;
    if (c->cpu) {
        // host context: the pointers are host memory and the call is synchronous (stream ignored)
        return host_call([&] { c->cpu->solve_batch(c->p, B, x0, obs, n_obs, ubar, u0, U, Xpred, status, iters); });
    }
    KParams kp = kparams(&c->p);
    if (!obs) kp.max_obs = 0;
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    return launch_solve(c, kp, B, x0, obs, n_obs, ubar, u0, U, Xpred, status, iters, (hipStream_t)stream);
}

// a host entry's round trip: its arrays bound to the context's arena, the uploads, its device twin on the device
// arrays and the downloads, all on the context's stream, then one synchronisation
template <typename Bind, typename Call>
static int staged_call(mpc_ctx* c, const char* no_memory, Bind&& bindings, Call&& device_entry) {
    staging::Staging S(c->arena);
    if (!S.bind([&] { bindings(S); })) return fail(MPC_E_ALLOC, no_memory);
    HIPCHK(S.upload(c->stream), MPC_E_DEVICE);
    if (int rc = device_entry()) return rc;
    HIPCHK(S.fetch(c->stream), MPC_E_DEVICE);
    HIPCHK(S.sync(c->stream), MPC_E_DEVICE);
    return MPC_SUCCESS;
}

// The inputs the batch entries share, bound to a host entry's arena: x0 [B][5], obs [B][max_obs][2], n_obs [B] (it
// travels only with obs), U [B][N][2] (the solver's ubar) and lam [B][N][7 + max_obs]; a null array stays null
struct BatchInputs {
    double *x0, *obs;
    int* n_obs;
    double *U, *lam;
};
static BatchInputs stage_inputs(staging::Staging& S, const mpc_ctx* c, int B, const double* x0, const double* obs,
                                const int* n_obs, const double* U, const double* lam) {
    const size_t nb = (size_t)B, N = (size_t)c->p.N, mo = (size_t)c->p.max_obs;
    BatchInputs d;
    d.x0 = S.in(x0, nb * 5);
    d.obs = S.in(obs, nb * mo * 2);
    d.n_obs = obs ? S.in(n_obs, nb) : nullptr;
    d.U = S.in(U, nb * N * 2);
    d.lam = S.in(lam, nb * N * (7 + mo));
    return d;
}

extern "C" int mpc_solve_batch(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                               const double* ubar, double* u0, double* U, double* Xpred, int* status, int* iters) {
    int rc = solve_args(c, B, x0, obs);
    if (rc || B == 0) return rc;
    if (c->cpu) return host_call([&] { c->cpu->solve_batch(c->p, B, x0, obs, n_obs, ubar, u0, U, Xpred, status, iters); });
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    const size_t nb = (size_t)B, N = (size_t)c->p.N;
    BatchInputs d;
    double *d_u0, *d_U, *d_X;
    int *d_status, *d_iters;
    // the kernel writes all five outputs, asked for or not
    return staged_call(c, "hipMalloc staging", [&](staging::Staging& S) {
        d = stage_inputs(S, c, B, x0, obs, n_obs, ubar, nullptr);
        d_u0 = S.out_or_scratch(u0, nb * 2);
        d_U = S.out_or_scratch(U, nb * N * 2);
        d_X = S.out_or_scratch(Xpred, nb * (N + 1) * 5);
        d_status = S.out_or_scratch(status, nb);
        d_iters = S.out_or_scratch(iters, nb);
    }, [&] {
        return mpc_solve_batch_device(c, B, d.x0, d.obs, d.n_obs, d.U, d_u0, d_U, d_X, d_status, d_iters, (void*)c->stream);
    });
}

// ------------------------------------------------------------------------------------------
// the batched evaluators (evaluator_common.h and the four kernels over it).  A host / device pair is one *_entry
// function, which states the pair's own parts once and hands them to evaluator_entry: the pair's checks (rc), the
// double arrays whose addresses a device call must have aligned, whether any output is asked for, the call of the host
// backend, the launch, and for the host entry (staged) its arena bindings and the call of itself on the device arrays.
// The order of a device entry: the shared checks and B == 0, device_args, no output asked for, a device = -1
// context's host backend, then the kernel's parameters (obstacle rows exist only when obstacles are passed; rw, the
// width of rows / lam / JV, keeps the context's slab width without them too), the device, the launch.  A host entry
// skips device_args and the launch: it stages its arrays and calls the device entry on the context's stream.
// ------------------------------------------------------------------------------------------
template <typename Host, typename Launch, typename Bind, typename Device>
static int evaluator_entry(mpc_ctx* c, int B, int rc, bool staged, const double* obs, const int* n_obs,
                           std::initializer_list<const double*> arrays, bool wanted, const char* no_memory, Host&& host,
                           Launch&& launch, Bind&& bindings, Device&& device_entry) {
    if (rc || B == 0) return rc;
    if (!staged && (rc = device_args(c, obs, n_obs, arrays))) return rc;
    if (!wanted) return MPC_SUCCESS;
    if (c->cpu) return host_call(host);
    if (staged) {
        HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
        return staged_call(c, no_memory, bindings, device_entry);
    }
    KParams kp = kparams(&c->p);
    const int rw = 7 + c->p.max_obs;
    if (!obs) kp.max_obs = 0;
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    launch(kp, rw, obs ? n_obs : nullptr);
    HIPCHK(hipGetLastError(), MPC_E_LAUNCH);
    return MPC_SUCCESS;
}

// batched evaluator (evaluate_kernel.h)
static int evaluate_entry(mpc_ctx* c, bool staged, int B, const double* x0, const double* obs, const int* n_obs,
                          const double* U, double* Xpred, double* summary, double* terms, double* rows, void* stream) {
    BatchInputs d;
    double *d_X, *d_sum, *d_terms, *d_rows;
    return evaluator_entry(
        c, B, evaluate_args(c, B, x0, obs, U), staged, obs, n_obs, {x0, obs, U, Xpred, summary, terms, rows},
        Xpred || summary || terms || rows, "hipMalloc evaluator staging",
        [&] { c->cpu->evaluate_batch(c->p, B, x0, obs, n_obs, U, Xpred, summary, terms, rows); },
        [&](const KParams& kp, int rw, const int* nob) {
            const int GL = lane_group(kp.N);
            for_gl_obs(GL, obs != nullptr, [&](auto gl, auto ob) {
                hipLaunchKernelGGL((mpc_evaluate_kernel<decltype(gl)::value, decltype(ob)::value>), group_grid(B, GL),
                                   dim3(WAVE), 0, (hipStream_t)stream, c->tab, kp, B, rw, x0, obs, nob, U, Xpred, summary,
                                   terms, rows);
            });
        },
        [&](staging::Staging& S) {
            const size_t nb = (size_t)B, N = (size_t)c->p.N, mo = (size_t)c->p.max_obs;
            d = stage_inputs(S, c, B, x0, obs, n_obs, U, nullptr);
            d_X = S.out(Xpred, nb * (N + 1) * 5);
            d_sum = S.out(summary, nb * MPC_EV_NQ);
            d_terms = S.out(terms, nb * 5);
            d_rows = S.out(rows, nb * N * (7 + mo));
        },
        [&] { return evaluate_entry(c, false, B, d.x0, d.obs, d.n_obs, d.U, d_X, d_sum, d_terms, d_rows, (void*)c->stream); });
}

extern "C" int mpc_evaluate_batch_device(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                                         const double* U, double* Xpred, double* summary, double* terms,
                                         double* rows, void* stream) {
    return evaluate_entry(c, false, B, x0, obs, n_obs, U, Xpred, summary, terms, rows, stream);
}

extern "C" int mpc_evaluate_batch(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                                  const double* U, double* Xpred, double* summary, double* terms, double* rows) {
    return evaluate_entry(c, true, B, x0, obs, n_obs, U, Xpred, summary, terms, rows, nullptr);
}

// batched gradients (gradient_kernel.h)
static int gradient_entry(mpc_ctx* c, bool staged, int B, const double* x0, const double* obs, const int* n_obs,
                          const double* U, const double* lam, double* grad, double* jtl, double* gx0, double* costate,
                          double* summary, void* stream) {
    BatchInputs d;
    double *d_grad, *d_jtl, *d_gx0, *d_cos, *d_sum;
    return evaluator_entry(
        c, B, gradient_args(c, B, x0, obs, U, lam, jtl), staged, obs, n_obs,
        {x0, obs, U, lam, grad, jtl, gx0, costate, summary}, grad || jtl || gx0 || costate || summary,
        "hipMalloc gradient staging",
        [&] { c->cpu->gradient_batch(c->p, B, x0, obs, n_obs, U, lam, grad, jtl, gx0, costate, summary); },
        [&](const KParams& kp, int rw, const int* nob) {
            const int GL = lane_group(kp.N);
            for_gl_obs(GL, obs != nullptr, [&](auto gl, auto ob) {
                hipLaunchKernelGGL((mpc_gradient_kernel<decltype(gl)::value, decltype(ob)::value>), group_grid(B, GL),
                                   dim3(WAVE), 0, (hipStream_t)stream, c->tab, kp, B, rw, x0, obs, nob, U, lam, grad, jtl,
                                   gx0, costate, summary);
            });
        },
        [&](staging::Staging& S) {
            const size_t nb = (size_t)B, N = (size_t)c->p.N;
            d = stage_inputs(S, c, B, x0, obs, n_obs, U, lam);
            d_grad = S.out(grad, nb * N * 2);
            d_jtl = S.out(jtl, nb * N * 2);
            d_gx0 = S.out(gx0, nb * 5);
            d_cos = S.out(costate, nb * N * 5);
            d_sum = S.out(summary, nb * MPC_GR_NQ);
        },
        [&] {
            return gradient_entry(c, false, B, d.x0, d.obs, d.n_obs, d.U, d.lam, d_grad, d_jtl, d_gx0, d_cos, d_sum,
                                  (void*)c->stream);
        });
}

extern "C" int mpc_gradient_batch_device(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                                         const double* U, const double* lam, double* grad, double* jtl, double* gx0,
                                         double* costate, double* summary, void* stream) {
    return gradient_entry(c, false, B, x0, obs, n_obs, U, lam, grad, jtl, gx0, costate, summary, stream);
}

extern "C" int mpc_gradient_batch(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                                  const double* U, const double* lam, double* grad, double* jtl, double* gx0,
                                  double* costate, double* summary) {
    return gradient_entry(c, true, B, x0, obs, n_obs, U, lam, grad, jtl, gx0, costate, summary, nullptr);
}

// batched multiplier estimates (multiplier_kernel.h)
static int multipliers_entry(mpc_ctx* c, bool staged, int B, const double* x0, const double* obs, const int* n_obs,
                             const double* U, double active_tol, double bound_tol, double rank_tol, double* lam,
                             int* active, double* summary, void* stream) {
    BatchInputs d;
    double *d_lam, *d_sum;
    int* d_act;
    return evaluator_entry(
        c, B, multipliers_args(c, B, x0, obs, U, active_tol, bound_tol, rank_tol), staged, obs, n_obs,
        {x0, obs, U, lam, summary}, lam || active || summary, "hipMalloc multiplier staging",
        [&] { c->cpu->multipliers_batch(c->p, B, x0, obs, n_obs, U, active_tol, bound_tol, rank_tol, lam, active, summary); },
        [&](const KParams& kp, int rw, const int* nob) {
            // one wavefront per instance; the lane-group class of N sizes the kernel's LDS
            for_gl_obs(lane_group(kp.N), obs != nullptr, [&](auto gl, auto ob) {
                hipLaunchKernelGGL((mpc_multipliers_kernel<decltype(gl)::value, decltype(ob)::value>), dim3(B), dim3(WAVE),
                                   0, (hipStream_t)stream, c->tab, kp, B, rw, x0, obs, nob, U, active_tol, bound_tol,
                                   rank_tol, lam, active, summary);
            });
        },
        [&](staging::Staging& S) {
            const size_t nb = (size_t)B, N = (size_t)c->p.N, mo = (size_t)c->p.max_obs;
            d = stage_inputs(S, c, B, x0, obs, n_obs, U, nullptr);
            d_lam = S.out(lam, nb * N * (7 + mo));
            d_act = S.out(active, nb * MPC_MAX_ACTIVE);
            d_sum = S.out(summary, nb * MPC_MU_NQ);
        },
        [&] {
            return multipliers_entry(c, false, B, d.x0, d.obs, d.n_obs, d.U, active_tol, bound_tol, rank_tol, d_lam, d_act,
                                     d_sum, (void*)c->stream);
        });
}

extern "C" int mpc_multipliers_batch_device(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                                            const double* U, double active_tol, double bound_tol, double rank_tol,
                                            double* lam, int* active, double* summary, void* stream) {
    return multipliers_entry(c, false, B, x0, obs, n_obs, U, active_tol, bound_tol, rank_tol, lam, active, summary, stream);
}

extern "C" int mpc_multipliers_batch(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                                     const double* U, double active_tol, double bound_tol, double rank_tol, double* lam,
                                     int* active, double* summary) {
    return multipliers_entry(c, true, B, x0, obs, n_obs, U, active_tol, bound_tol, rank_tol, lam, active, summary, nullptr);
}

// batched Hessian-vector products and row tangents (hessvec_kernel.h)
static int hessvec_args(mpc_ctx* c, int B, const double* x0, const double* obs, const double* U, int M, const double* V,
                        int mode) {
    int rc = batch_args(c, B, x0, obs, U ? nullptr : "U is NULL (the Hessian needs the control sequence to differentiate at)");
    if (rc || B == 0) return rc;
    if (M < 1 || M > MPC_HV_MAX_DIRS) return fail(MPC_E_ARG, "M must be in 1..MPC_HV_MAX_DIRS");
    if (!V && M > 2 * c->p.N) return fail(MPC_E_ARG, "V is NULL (unit directions) but M > 2 N");
    if (mode != MPC_HV_EXACT && mode != MPC_HV_GAUSS_NEWTON)
        return fail(MPC_E_ARG, "mode must be MPC_HV_EXACT or MPC_HV_GAUSS_NEWTON");
    return MPC_SUCCESS;
}

static int hessvec_entry(mpc_ctx* c, bool staged, int B, const double* x0, const double* obs, const int* n_obs,
                         const double* U, const double* lam, int M, const double* V, int mode, double* HV, double* JV,
                         double* curv, double* summary, void* stream) {
    BatchInputs d;
    double *d_V, *d_HV, *d_JV, *d_curv, *d_sum;
    return evaluator_entry(
        c, B, hessvec_args(c, B, x0, obs, U, M, V, mode), staged, obs, n_obs, {x0, obs, U, lam, V, HV, JV, curv, summary},
        HV || JV || curv || summary, "hipMalloc hessvec staging",
        [&] { c->cpu->hessvec_batch(c->p, B, x0, obs, n_obs, U, lam, M, V, mode, HV, JV, curv, summary); },
        [&](const KParams& kp, int rw, const int* nob) {
            // one wavefront per instance; the pass width and the actual N size its LDS
            const int W = hv_pass_width(kp.N);
            const size_t lds = sizeof(double) * (size_t)hv_lds_doubles(kp.N, W);
            for_gl_obs(W, obs != nullptr, [&](auto w, auto ob) {
                constexpr int WV = decltype(w)::value == 32 ? 32 : 64;
                hipLaunchKernelGGL((mpc_hessvec_kernel<WV, decltype(ob)::value>), dim3(B), dim3(WAVE), lds,
                                   (hipStream_t)stream, c->tab, kp, B, rw, x0, obs, nob, U, lam, M, V, mode, HV, JV, curv,
                                   summary);
            });
        },
        [&](staging::Staging& S) {
            const size_t nb = (size_t)B, N = (size_t)c->p.N, mo = (size_t)c->p.max_obs, nm = nb * (size_t)M;
            d = stage_inputs(S, c, B, x0, obs, n_obs, U, lam);
            d_V = S.in(V, nm * N * 2);
            d_HV = S.out(HV, nm * N * 2);
            d_JV = S.out(JV, nm * N * (7 + mo));
            d_curv = S.out(curv, nm * 2);
            d_sum = S.out(summary, nb * MPC_HV_NQ);
        },
        [&] {
            return hessvec_entry(c, false, B, d.x0, d.obs, d.n_obs, d.U, d.lam, M, d_V, mode, d_HV, d_JV, d_curv, d_sum,
                                 (void*)c->stream);
        });
}

extern "C" int mpc_hessvec_batch_device(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                                        const double* U, const double* lam, int M, const double* V, int mode, double* HV,
                                        double* JV, double* curv, double* summary, void* stream) {
    return hessvec_entry(c, false, B, x0, obs, n_obs, U, lam, M, V, mode, HV, JV, curv, summary, stream);
}

extern "C" int mpc_hessvec_batch(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                                 const double* U, const double* lam, int M, const double* V, int mode, double* HV,
                                 double* JV, double* curv, double* summary) {
    return hessvec_entry(c, true, B, x0, obs, n_obs, U, lam, M, V, mode, HV, JV, curv, summary, nullptr);
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

// ------------------------------------------------------------------------------------------
// the closed-loop entries: each checks its arguments, hands a device = -1 context to the host backend, and
// otherwise configures the shared driver (closed_loop_host.h) with its buffers, outputs and kernels
// ------------------------------------------------------------------------------------------
#include "closed_loop_host.h"

// a host-backend closed loop behind an entry: its return code, unless an exception was turned into one
template <typename F>
static int host_loop(F&& f) {
    int hrc = MPC_SUCCESS;
    const int erc = host_call([&] { hrc = f(); });
    return erc != MPC_SUCCESS ? erc : hrc;
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
    if (c->cpu)
        return host_loop([&] {
            return c->cpu->closed_loop(c->p, B, x_init, F, with_fsm, max_steps, s_stop, hist_x, hist_u, hist_obs_s,
                                       hist_tl, hist_status, n_steps, step_ms);
        });
    KParams kp = kparams(&c->p);
    kp.max_obs = with_fsm ? 2 : 0;          // the FSM yields at most the car and the light
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    ClDriver D(c, "closed-loop", B, max_steps);
    const size_t nb = D.nb, ns = D.ns;
    const hipStream_t st = D.st;
    D.cl_state(x_init, 2, true);
    const ClState& C = D.C;
    int* d_ns = D.out(n_steps, nb, false);  // histories of every ego: [B] rows
    double* d_hx = D.out(hist_x, nb * (ns + 1) * 5);
    double* d_hu = D.out(hist_u, nb * ns * 2);
    double* d_ho = D.out(hist_obs_s, nb * ns);
    int* d_ht = D.out(hist_tl, nb * ns);
    int* d_hs = D.out(hist_status, nb * ns);
    rc = D.begin();
    if (rc) return rc;
    hipLaunchKernelGGL(cl_init_kernel, D.tg, D.tb, 0, st, B, F, C, D.xinit, s_stop, d_hx, d_ns, max_steps);
    rc = D.run(kp, with_fsm, step_ms != nullptr,
               [&](int step, int nl, dim3 lg) {
                   // runs without scenarios too: records the RED light / no-car histories like the reference
                   hipLaunchKernelGGL(cl_fsm_kernel, D.tg, D.tb, 0, st, B, F, kp.dt, C, d_ho, d_ht, step, max_steps);
                   hipLaunchKernelGGL(cl_gather_kernel, lg, D.tb, 0, st, nl, C);
               },
               [&](int step, int nl, dim3 lg) {
                   hipLaunchKernelGGL(cl_plant_kernel, lg, D.tb, 0, st, c->tab, nl, kp.dt, C, s_stop, d_hx, d_hu, d_hs,
                                      d_ns, step, max_steps);
               });
    if (rc == MPC_SUCCESS && !(D.fetch() && hipStreamSynchronize(st) == hipSuccess))
        rc = fail(MPC_E_DEVICE, "closed-loop copy-back");
    if (step_ms) D.fill_step_ms(step_ms);
    return rc;
}

// mpc_closed_loop with a scenario per ego, the check quantities accumulated on the device and histories for
// the named egos only (include/mpcqp.h)
extern "C" int mpc_closed_loop_sweep(mpc_ctx* c, int B, const double* x_init, const mpc_fsm* fsm, int n_fsm,
                                     int max_steps, double s_stop, double* quant, int n_hist, const int* hist_egos,
                                     double* hist_x, double* hist_u, double* hist_obs_s, int* hist_tl,
                                     int* hist_status, int* n_steps, double* step_ms) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0 || max_steps < 1) return fail(MPC_E_ARG, "B < 0 or max_steps < 1");
    if (fsm ? !(n_fsm == 1 || n_fsm == B) : n_fsm != 0)
        return fail(MPC_E_ARG, "n_fsm must be B (a scenario per ego), 1 (shared) or 0 with fsm NULL");
    int rc = cl_check_outputs(quant, n_hist, hist_x || hist_u || hist_obs_s || hist_tl || hist_status);
    if (rc) return rc;
    std::vector<int> slot;
    rc = cl_slot_map(B, n_hist, hist_egos, slot);
    if (rc) return rc;
    if (B == 0) return MPC_SUCCESS;
    if (!x_init) return fail(MPC_E_ARG, "x_init is required");
    rc = check_params(&c->p);
    if (rc) return rc;
    mpc_fsm F;
    mpc_default_fsm(&F);                             // no scenario: both switches off
    if (fsm && n_fsm == 1) F = fsm[0];
    const bool per_ego = fsm && n_fsm != 1;          // n_fsm == B > 1
    bool with_fsm = F.dynamic_obstacle || F.traffic_light;
    if (per_ego)
        for (int b = 0; b < B && !with_fsm; ++b) with_fsm = fsm[b].dynamic_obstacle || fsm[b].traffic_light;
    if (c->cpu)
        return host_loop([&] {
            return c->cpu->closed_loop_sweep(c->p, B, x_init, per_ego ? fsm : &F, per_ego ? B : 1, with_fsm, max_steps,
                                             s_stop, quant, n_hist, slot.data(), hist_x, hist_u, hist_obs_s, hist_tl,
                                             hist_status, n_steps, step_ms);
        });
    KParams kp = kparams(&c->p);
    kp.max_obs = with_fsm ? 2 : 0;          // the FSM yields at most the car and the light
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    ClDriver D(c, "sweep", B, max_steps);
    const hipStream_t st = D.st;
    D.cl_state(x_init, 2, true);
    const ClState& C = D.C;
    const SwState S = D.sw_state(slot.data(), n_hist, hist_x, hist_u, hist_obs_s, hist_tl, hist_status);
    const mpc_fsm* d_fsm = per_ego ? D.in(fsm, D.nb, D.nb) : nullptr;     // the scenarios [B] when they differ
    rc = D.begin();
    if (rc) return rc;
    if (per_ego) hipLaunchKernelGGL(sw_init_kernel<true>, D.tg, D.tb, 0, st, B, F, d_fsm, C, S, D.xinit, s_stop, max_steps);
    else hipLaunchKernelGGL(sw_init_kernel<false>, D.tg, D.tb, 0, st, B, F, d_fsm, C, S, D.xinit, s_stop, max_steps);
    rc = D.run(kp, with_fsm, true,
               [&](int step, int nl, dim3 lg) {
                   if (per_ego) hipLaunchKernelGGL(sw_fsm_kernel<true>, D.tg, D.tb, 0, st, B, F, d_fsm, kp.dt, C, S, step, max_steps);
                   else hipLaunchKernelGGL(sw_fsm_kernel<false>, D.tg, D.tb, 0, st, B, F, d_fsm, kp.dt, C, S, step, max_steps);
                   hipLaunchKernelGGL(cl_gather_kernel, lg, D.tb, 0, st, nl, C);
               },
               [&](int step, int nl, dim3 lg) {
                   hipLaunchKernelGGL(sw_plant_kernel, lg, D.tb, 0, st, c->tab, B, nl, kp.dt, C, S, s_stop, step, max_steps);
               });
    return rc ? rc : D.finish(S, nullptr, 0, quant, nullptr, n_steps, step_ms);
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

extern "C" void mpc_default_noise(mpc_noise* n) { std::memset(n, 0, sizeof(*n)); }

extern "C" void mpc_default_warm(mpc_warm* w) {
    w->mode = MPC_WARM_REFERENCE;
    w->tail = MPC_WTAIL_REFERENCE;
    w->reset = 0;
}

// The five scripted entries check their arguments and fill one ScriptedLoop (scripted_loop.h) by name:
// mpc_closed_loop_traffic (no worlds), mpc_closed_loop_convoy (worlds), mpc_closed_loop_noisy (noisy worlds),
// mpc_closed_loop_traced (with the trace outputs) and mpc_closed_loop_warm (with `warm` set when the solver is to be
// handed a ubar).  scripted_loop() derives the history slots once and passes the request on as it is: to
// Backend::closed_loop_scripted on a host context, to the kernels below otherwise.
//
// The device loop of the scripted entries around tr_fsm_kernel and an (A + K)-wide slab.  With worlds, cv_lead_kernel
// ranks the leaders between the FSM and the gather and writes the slab histories (tr_fsm_kernel's rows are A
// wide); without worlds no cv_* kernel is launched.  Noisy: nz_measure_kernel for tr_gather_kernel and
// nz_plant_kernel for sw_plant_kernel, on the field-major sigma table [14][B] for per-ego noise; the other kernels
// are reused untouched and see the true states.  Traced (any trace output asked for): the solver also writes its U
// and Xpred of the listed egos, and tg_gap_kernel and tg_hist_kernel follow the plant kernel.  Warm (a.warm set):
// ws_carry_kernel fills the solver's ubar after the measure kernel, the solver is asked for its U, and
// ws_keep_kernel follows the plant kernel
static int scripted_loop(mpc_ctx* c, const ScriptedLoop& a) {
    const int B = a.B, A = a.A, K = a.K, AK = A + K, max_steps = a.max_steps;
    std::vector<int> slot;
    int rc = cl_slot_map(B, a.n_hist, a.hist_egos, slot);
    if (rc) return rc;
    if (B == 0) return MPC_SUCCESS;
    if (!a.x_init) return fail(MPC_E_ARG, "x_init is required");
    rc = check_params(&c->p);
    if (rc) return rc;
    if (c->cpu) return host_loop([&] { return c->cpu->closed_loop_scripted(c->p, a, slot.data()); });
    const bool per_ego = a.per_ego(), nz_per_ego = a.nz_per_ego(), traced = a.traced();
    KParams kp = kparams(&c->p);
    kp.max_obs = a.with_slab ? AK : 0;      // every actor and every leader adds at most one entry
    HIPCHK(hipSetDevice(c->device), MPC_E_DEVICE);
    std::vector<double> hsig;               // per-ego sigmas, field-major: the loads of a wave coalesce
    if (nz_per_ego) {
        try {
            hsig.resize((size_t)B * NZ_NSIG);
        } catch (const std::bad_alloc&) {
            return fail(MPC_E_ALLOC, "noise table");
        }
        for (size_t b = 0; b < (size_t)B; ++b)   // mpc_noise is NZ_NSIG doubles, no padding
            for (size_t f = 0; f < NZ_NSIG; ++f)
                hsig[f * (size_t)B + b] = reinterpret_cast<const double*>(a.noise + b)[f];
    }
    ClDriver D(c, a.label, B, max_steps);
    const hipStream_t st = D.st;
    const size_t nhs = (size_t)a.n_hist * D.ns;
    D.cl_state(a.x_init, (size_t)AK, false);
    const ClState& C = D.C;
    SwState S = D.sw_state(slot.data(), a.n_hist, a.hist_x, a.hist_u, a.hist_car_s, a.hist_tl, a.hist_status);
    TrState T = D.tr_state(a.actors, A, a.nsc(), per_ego, (size_t)AK, a.nx(), a.n_hist, a.hist_nobs);
    CvState V = {};
    V.W = a.W;
    V.K = K;
    V.lead_range = a.lead_range;
    if (a.worlds) {
        V.hist_slab = D.out(a.hist_slab, nhs * (size_t)AK * 2);
        V.hist_lead = D.out(a.hist_lead, nhs * (size_t)K);
    } else {
        T.hist_slab = D.out(a.hist_slab, nhs * (size_t)A * 2);
    }
    NzState Z = {};
    if (a.noisy) {
        Z.sig = nz_per_ego ? D.in(hsig.data(), hsig.size(), hsig.size()) : nullptr;
        Z.shared = nz_per_ego ? a.quiet : a.noise_of(0);
        Z.k0 = (unsigned)(a.seed & 0xffffffffull);
        Z.k1 = (unsigned)(a.seed >> 32);
        Z.g0 = (unsigned long long)a.ego_offset;
        Z.u_min0 = c->p.u_min[0];
        Z.u_min1 = c->p.u_min[1];
        Z.u_max0 = c->p.u_max[0];
        Z.u_max1 = c->p.u_max[1];
        Z.hist_ua = D.out(a.hist_ua, nhs * 2);
        Z.hist_xm = D.out(a.hist_xm, nhs * 5);
    }
    TgState G = {};
    std::vector<double> hgap;               // the gaps as the device keeps them, [n_look][MPC_TG_NQ][B]
    double *d_U = nullptr, *d_Xp = nullptr;
    if (traced) {
        const size_t nN = (size_t)c->p.N;
        try {
            hgap.resize((size_t)a.n_look * MPC_TG_NQ * D.nb);
        } catch (const std::bad_alloc&) {
            return fail(MPC_E_ALLOC, "gap table");
        }
        size_t slots = 0;
        for (int i = 0; i < a.n_look; ++i) {
            G.look[i] = a.lookahead[i];
            G.ring0[i] = (int)slots;
            slots += (size_t)a.lookahead[i];
        }
        G.N = c->p.N;
        G.n_look = a.n_look;
        G.Ua = d_U = D.mem.alloc<double>(D.nb * nN * 2);
        G.Xpa = d_Xp = D.mem.alloc<double>(D.nb * (nN + 1) * 5);
        G.ring = D.mem.alloc<double>(slots * 3 * D.nb);
        G.gq = D.out(hgap.data(), hgap.size(), false);
        G.hist_pred = D.out(a.hist_pred, nhs * (nN + 1) * 5);
        G.hist_plan = D.out(a.hist_plan, nhs * nN * 2);
    }
    WsState Ws = {};
    std::vector<double> hwq;                // the warm rows as the device keeps them, [MPC_WQ_NQ][B]
    if (a.warm) {
        const size_t nN = (size_t)c->p.N;
        try {
            hwq.resize(a.warmq ? MPC_WQ_NQ * D.nb : 0);
        } catch (const std::bad_alloc&) {
            return fail(MPC_E_ALLOC, "warm table");
        }
        if (!d_U) d_U = D.mem.alloc<double>(D.nb * nN * 2);
        Ws.warm = *a.warm;
        Ws.N = c->p.N;
        Ws.max_obs = kp.max_obs;
        Ws.dt = kp.dt;
        Ws.brake_distance = kp.brake_distance;
        Ws.brake_accel = kp.brake_accel;
        Ws.u_min0 = kp.u_min0;
        Ws.u_min1 = kp.u_min1;
        Ws.u_max0 = kp.u_max0;
        Ws.u_max1 = kp.u_max1;
        Ws.ubara = D.mem.alloc<double>(D.nb * nN * 2);
        Ws.Ua = d_U;
        Ws.plan = D.mem.alloc<double>(D.nb * nN * 2);
        Ws.status = D.mem.alloc<int>(D.nb);
        Ws.nobs = D.mem.alloc<int>(D.nb);
        Ws.wq = a.warmq ? D.out(hwq.data(), hwq.size(), false) : D.mem.alloc<double>(MPC_WQ_NQ * D.nb);
        Ws.hist_ubar = D.out(a.hist_ubar, nhs * nN * 2);
    }
    rc = D.begin();
    if (rc) return rc;
    const dim3 tb = D.tb, tg = D.tg;
    const dim3 wb(64 * ((a.W + 63) / 64)), wg(B / a.W);              // a workgroup per world
    hipLaunchKernelGGL(tr_init_kernel, tg, tb, 0, st, B, A, C, S, T, D.xinit, a.s_stop, max_steps);
    if (a.worlds) hipLaunchKernelGGL(cv_init_kernel, tg, tb, 0, st, B, T);
    if (a.noisy) hipLaunchKernelGGL(nz_init_kernel, tg, tb, 0, st, B, T);
    if (G.n_look) hipLaunchKernelGGL(tg_init_kernel, tg, tb, 0, st, B, G);
    if (a.warm) hipLaunchKernelGGL(ws_init_kernel, tg, tb, 0, st, B, Ws);
    rc = D.run(kp, a.with_slab, true,
               [&](int step, int nl, dim3 lg) {
                   hipLaunchKernelGGL(tr_fsm_kernel, tg, tb, 0, st, B, A, kp.dt, C, S, T, step, max_steps);
                   if (a.worlds) hipLaunchKernelGGL(cv_lead_kernel, wg, wb, 0, st, B, A, C, S, T, V, step, max_steps);
                   if (a.noisy) hipLaunchKernelGGL(nz_measure_kernel, lg, tb, 0, st, nl, B, AK, C, S, T, Z, step, max_steps);
                   else hipLaunchKernelGGL(tr_gather_kernel, lg, tb, 0, st, nl, B, AK, C, T);
                   if (a.warm) hipLaunchKernelGGL(ws_carry_kernel, lg, tb, 0, st, c->tab, nl, B, C, S, Ws, step, max_steps);
               },
               [&](int step, int nl, dim3 lg) {
                   if (a.noisy)
                       hipLaunchKernelGGL(nz_plant_kernel, lg, tb, 0, st, c->tab, B, nl, kp.dt, C, S, T, Z, a.s_stop, step,
                                          max_steps);
                   else
                       hipLaunchKernelGGL(sw_plant_kernel, lg, tb, 0, st, c->tab, B, nl, kp.dt, C, S, a.s_stop, step,
                                          max_steps);
                   if (G.n_look) hipLaunchKernelGGL(tg_gap_kernel, lg, tb, 0, st, nl, B, C, S, G, step);
                   if (G.hist_pred || G.hist_plan) {
                       const size_t ne = (size_t)nl * (size_t)(7 * G.N + 5);    // 5 (N + 1) + 2 N elements per ego
                       hipLaunchKernelGGL(tg_hist_kernel, dim3((unsigned)((ne + 255) / 256)), tb, 0, st, nl, C, S, G, step,
                                          max_steps);
                   }
                   if (a.warm) hipLaunchKernelGGL(ws_keep_kernel, lg, tb, 0, st, nl, B, C, S, Ws, step);
               },
               d_U, d_Xp, Ws.ubara);
    if (rc == MPC_SUCCESS) rc = D.finish(S, T.ex, a.nx(), a.quant, a.extra, a.n_steps, a.step_ms);
    if (rc == MPC_SUCCESS)                  // field-major on the device, one row per ego and lookahead outside
        for (size_t b = 0; b < D.nb; ++b)
            for (size_t k = 0; k < (size_t)a.n_look * MPC_TG_NQ; ++k) a.gapq[b * a.n_look * MPC_TG_NQ + k] = hgap[k * D.nb + b];
    if (rc == MPC_SUCCESS && a.warmq)
        for (size_t b = 0; b < D.nb; ++b)
            for (size_t k = 0; k < MPC_WQ_NQ; ++k) a.warmq[b * MPC_WQ_NQ + k] = hwq[k * D.nb + b];
    return rc;
}

// mpc_closed_loop_sweep with a script of A actors per ego (include/mpcqp.h)
extern "C" int mpc_closed_loop_traffic(mpc_ctx* c, int B, const double* x_init, const mpc_actor* actors, int A,
                                       int n_scripts, int max_steps, double s_stop, double* quant, double* extra,
                                       int n_hist, const int* hist_egos, double* hist_x, double* hist_u,
                                       double* hist_car_s, int* hist_tl, int* hist_status, int* hist_nobs,
                                       double* hist_slab, int* n_steps, double* step_ms) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0 || max_steps < 1) return fail(MPC_E_ARG, "B < 0 or max_steps < 1");
    ScriptedLoop a;
    a.label = "traffic";
    int rc = cl_check_script(actors, A, n_scripts, B, a.with_slab);
    if (rc) return rc;
    rc = cl_check_outputs(quant, n_hist, hist_x || hist_u || hist_car_s || hist_tl || hist_status || hist_nobs || hist_slab);
    if (rc) return rc;
    if (hist_slab && A == 0) return fail(MPC_E_ARG, "hist_slab is given but A == 0");
    a.B = B; a.x_init = x_init; a.max_steps = max_steps; a.s_stop = s_stop;
    a.actors = actors; a.A = A; a.n_scripts = n_scripts;
    a.quant = quant; a.extra = extra; a.n_hist = n_hist; a.hist_egos = hist_egos; a.hist_x = hist_x; a.hist_u = hist_u;
    a.hist_car_s = hist_car_s; a.hist_tl = hist_tl; a.hist_status = hist_status; a.hist_nobs = hist_nobs;
    a.hist_slab = hist_slab; a.n_steps = n_steps; a.step_ms = step_ms;
    return scripted_loop(c, a);
}

// mpc_closed_loop_traffic with the egos of a world as each other's obstacles (include/mpcqp.h)
extern "C" int mpc_closed_loop_convoy(mpc_ctx* c, int B, int W, int K, double lead_range, const double* x_init,
                                      const mpc_actor* actors, int A, int n_scripts, int max_steps, double s_stop,
                                      double* quant, double* extra, int n_hist, const int* hist_egos, double* hist_x,
                                      double* hist_u, double* hist_car_s, int* hist_tl, int* hist_status,
                                      int* hist_nobs, double* hist_slab, int* hist_lead, int* n_steps,
                                      double* step_ms) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (B < 0 || max_steps < 1) return fail(MPC_E_ARG, "B < 0 or max_steps < 1");
    int rc = cl_check_world(B, W, K, A, lead_range);
    if (rc) return rc;
    ScriptedLoop a;
    a.label = "convoy";
    a.with_slab = K > 0 && W > 1;
    rc = cl_check_script(actors, A, n_scripts, B, a.with_slab);
    if (rc) return rc;
    rc = cl_check_outputs(quant, n_hist, hist_x || hist_u || hist_car_s || hist_tl || hist_status || hist_nobs ||
                                             hist_slab || hist_lead);
    if (rc) return rc;
    if (hist_slab && A + K == 0) return fail(MPC_E_ARG, "hist_slab is given but A + K == 0");
    if (hist_lead && K == 0) return fail(MPC_E_ARG, "hist_lead is given but K == 0");
    a.B = B; a.x_init = x_init; a.max_steps = max_steps; a.s_stop = s_stop;
    a.actors = actors; a.A = A; a.n_scripts = n_scripts;
    a.worlds = true; a.W = W; a.K = K; a.lead_range = lead_range;
    a.quant = quant; a.extra = extra; a.n_hist = n_hist; a.hist_egos = hist_egos; a.hist_x = hist_x; a.hist_u = hist_u;
    a.hist_car_s = hist_car_s; a.hist_tl = hist_tl; a.hist_status = hist_status; a.hist_nobs = hist_nobs;
    a.hist_slab = hist_slab; a.hist_lead = hist_lead; a.n_steps = n_steps; a.step_ms = step_ms;
    return scripted_loop(c, a);
}

// mpc_closed_loop_noisy, _traced and _warm (include/mpcqp.h) behind one argument check: each fills the request with
// the arguments it has (the noisy entry has no trace output, the traced one no warm start), this sets what follows
// from them.  noise == NULL runs the same kernels on an all-zero shared struct
static int noisy_entry(mpc_ctx* c, ScriptedLoop& a) {
    if (!c) return fail(MPC_E_ARG, "ctx is NULL");
    if (a.B < 0 || a.max_steps < 1) return fail(MPC_E_ARG, "B < 0 or max_steps < 1");
    int rc = cl_check_world(a.B, a.W, a.K, a.A, a.lead_range);
    if (rc) return rc;
    a.worlds = a.noisy = true;
    a.with_slab = a.K > 0 && a.W > 1;
    rc = cl_check_script(a.actors, a.A, a.n_scripts, a.B, a.with_slab);
    if (rc) return rc;
    if (a.noise ? !(a.n_noise == 1 || a.n_noise == a.B) : a.n_noise != 0)
        return fail(MPC_E_ARG, "n_noise must be B (a struct per ego), 1 (shared) or 0 with noise NULL");
    if (a.ego_offset < 0) return fail(MPC_E_ARG, "ego_offset < 0");
    rc = cl_check_outputs(a.quant, a.n_hist, a.hist_x || a.hist_u || a.hist_ua || a.hist_xm || a.hist_car_s || a.hist_tl ||
                                                 a.hist_status || a.hist_nobs || a.hist_slab || a.hist_lead ||
                                                 a.hist_pred || a.hist_plan || a.hist_ubar);
    if (rc) return rc;
    mpc_warm wdef;
    mpc_default_warm(&wdef);
    const mpc_warm* warm = a.warm ? a.warm : &wdef;
    if (warm->mode != MPC_WARM_REFERENCE && warm->mode != MPC_WARM_CARRY)
        return fail(MPC_E_ARG, "warm.mode is neither MPC_WARM_REFERENCE nor MPC_WARM_CARRY");
    if (warm->tail != MPC_WTAIL_REFERENCE && warm->tail != MPC_WTAIL_HOLD)
        return fail(MPC_E_ARG, "warm.tail is neither MPC_WTAIL_REFERENCE nor MPC_WTAIL_HOLD");
    if (warm->reset & ~(MPC_WRESET_NOBS | MPC_WRESET_INFEASIBLE | MPC_WRESET_MAX_ITER))
        return fail(MPC_E_ARG, "warm.reset has unknown bits");
    if (warm->mode == MPC_WARM_CARRY && c->p.sqp_iters == 0)
        return fail(MPC_E_ARG, "MPC_WARM_CARRY needs sqp_iters >= 1 (sqp_iters == 0 returns ubar itself)");
    // the reference warm start with no warm output: the solver computes it for itself, the traced entry's kernels
    a.warm = warm->mode == MPC_WARM_CARRY || a.warmq || a.hist_ubar ? warm : nullptr;
    if (a.n_look < 0 || a.n_look > MPC_MAX_LOOK) return fail(MPC_E_ARG, "n_look out of range [0, 4]");
    if (a.n_look > 0 && !a.lookahead) return fail(MPC_E_ARG, "lookahead is NULL but n_look > 0");
    if (a.n_look > 0 ? !a.gapq : a.gapq != nullptr)
        return fail(MPC_E_ARG, "gapq is required with n_look > 0 and must be NULL with n_look == 0");
    for (int i = 0; i < a.n_look; ++i) {
        if (a.lookahead[i] < 1 || a.lookahead[i] > c->p.N) return fail(MPC_E_ARG, "a lookahead is outside [1, N]");
        for (int k = 0; k < i; ++k)
            if (a.lookahead[k] == a.lookahead[i]) return fail(MPC_E_ARG, "a lookahead is repeated");
    }
    if (a.hist_slab && a.A + a.K == 0) return fail(MPC_E_ARG, "hist_slab is given but A + K == 0");
    if (a.hist_lead && a.K == 0) return fail(MPC_E_ARG, "hist_lead is given but K == 0");
    for (size_t k = 0; k < (size_t)a.n_noise * NZ_NSIG; ++k)     // mpc_noise is NZ_NSIG doubles, no padding
        if (!(reinterpret_cast<const double*>(a.noise)[k] >= 0.0))
            return fail(MPC_E_ARG, "a noise sigma is negative or NaN");
    return scripted_loop(c, a);
}

extern "C" int mpc_closed_loop_noisy(mpc_ctx* c, int B, int W, int K, double lead_range, const double* x_init,
                                     const mpc_actor* actors, int A, int n_scripts, const mpc_noise* noise,
                                     int n_noise, unsigned long long seed, long long ego_offset, int max_steps,
                                     double s_stop, double* quant, double* extra, int n_hist, const int* hist_egos,
                                     double* hist_x, double* hist_u, double* hist_ua, double* hist_xm,
                                     double* hist_car_s, int* hist_tl, int* hist_status, int* hist_nobs,
                                     double* hist_slab, int* hist_lead, int* n_steps, double* step_ms) {
    ScriptedLoop a;
    a.label = "noisy-loop";
    a.B = B; a.x_init = x_init; a.max_steps = max_steps; a.s_stop = s_stop;
    a.actors = actors; a.A = A; a.n_scripts = n_scripts;
    a.W = W; a.K = K; a.lead_range = lead_range;
    a.noise = noise; a.n_noise = n_noise; a.seed = seed; a.ego_offset = ego_offset;
    a.quant = quant; a.extra = extra; a.n_hist = n_hist; a.hist_egos = hist_egos; a.hist_x = hist_x; a.hist_u = hist_u;
    a.hist_ua = hist_ua; a.hist_xm = hist_xm; a.hist_car_s = hist_car_s; a.hist_tl = hist_tl; a.hist_status = hist_status;
    a.hist_nobs = hist_nobs; a.hist_slab = hist_slab; a.hist_lead = hist_lead; a.n_steps = n_steps; a.step_ms = step_ms;
    return noisy_entry(c, a);
}

extern "C" int mpc_closed_loop_traced(mpc_ctx* c, int B, int W, int K, double lead_range, const double* x_init,
                                      const mpc_actor* actors, int A, int n_scripts, const mpc_noise* noise,
                                      int n_noise, unsigned long long seed, long long ego_offset, int max_steps,
                                      double s_stop, double* quant, double* extra, int n_hist, const int* hist_egos,
                                      double* hist_x, double* hist_u, double* hist_ua, double* hist_xm,
                                      double* hist_car_s, int* hist_tl, int* hist_status, int* hist_nobs,
                                      double* hist_slab, int* hist_lead, int* n_steps, double* step_ms,
                                      const int* lookahead, int n_look, double* gapq, double* hist_pred,
                                      double* hist_plan) {
    ScriptedLoop a;
    a.label = "traced-loop";
    a.B = B; a.x_init = x_init; a.max_steps = max_steps; a.s_stop = s_stop;
    a.actors = actors; a.A = A; a.n_scripts = n_scripts;
    a.W = W; a.K = K; a.lead_range = lead_range;
    a.noise = noise; a.n_noise = n_noise; a.seed = seed; a.ego_offset = ego_offset;
    a.quant = quant; a.extra = extra; a.n_hist = n_hist; a.hist_egos = hist_egos; a.hist_x = hist_x; a.hist_u = hist_u;
    a.hist_ua = hist_ua; a.hist_xm = hist_xm; a.hist_car_s = hist_car_s; a.hist_tl = hist_tl; a.hist_status = hist_status;
    a.hist_nobs = hist_nobs; a.hist_slab = hist_slab; a.hist_lead = hist_lead; a.n_steps = n_steps; a.step_ms = step_ms;
    a.lookahead = lookahead; a.n_look = n_look; a.gapq = gapq; a.hist_pred = hist_pred; a.hist_plan = hist_plan;
    return noisy_entry(c, a);
}

// mpc_closed_loop_traced whose solver may be handed the ego's previous plan as its ubar (include/mpcqp.h)
extern "C" int mpc_closed_loop_warm(mpc_ctx* c, int B, int W, int K, double lead_range, const double* x_init,
                                    const mpc_actor* actors, int A, int n_scripts, const mpc_noise* noise, int n_noise,
                                    unsigned long long seed, long long ego_offset, int max_steps, double s_stop,
                                    double* quant, double* extra, int n_hist, const int* hist_egos, double* hist_x,
                                    double* hist_u, double* hist_ua, double* hist_xm, double* hist_car_s, int* hist_tl,
                                    int* hist_status, int* hist_nobs, double* hist_slab, int* hist_lead, int* n_steps,
                                    double* step_ms, const int* lookahead, int n_look, double* gapq, double* hist_pred,
                                    double* hist_plan, const mpc_warm* warm, double* warmq, double* hist_ubar) {
    ScriptedLoop a;
    a.label = "warm-loop";
    a.B = B; a.x_init = x_init; a.max_steps = max_steps; a.s_stop = s_stop;
    a.actors = actors; a.A = A; a.n_scripts = n_scripts;
    a.W = W; a.K = K; a.lead_range = lead_range;
    a.noise = noise; a.n_noise = n_noise; a.seed = seed; a.ego_offset = ego_offset;
    a.quant = quant; a.extra = extra; a.n_hist = n_hist; a.hist_egos = hist_egos; a.hist_x = hist_x; a.hist_u = hist_u;
    a.hist_ua = hist_ua; a.hist_xm = hist_xm; a.hist_car_s = hist_car_s; a.hist_tl = hist_tl; a.hist_status = hist_status;
    a.hist_nobs = hist_nobs; a.hist_slab = hist_slab; a.hist_lead = hist_lead; a.n_steps = n_steps; a.step_ms = step_ms;
    a.lookahead = lookahead; a.n_look = n_look; a.gapq = gapq; a.hist_pred = hist_pred; a.hist_plan = hist_plan;
    a.warm = warm; a.warmq = warmq; a.hist_ubar = hist_ubar;
    return noisy_entry(c, a);
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
    staging::Staging S(c->arena);
    long long* d_ego;
    int *d_step, *d_ch;
    unsigned* d_w;
    double* d_z;
    const bool bound = S.bind([&] {
        d_ego = S.in(ego, nn);
        d_step = S.in(step, nn);
        d_ch = S.in(channel, nn);
        d_w = S.out(words, nn * 4);
        d_z = S.out(z, nn);
    });
    if (!bound) return fail(MPC_E_ALLOC, "hipMalloc noise-draw buffers");
    hipStream_t st = c->stream;
    bool ok = S.upload(st) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(nz_draw_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, (unsigned)(seed & 0xffffffffull),
                           (unsigned)(seed >> 32), d_ego, d_step, d_ch, d_w, d_z);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && S.fetch(st) == hipSuccess;
    ok = S.sync(st) == hipSuccess && ok;
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
    staging::Staging S(c->arena);
    double *d_s, *d_d, *d_out;
    const bool bound = S.bind([&] {
        d_s = S.in(s, (size_t)n);
        d_d = S.in(d, (size_t)n);
        d_out = S.out(out, 3 * (size_t)n);
    });
    if (!bound) return fail(MPC_E_ALLOC, "hipMalloc global pose staging");
    hipStream_t st = c->stream;
    int rc = MPC_SUCCESS;
    if (S.upload(st) != hipSuccess) {
        rc = fail(MPC_E_DEVICE, "hipMemcpy global pose inputs");
    } else {
        hipLaunchKernelGGL(mpc_pose_kernel, dim3((n + 255) / 256), dim3(256), 0, st, c->tab, n, d_s, d_d, d_out);
        if (hipGetLastError() != hipSuccess) rc = fail(MPC_E_LAUNCH, "global pose kernel");
        else if (S.fetch(st) != hipSuccess || S.sync(st) != hipSuccess) rc = fail(MPC_E_DEVICE, "hipMemcpy global pose");
    }
    if (rc) S.sync(st);     // the caller's arrays are free again when the entry returns
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
    double *d_s, *d_state, *d_control;
    return staged_call(c, "hipMalloc lookup", [&](staging::Staging& S) {
        d_s = S.in(s, (size_t)n);
        d_state = S.out_or_scratch(out_state, 5 * (size_t)n);     // the kernel writes both
        d_control = S.out_or_scratch(out_control, 2 * (size_t)n);
    }, [&] {
        hipLaunchKernelGGL(mpc_lookup_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->tab, n, d_s, d_state,
                           d_control);
        HIPCHK(hipGetLastError(), MPC_E_LAUNCH);
        return (int)MPC_SUCCESS;
    });
}

// multi-GPU: the ego-shard communicator (RCCL gather behind the C ABI)
#include "comm.h"
