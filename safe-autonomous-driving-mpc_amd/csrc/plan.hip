// plan.hip — MI355X batched offline planner: libmpcplan.so (C ABI: include/mpcplan.h).
//
// The chunk NLP of the reference's offline planner (TrajectoryOptimizer, trajectory_planning.py:8-391,
// driven by optimize_full_trajectory :419-559) solved for B independent chunks per launch, FP64.  The
// algorithm is the one DESIGN.md ("Offline planner") describes and oracle/plan_oracle.c restates on the CPU
// (the tests' checker; nothing here includes, links or calls it):
//   Gauss-Newton / exact-Hessian SQP over z = [X, U, S] from the reference's initial guess (:357-376), a
//   non-monotone L1-merit line search, speed limits frozen after a 2-cycle at a limit change; each QP by an
//   active-set crossover from the previous QP's active rows, else a Mehrotra interior point on the
//   stage-wise Riccati recursion followed by the same equality-constrained solve ("polish").
//
// Mapping: one wavefront (one 64-lane workgroup) = one chunk, its whole working set in LDS (265 doubles per
// stage, about 37 KB at N = 16: four chunks per CU).  Everything that is independent per stage runs
// stage-parallel, lane k on stage k: the linearisation (Hermite-Simpson Jacobians, the exact-Hessian fold),
// the barrier-weighted stage Hessians, the interior point's row residuals, directions, ratio tests and
// updates, the merit evaluations of the line search (defects of every interval), the multiplier recovery.
// The Riccati factorisation and its backward / forward recursions are sequential in the stage and run
// lane-distributed inside the wave (plan_kernel.h: factor_par, solve_core).  Reductions (complementarity,
// step lengths, norms) are wave shuffles.  Every chunk's wave retires on its own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mpcplan.h"
#include "../../include/mpcplan_evaluate.h"
#include "staging.h"
#include "plan_kernel.h"
#include "plan_evaluate_kernel.h"
#include "plan_host.h"
#include "plan_evaluate_host.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

size_t lds_bytes(int Nmax) { return sizeof(double) * (size_t)make_layout(Nmax).total; }

}  // namespace

struct plan_ctx {
    int device;
    plan_params p;
    plan_host::route* host;   // device = -1: the host backend's route (plan_host.h); every HIP member unused
    int host_threads;
    DevRoute R;
    double* d_route;          // s | cx | cy | vmax
    size_t lds_max;           // the device's LDS per workgroup
    staging::Arena arena;     // what the host entries stage their arrays through (staging.h)
    // longest-first dispatch (plan_order_*_kernel): a small pool of buffers (2 * ORDER_BUCKETS counters, then
    // bucket[cap], order[cap]), each remembering the stream it last served and an event recorded after its last
    // chunk kernel.  A call prefers its stream's buffer, else a new one (up to ORDER_POOL), else the least
    // recently used; before using a buffer it waits for that buffer's event, so a buffer is never rewritten
    // while an earlier plan_chunk_kernel still reads its order[] (whatever stream that ran on, and whether or
    // not a new stream reuses a destroyed stream's address).  Concurrent launches on distinct streams keep
    // distinct buffers.  A call on a stream that is being captured into a graph never uses the pool (index
    // order, same results): a graph must not replay order kernels against a buffer shared with eager calls.
    struct OrderBuf {
        int* ptr;
        hipEvent_t done;
        void* stream;
        unsigned long long last_use;
        bool used;
    };
    std::vector<OrderBuf> order_bufs;
    unsigned long long order_clock;
    std::mutex order_mu;
    int cap_order;
    bool order_on;
};

#define ORDER_POOL 8

// the buffer this call may use (its event already waited on by `stream`), or nullptr: index order (the stream
// is being captured, or an allocation failed)
static plan_ctx::OrderBuf* order_buffer(plan_ctx* c, void* stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
    std::lock_guard<std::mutex> g(c->order_mu);
    plan_ctx::OrderBuf* b = nullptr;
    for (auto& e : c->order_bufs)
        if (e.stream == stream) b = &e;
    if (!b && c->order_bufs.size() < ORDER_POOL) {
        plan_ctx::OrderBuf e{};
        if (hipMalloc(&e.ptr, sizeof(int) * (2 * (size_t)ORDER_BUCKETS + 2 * (size_t)c->cap_order)) != hipSuccess)
            return nullptr;
        if (hipEventCreateWithFlags(&e.done, hipEventDisableTiming) != hipSuccess) {
            (void)hipFree(e.ptr);
            return nullptr;
        }
        c->order_bufs.push_back(e);
        b = &c->order_bufs.back();
    }
    if (!b) {
        b = &c->order_bufs[0];
        for (auto& e : c->order_bufs)
            if (e.last_use < b->last_use) b = &e;
    }
    if (b->used && hipStreamWaitEvent((hipStream_t)stream, b->done, 0) != hipSuccess) return nullptr;
    b->stream = stream;
    b->last_use = ++c->order_clock;
    return b;
}

static int check_params(const plan_params* p) {
    if (!p) return fail(PLAN_E_ARG, "params is NULL");
    if (!(p->dt > 0.0)) return fail(PLAN_E_ARG, "dt must be > 0");
    if (p->N < 1 || p->N > PLAN_MAX_N) return fail(PLAN_E_ARG, "N out of range [1, PLAN_MAX_N]");
    if (p->sqp_iters < 1 || p->max_iter < 1) return fail(PLAN_E_ARG, "sqp_iters and max_iter must be >= 1");
    if (!(p->sqp_tol >= 0.0) || !(p->tol > 0.0)) return fail(PLAN_E_ARG, "tolerances must be positive");
    if (!(p->defect_sign == 1.0 || p->defect_sign == -1.0)) return fail(PLAN_E_ARG, "defect_sign must be +1 or -1");
    if (!(p->u_min[0] < p->u_max[0]) || !(p->u_min[1] < p->u_max[1]) || !(p->k_min < p->k_max))
        return fail(PLAN_E_ARG, "bounds must satisfy min < max");
    return PLAN_SUCCESS;
}

// The checks each host / device pair of entries shares; B == 0 passes (the entry returns success on it).  A device
// entry refuses a host context before it calls its pair's
static int chunks_args(plan_ctx* c, int B, const double* x0, const double* s_target) {
    if (!c) return fail(PLAN_E_ARG, "ctx is NULL");
    if (B < 0) return fail(PLAN_E_ARG, "B must be >= 0");
    if (B == 0) return PLAN_SUCCESS;
    if (!x0 || !s_target) return fail(PLAN_E_ARG, "x0 and s_target are required");
    return PLAN_SUCCESS;
}

static int optimize_args(plan_ctx* c, const char* entry, int B, int Nmax, std::initializer_list<const void*> arrays,
                         double max_chunk_size, int max_chunks, int nav) {
    if (!c) return fail(PLAN_E_ARG, "ctx is NULL");
    if (B < 0) return fail(PLAN_E_ARG, "B must be >= 0");
    if (B == 0) return PLAN_SUCCESS;
    for (const void* a : arrays)
        if (!a) return fail(PLAN_E_ARG, std::string(entry) + ": every array is required");
    if (Nmax < 1 || Nmax > PLAN_MAX_N) return fail(PLAN_E_ARG, "Nmax out of range [1, PLAN_MAX_N]");
    if (max_chunks < 1) return fail(PLAN_E_ARG, "max_chunks must be >= 1");
    if (nav < 1) return fail(PLAN_E_ARG, "avg must have at least one entry");
    if (!(max_chunk_size > 0.0) || !std::isfinite(max_chunk_size)) return fail(PLAN_E_ARG, "max_chunk_size must be > 0");
    return PLAN_SUCCESS;
}

// *lds = the dynamic LDS `kernel` needs at row stride Nmax on the context's device; above 64 KiB its limit is raised
static int kernel_lds(plan_ctx* c, int Nmax, const void* kernel, size_t* lds) {
    *lds = lds_bytes(Nmax);
    if (*lds > c->lds_max) return fail(PLAN_E_ARG, "Nmax too large for the device's LDS");
    if (hipSetDevice(c->device) != hipSuccess) return fail(PLAN_E_DEVICE, "hipSetDevice failed");
    if (*lds > 65536 && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds) != hipSuccess)
        return fail(PLAN_E_LAUNCH, "cannot raise the kernel's LDS limit");
    return PLAN_SUCCESS;
}

// A host entry's round trip: its arrays bound to the context's arena (staging.h), then in blocking order on the null
// stream the uploads, its device twin on the device arrays, a device synchronisation and the downloads
template <typename Bind, typename Call>
static int staged_call(plan_ctx* c, const char* kernel, Bind&& bindings, Call&& device_entry) {
    staging::Staging S(c->arena);
    if (!S.bind([&] { bindings(S); })) return fail(PLAN_E_ALLOC, "staging allocation failed");
    if (S.upload() != hipSuccess) return fail(PLAN_E_DEVICE, "input upload failed");
    if (int rc = device_entry()) return rc;
    if (hipError_t e = S.sync(); e != hipSuccess)
        return fail(PLAN_E_DEVICE, std::string(kernel) + " failed: " + hipGetErrorString(e));
    if (S.fetch() != hipSuccess) return fail(PLAN_E_DEVICE, "output download failed");
    return PLAN_SUCCESS;
}

extern "C" {

void plan_default_params(plan_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->N = 20;
    p->dt = 0.3;
    p->w_y = 10.0; p->w_s = 10.0; p->w_u = 0.1; p->w_slack = 100.0;
    p->u_min[0] = -0.6; p->u_min[1] = -5.0;
    p->u_max[0] = 0.6; p->u_max[1] = 4.0;
    p->k_min = -0.8; p->k_max = 0.8;
    p->a_max = 6.0;
    p->v_min = 0.0;
    p->defect_sign = 1.0;
    p->sqp_iters = 100;
    p->sqp_tol = 1e-9;
    p->max_iter = 100;
    p->tol = 1e-10;
}

const char* plan_last_error(void) { return g_err.c_str(); }
int plan_version(void) { return MPCPLAN_VERSION; }

int plan_create(const double* s, int M, const double* cx, const double* cy, const double* vmax, const plan_params* p,
                int device, plan_ctx** out) {
    if (!out) return fail(PLAN_E_ARG, "out is NULL");
    *out = nullptr;
    if (!s || !cx || !cy || !vmax) return fail(PLAN_E_ARG, "route arrays must not be NULL");
    if (M < 3) return fail(PLAN_E_ARG, "a route needs at least 3 way-points");
    for (int i = 1; i < M; ++i)
        if (!(s[i] > s[i - 1])) return fail(PLAN_E_ARG, "route s must be strictly increasing");
    for (int i = 0; i < 4 * (M - 1); ++i)
        if (!std::isfinite(cx[i]) || !std::isfinite(cy[i])) return fail(PLAN_E_ARG, "spline coefficients must be finite");
    for (int i = 0; i < M; ++i)
        if (!std::isfinite(vmax[i])) return fail(PLAN_E_ARG, "speed limits must be finite");
    if (int rc = check_params(p)) return rc;
    if (device == -1) {
        // host backend: the chunk solve on std::thread workers (plan_host.h), no HIP call
        plan_ctx* c = new plan_ctx();
        c->device = -1;
        c->p = *p;
        if (plan_host::route_create(s, M, cx, cy, vmax, &c->host) != PLAN_SUCCESS) {
            delete c;
            return fail(PLAN_E_ALLOC, "host route allocation failed");
        }
        const char* te = std::getenv("PLAN_CPU_THREADS");
        const int hw = (int)std::thread::hardware_concurrency();
        c->host_threads = te && std::atoi(te) > 0 ? std::atoi(te) : std::max(1, hw);
        *out = c;
        return PLAN_SUCCESS;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PLAN_E_DEVICE, "no HIP device");
    if (device < 0 || device >= ndev) return fail(PLAN_E_DEVICE, "device index out of range (-1: the host backend)");
    if (hipSetDevice(device) != hipSuccess) return fail(PLAN_E_DEVICE, "hipSetDevice failed");
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) lds = 65536;
    plan_ctx* c = new plan_ctx();
    c->device = device;
    c->p = *p;
    c->lds_max = (size_t)lds;
    // route arrays (s | cx | cy | vmax) followed by the search grid (ints), one allocation
    const int T = std::max(64, std::min(1 << 18, 4 * M));
    const size_t n = (size_t)M + 8 * (size_t)(M - 1) + M;
    const size_t nb = n * sizeof(double) + sizeof(int) * (size_t)T;
    if (hipMalloc(&c->d_route, nb) != hipSuccess) {
        delete c;
        return fail(PLAN_E_ALLOC, "route allocation failed");
    }
    std::vector<double> h(n + (T + 1) / 2);
    std::memcpy(h.data(), s, sizeof(double) * M);
    std::memcpy(h.data() + M, cx, sizeof(double) * 4 * (M - 1));
    std::memcpy(h.data() + M + 4 * (M - 1), cy, sizeof(double) * 4 * (M - 1));
    std::memcpy(h.data() + M + 8 * (M - 1), vmax, sizeof(double) * M);
    double ginv = 0.0;
    route_grid(s, M, T, (int*)(h.data() + n), &ginv);
    if (hipMemcpy(c->d_route, h.data(), nb, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(c->d_route);
        delete c;
        return fail(PLAN_E_DEVICE, "route upload failed");
    }
    c->R.s = c->d_route;
    c->R.cx = c->d_route + M;
    c->R.cy = c->d_route + M + 4 * (M - 1);
    c->R.vmax = c->d_route + M + 8 * (M - 1);
    c->R.grid = (const int*)(c->d_route + n);
    c->R.T = T;
    c->R.ginv = ginv;
    c->R.M = M;
    c->R.s_total = s[M - 1];
    c->cap_order = 1 << 17;
    c->order_bufs.reserve(ORDER_POOL);      // never reallocated: buffer pointers stay valid
    const char* oe = std::getenv("PLAN_ORDER");        // PLAN_ORDER=0: index order (A/B)
    c->order_on = !(oe && oe[0] == '0');
    *out = c;
    return PLAN_SUCCESS;
}

int plan_set_params(plan_ctx* c, const plan_params* p) {
    if (!c) return fail(PLAN_E_ARG, "ctx is NULL");
    if (int rc = check_params(p)) return rc;
    c->p = *p;
    return PLAN_SUCCESS;
}

void plan_destroy(plan_ctx* c) {
    if (!c) return;
    if (c->host) {
        plan_host::route_destroy(c->host);
        delete c;
        return;
    }
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    if (c->d_route) (void)hipFree(c->d_route);
    c->arena.release();
    for (auto& e : c->order_bufs) {
        (void)hipFree(e.ptr);
        (void)hipEventDestroy(e.done);
    }
    delete c;
}

int plan_solve_chunks_device(plan_ctx* c, int B, int Nmax, const int* N, const double* x0, const double* s_target,
                             const int* is_final, double* X, double* U, double* S, int* status, int* iters, int* sqp,
                             void* stream) {
    if (c && c->host) return fail(PLAN_E_DEVICE, "plan_solve_chunks_device on a host context (device = -1): use plan_solve_chunks");
    if (int rc = chunks_args(c, B, x0, s_target); rc || B == 0) return rc;
    // Nmax is always the caller's row stride; without per-chunk N every chunk has the params' horizon
    if (Nmax < 1 || Nmax > PLAN_MAX_N) return fail(PLAN_E_ARG, "Nmax out of range [1, PLAN_MAX_N]");
    if (!N && Nmax < c->p.N) return fail(PLAN_E_ARG, "Nmax must be >= params N when N is NULL (Nmax is the row stride)");
    size_t lds = 0;
    if (int rc = kernel_lds(c, Nmax, (const void*)plan_chunk_kernel, &lds)) return rc;
    KArgs a;
    a.R = c->R;
    a.P = c->p;
    a.B = B;
    a.Nmax = Nmax;
    a.Nfixed = c->p.N;
    // PLAN_DBG (diagnostics only): repeats a phase for A/B timing, the results do not change.  Bits: 1 each
    // interior-point factorisation, 2 each solve, 4 the interior point's gradient/row loop, 8 its direction
    // loop, 16 build_qp, 32 multipliers, 64 each line-search merit evaluation
    const char* dbg = std::getenv("PLAN_DBG");
    a.dbg = dbg ? std::atoi(dbg) : 0;
    a.N = N;
    a.x0 = x0;
    a.st = s_target;
    a.order = nullptr;
    plan_ctx::OrderBuf* ob = (c->order_on && B >= 2 * WAVE && B <= c->cap_order) ? order_buffer(c, stream) : nullptr;
    if (ob) {
        int* cnt = ob->ptr;
        int* bucket = cnt + 2 * ORDER_BUCKETS;
        int* order = bucket + c->cap_order;
        const int nb = (B + 255) / 256;
        if (hipMemsetAsync(cnt, 0, sizeof(int) * 2 * ORDER_BUCKETS, (hipStream_t)stream) != hipSuccess)
            return fail(PLAN_E_LAUNCH, "order reset failed");
        hipLaunchKernelGGL(plan_order_count_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, c->R, c->p, B, x0,
                           s_target, bucket, cnt);
        hipLaunchKernelGGL(plan_order_scatter_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, B, bucket, cnt,
                           cnt + ORDER_BUCKETS, order);
        if (hipError_t e = hipGetLastError(); e != hipSuccess)
            return fail(PLAN_E_LAUNCH, std::string("order kernels failed: ") + hipGetErrorString(e));
        a.order = order;
    }
    a.fin = is_final;
    a.X = X;
    a.U = U;
    a.S = S;
    a.status = status;
    a.iters = iters;
    a.sqp = sqp;
    hipLaunchKernelGGL(plan_chunk_kernel, dim3(B), dim3(WAVE), lds, (hipStream_t)stream, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return fail(PLAN_E_LAUNCH, std::string("plan kernel launch failed: ") + hipGetErrorString(e));
    if (ob) {
        // the buffer is free again once this kernel has read its order[]
        std::lock_guard<std::mutex> g(c->order_mu);
        if (hipEventRecord(ob->done, (hipStream_t)stream) != hipSuccess)
            return fail(PLAN_E_DEVICE, "order buffer event record failed");
        ob->used = true;
    }
    return PLAN_SUCCESS;
}

int plan_chunks_per_cu(plan_ctx* c, int Nmax, int* out) {
    if (!c || !out) return fail(PLAN_E_ARG, "ctx and out are required");
    if (c->host) return fail(PLAN_E_DEVICE, "plan_chunks_per_cu on a host context (device = -1)");
    if (Nmax < 1 || Nmax > PLAN_MAX_N) return fail(PLAN_E_ARG, "Nmax out of range [1, PLAN_MAX_N]");
    size_t lds = 0;
    if (int rc = kernel_lds(c, Nmax, (const void*)plan_chunk_kernel, &lds)) return rc;
    // one workgroup (one wavefront) per chunk: the residency is set by the kernel's registers and its LDS
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)plan_chunk_kernel, WAVE, lds) != hipSuccess)
        return fail(PLAN_E_DEVICE, "occupancy query failed");
    *out = n;
    return PLAN_SUCCESS;
}

int plan_optimize_device(plan_ctx* c, int B, int Nmax, const double* starts, double max_chunk_size, int max_chunks,
                         const double* avg, int nav, double* X, double* U, double* S, int* N, int* is_final,
                         int* status, int* iters, int* sqp, int* nchunks, void* stream) {
    if (c && c->host) return fail(PLAN_E_DEVICE, "plan_optimize_device on a host context (device = -1): use plan_optimize");
    if (int rc = optimize_args(c, "plan_optimize_device", B, Nmax,
                               {starts, avg, X, U, S, N, is_final, status, iters, sqp, nchunks}, max_chunk_size, max_chunks, nav);
        rc || B == 0)
        return rc;
    size_t lds = 0;
    if (int rc = kernel_lds(c, Nmax, (const void*)plan_loop_kernel, &lds)) return rc;
    LArgs a;
    a.R = c->R;
    a.P = c->p;
    a.B = B;
    a.Nmax = Nmax;
    a.max_chunks = max_chunks;
    a.nav = nav;
    a.max_chunk_size = max_chunk_size;
    a.avg = avg;
    a.starts = starts;
    a.X = X;
    a.U = U;
    a.S = S;
    a.N = N;
    a.fin = is_final;
    a.status = status;
    a.iters = iters;
    a.sqp = sqp;
    a.nchunks = nchunks;
    hipLaunchKernelGGL(plan_loop_kernel, dim3(B), dim3(WAVE), lds, (hipStream_t)stream, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return fail(PLAN_E_LAUNCH, std::string("plan loop kernel launch failed: ") + hipGetErrorString(e));
    return PLAN_SUCCESS;
}

int plan_solve_chunks(plan_ctx* c, int B, const int* N, const double* x0, const double* s_target, const int* is_final,
                      double* X, double* U, double* S, int* status, int* iters, int* sqp) {
    if (int rc = chunks_args(c, B, x0, s_target); rc || B == 0) return rc;
    int Nmax = c->p.N;
    if (N) {
        Nmax = 0;
        for (int b = 0; b < B; ++b) {
            if (N[b] < 1 || N[b] > PLAN_MAX_N) return fail(PLAN_E_ARG, "N[b] out of range [1, PLAN_MAX_N]");
            Nmax = std::max(Nmax, N[b]);
        }
    }
    if (c->host) {
        plan_host::batch(c->host, &c->p, B, Nmax, N, x0, s_target, is_final, X, U, S, status, iters, sqp, c->host_threads);
        return PLAN_SUCCESS;
    }
    if (hipSetDevice(c->device) != hipSuccess) return fail(PLAN_E_DEVICE, "hipSetDevice failed");
    const size_t nb = (size_t)B, nm = (size_t)Nmax;
    double *d_x0, *d_st, *d_X, *d_U, *d_S;
    int *d_N, *d_fin, *d_status, *d_iters, *d_sqp;
    // the kernel writes all six outputs, asked for or not
    return staged_call(c, "plan kernel", [&](staging::Staging& G) {
        d_x0 = G.in(x0, nb * 5);
        d_st = G.in(s_target, nb);
        d_N = G.in(N, nb);
        d_fin = G.in(is_final, nb);
        d_X = G.out_or_scratch(X, nb * (nm + 1) * 5);
        d_U = G.out_or_scratch(U, nb * nm * 2);
        d_S = G.out_or_scratch(S, nb * nm);
        d_status = G.out_or_scratch(status, nb);
        d_iters = G.out_or_scratch(iters, nb);
        d_sqp = G.out_or_scratch(sqp, nb);
    }, [&] {
        return plan_solve_chunks_device(c, B, Nmax, d_N, d_x0, d_st, d_fin, d_X, d_U, d_S, d_status, d_iters, d_sqp, nullptr);
    });
}

int plan_optimize(plan_ctx* c, int B, int Nmax, const double* starts, double max_chunk_size, int max_chunks,
                  const double* avg, int nav, double* X, double* U, double* S, int* N, int* is_final, int* status,
                  int* iters, int* sqp, int* nchunks) {
    if (int rc = optimize_args(c, "plan_optimize", B, Nmax, {starts, avg, X, U, S, N, is_final, status, iters, sqp, nchunks},
                               max_chunk_size, max_chunks, nav);
        rc || B == 0)
        return rc;
    if (c->host) {
        plan_host::optimize(c->host, &c->p, B, Nmax, starts, max_chunk_size, max_chunks, avg, nav, X, U, S, N, is_final,
                            status, iters, sqp, nchunks, c->host_threads);
        return PLAN_SUCCESS;
    }
    if (hipSetDevice(c->device) != hipSuccess) return fail(PLAN_E_DEVICE, "hipSetDevice failed");
    const size_t nb = (size_t)B, nm = (size_t)Nmax, slots = nb * max_chunks;
    double *d_st, *d_avg, *d_X, *d_U, *d_S;
    int *d_N, *d_fin, *d_status, *d_iters, *d_sqp, *d_nch;
    return staged_call(c, "plan loop kernel", [&](staging::Staging& G) {
        d_st = G.in(starts, nb * 5);
        d_avg = G.in(avg, (size_t)nav);
        d_X = G.out(X, slots * (nm + 1) * 5);
        d_U = G.out(U, slots * nm * 2);
        d_S = G.out(S, slots * nm);
        d_N = G.out(N, slots);
        d_fin = G.out(is_final, slots);
        d_status = G.out(status, slots);
        d_iters = G.out(iters, slots);
        d_sqp = G.out(sqp, slots);
        d_nch = G.out(nchunks, nb);
    }, [&] {
        return plan_optimize_device(c, B, Nmax, d_st, max_chunk_size, max_chunks, d_avg, nav, d_X, d_U, d_S, d_N, d_fin,
                                    d_status, d_iters, d_sqp, d_nch, nullptr);
    });
}

// ---- the evaluator (plan_evaluate_kernel.h; host backend: plan_evaluate_host.h) ----
static int evaluate_args(plan_ctx* c, int B, int Nmax, const int* N, const double* x0, const double* s_target,
                         const double* X, const double* U) {
    if (!c) return fail(PLAN_E_ARG, "ctx is NULL");
    if (B < 0) return fail(PLAN_E_ARG, "B must be >= 0");
    if (B == 0) return PLAN_SUCCESS;
    if (!x0 || !s_target || !X || !U) return fail(PLAN_E_ARG, "plan_evaluate_chunks: x0, s_target, X and U are required");
    if (Nmax < 1) return fail(PLAN_E_ARG, "Nmax must be >= 1");
    if ((size_t)Nmax > ((size_t)1 << 26)) return fail(PLAN_E_ARG, "Nmax too large");
    if (!N && Nmax < c->p.N) return fail(PLAN_E_ARG, "Nmax must be >= params N when N is NULL (Nmax is the row stride)");
    return PLAN_SUCCESS;
}

int plan_evaluate_chunks_device(plan_ctx* c, int B, int Nmax, const int* N, const double* x0, const double* s_target,
                                const int* is_final, const double* X, const double* U, const double* S, double* summary,
                                double* defects, double* rows, void* stream) {
    if (int rc = evaluate_args(c, B, Nmax, N, x0, s_target, X, U)) return rc;
    if (B == 0 || (!summary && !defects && !rows)) return PLAN_SUCCESS;
    if (c->host) {
        // the host backend: host pointers, synchronous (include/mpcplan_evaluate.h documents the exception)
        plan_host::evaluate_batch(c->host, &c->p, B, Nmax, N, x0, s_target, is_final, X, U, S, summary, defects, rows,
                                  c->host_threads);
        return PLAN_SUCCESS;
    }
    if (hipSetDevice(c->device) != hipSuccess) return fail(PLAN_E_DEVICE, "hipSetDevice failed");
    EArgs a;
    a.R = c->R;
    a.P = c->p;
    a.B = B;
    a.Nmax = Nmax;
    a.Nfixed = c->p.N;
    a.N = N;
    a.x0 = x0;
    a.st = s_target;
    a.fin = is_final;
    a.X = X;
    a.U = U;
    a.S = S;
    a.sum = summary;
    a.def = defects;
    a.rows = rows;
    hipLaunchKernelGGL(plan_evaluate_kernel, dim3(B), dim3(WAVE), 0, (hipStream_t)stream, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return fail(PLAN_E_LAUNCH, std::string("plan evaluate kernel launch failed: ") + hipGetErrorString(e));
    return PLAN_SUCCESS;
}

int plan_evaluate_chunks(plan_ctx* c, int B, int Nmax, const int* N, const double* x0, const double* s_target,
                         const int* is_final, const double* X, const double* U, const double* S, double* summary,
                         double* defects, double* rows) {
    if (int rc = evaluate_args(c, B, Nmax, N, x0, s_target, X, U)) return rc;
    if (B == 0 || (!summary && !defects && !rows)) return PLAN_SUCCESS;
    if (c->host)
        return plan_evaluate_chunks_device(c, B, Nmax, N, x0, s_target, is_final, X, U, S, summary, defects, rows, nullptr);
    if (hipSetDevice(c->device) != hipSuccess) return fail(PLAN_E_DEVICE, "hipSetDevice failed");
    // a chunk whose N[b] is out of range leaves its rows and defects unwritten on the device; the caller's buffers
    // keep their contents there, as with device pointers: then the two are copied back chunk by chunk below
    bool all_in = true;
    for (int b = 0; b < B && N && all_in; ++b) all_in = N[b] >= 1 && N[b] <= Nmax;
    const size_t nb = (size_t)B, nm = (size_t)Nmax, def_row = nm * 5, rows_row = (nm + 1) * PLAN_EV_NR;
    double *d_x0, *d_st, *d_X, *d_U, *d_S, *d_Q, *d_D, *d_R;
    int *d_N, *d_fin;
    int rc = staged_call(c, "plan evaluate kernel", [&](staging::Staging& G) {
        d_x0 = G.in(x0, nb * 5);
        d_st = G.in(s_target, nb);
        d_X = G.in(X, nb * (nm + 1) * 5);
        d_U = G.in(U, nb * nm * 2);
        d_S = G.in(S, nb * nm);
        d_N = G.in(N, nb);
        d_fin = G.in(is_final, nb);
        d_D = all_in ? G.out(defects, nb * def_row) : (defects ? G.scratch<double>(nb * def_row) : nullptr);
        d_R = all_in ? G.out(rows, nb * rows_row) : (rows ? G.scratch<double>(nb * rows_row) : nullptr);
        d_Q = G.out(summary, nb * PLAN_EV_NQ);
    }, [&] {
        return plan_evaluate_chunks_device(c, B, Nmax, d_N, d_x0, d_st, d_fin, d_X, d_U, d_S, d_Q, d_D, d_R, nullptr);
    });
    bool ok = true;
    for (int b = 0; b < B && rc == PLAN_SUCCESS && ok && !all_in; ++b) {
        if (N[b] < 1 || N[b] > Nmax) continue;
        if (defects)
            ok = hipMemcpy(defects + b * def_row, d_D + b * def_row, sizeof(double) * def_row, hipMemcpyDeviceToHost) == hipSuccess;
        if (ok && rows)
            ok = hipMemcpy(rows + b * rows_row, d_R + b * rows_row, sizeof(double) * rows_row, hipMemcpyDeviceToHost) == hipSuccess;
    }
    return ok ? rc : fail(PLAN_E_DEVICE, "output download failed");
}

int plan_check_verdicts(const plan_ctx* c, int B, const double* summary, int* verdicts, int counts[8]) {
    if (!c) return fail(PLAN_E_ARG, "ctx is NULL");
    if (B < 0) return fail(PLAN_E_ARG, "B must be >= 0");
    if (B > 0 && !summary) return fail(PLAN_E_ARG, "summary is NULL");
    if (counts)
        for (int k = 0; k < 8; ++k) counts[k] = 0;
    for (int b = 0; b < B; ++b) {
        const int v = plan_host::check_verdict(&c->p, summary + (size_t)b * PLAN_EV_NQ);
        if (verdicts) verdicts[b] = v;
        if (counts)
            for (int k = 0; k < 8; ++k) counts[k] += (v >> k) & 1;
    }
    return PLAN_SUCCESS;
}

int plan_route_eval(plan_ctx* c, int n, const double* s, double* kappa, double* dkappa, double* vmax) {
    if (!c) return fail(PLAN_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!s || !kappa || !dkappa || !vmax))) return fail(PLAN_E_ARG, "bad arguments");
    if (n == 0) return PLAN_SUCCESS;
    if (c->host) {
        for (int i = 0; i < n; ++i) {
            kappa[i] = plan_host::route_kappa_at(c->host, s[i], &dkappa[i]);
            vmax[i] = plan_host::route_vmax_at(c->host, s[i]);
        }
        return PLAN_SUCCESS;
    }
    if (hipSetDevice(c->device) != hipSuccess) return fail(PLAN_E_DEVICE, "hipSetDevice failed");
    staging::Staging G(c->arena);
    double *d_s, *d_kappa, *d_dkappa, *d_vmax;
    const bool bound = G.bind([&] {
        d_s = G.in(s, (size_t)n);
        d_kappa = G.out(kappa, (size_t)n);
        d_dkappa = G.out(dkappa, (size_t)n);
        d_vmax = G.out(vmax, (size_t)n);
    });
    if (!bound) return fail(PLAN_E_ALLOC, "allocation failed");
    if (G.upload() != hipSuccess) return fail(PLAN_E_DEVICE, "upload failed");
    hipLaunchKernelGGL(route_eval_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, c->R, n, d_s, d_kappa, d_dkappa, d_vmax);
    if (hipGetLastError() != hipSuccess || G.sync() != hipSuccess) return fail(PLAN_E_LAUNCH, "route kernel failed");
    if (G.fetch() != hipSuccess) return fail(PLAN_E_DEVICE, "download failed");
    return PLAN_SUCCESS;
}

#ifdef PLAN_PROF
// diagnostic build only: summed s_memtime ticks per phase ([0, PH_COUNT)) and the chunk count ([15])
int plan_debug_prof(unsigned long long* out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_plan_prof), sizeof(unsigned long long) * 16) != hipSuccess)
        return fail(PLAN_E_DEVICE, "profile read failed");
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_plan_prof), z, sizeof(z)) != hipSuccess)
            return fail(PLAN_E_DEVICE, "profile reset failed");
    }
    return PLAN_SUCCESS;
}
#endif

}  // extern "C"
