// closed_loop_host.h -- the host-side driver behind the seven closed-loop entries of the C ABI (mpc_closed_loop,
// _sweep, _traffic, _convoy, _noisy, _traced, _warm).  Included by mpcqp.hip below launch_solve: it uses that file's fail(), mpc_ctx
// and launch_solve, and the state structs of the closed-loop kernel headers.
//
// An entry checks its arguments, declares its buffers and outputs on a ClDriver, launches its own init kernels and
// hands the loop two callables: what runs before the solve of a step and the plant kernel after it.  The five
// scripted entries do so in one place, scripted_loop() of mpcqp.hip, from the one ScriptedLoop request
// (scripted_loop.h) that the host backend takes too, with what follows from its fields stated there.  Everything
// else is here, once: the device-buffer owner, the output table (allocation, all-ones pre-fill and copy-back of a
// host output from one binding), the step-time event ring, the loop with its every-8-steps host sync and list
// compaction, and the copy-out of n_steps / quant / extra.
#ifndef MPCQP_CLOSED_LOOP_HOST_H
#define MPCQP_CLOSED_LOOP_HOST_H

// Step times come from a ring of SW_EVENTS events: step i ran between events i and i + 1 of the ring; they are read
// at a host sync, at most 8 steps after the last read, so no event is re-recorded before its interval has been taken
#define SW_EVENTS 9

// Owner of a call's device buffers: typed arrays, one ok() for all of them, everything freed when the owner goes.
// A request for zero elements allocates one, so a null pointer always means a failure
struct DevBufs {
    enum { CAP = 48 };
    void* bufs[CAP];
    int n = 0;
    bool failed = false;
    DevBufs() = default;
    DevBufs(const DevBufs&) = delete;
    DevBufs& operator=(const DevBufs&) = delete;
    ~DevBufs() {
        for (int i = 0; i < n; ++i) hipFree(bufs[i]);
    }
    template <typename T>
    T* alloc(size_t count) {
        void* ptr = nullptr;
        if (n == CAP || hipMalloc(&ptr, (count ? count : 1) * sizeof(T)) != hipSuccess) {
            failed = true;
            return nullptr;
        }
        bufs[n++] = ptr;
        return (T*)ptr;
    }
    bool ok() const { return !failed; }
};

// ------------------------------------------------------------------------------------------
// argument helpers of the entries
// ------------------------------------------------------------------------------------------
// hist_egos -> slot[b]: the history row of ego b, -1 for an ego whose history is not kept
static int cl_slot_map(int B, int n_hist, const int* hist_egos, std::vector<int>& slot) {
    if (n_hist > 0 && !hist_egos) return fail(MPC_E_ARG, "hist_egos is NULL but n_hist > 0");
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
    return MPC_SUCCESS;
}

// quant and the history count of the entries that keep histories for named egos only
static int cl_check_outputs(const double* quant, int n_hist, bool any_hist) {
    if (!quant) return fail(MPC_E_ARG, "quant is required");
    if (n_hist < 0) return fail(MPC_E_ARG, "n_hist < 0");
    if (n_hist == 0 && any_hist) return fail(MPC_E_ARG, "a history array is given but n_hist == 0");
    return MPC_SUCCESS;
}

// the scripts: [n_scripts][A] actors; with_slab becomes true when some actor of some script is not NONE
static int cl_check_script(const mpc_actor* actors, int A, int n_scripts, int B, bool& with_slab) {
    if (A < 0 || A > MPC_MAX_ACTORS) return fail(MPC_E_ARG, "A out of range [0, 16]");
    if (actors ? !(n_scripts == 1 || n_scripts == B) : n_scripts != 0)
        return fail(MPC_E_ARG, "n_scripts must be B (a script per ego), 1 (shared) or 0 with actors NULL");
    if (!actors && A != 0) return fail(MPC_E_ARG, "actors is NULL but A > 0");
    for (size_t k = 0; k < (size_t)n_scripts * (size_t)A; ++k) {
        if (actors[k].kind < MPC_ACTOR_NONE || actors[k].kind > MPC_ACTOR_LIGHT)
            return fail(MPC_E_ARG, "actor kind outside MPC_ACTOR_NONE .. MPC_ACTOR_LIGHT");
        with_slab = with_slab || actors[k].kind != MPC_ACTOR_NONE;
    }
    return MPC_SUCCESS;
}

// the worlds of the convoy entries: B egos in worlds of W, up to K leaders beside the A actors
static int cl_check_world(int B, int W, int K, int A, double lead_range) {
    if (W < 1 || W > MPC_MAX_WORLD) return fail(MPC_E_ARG, "W out of range [1, 256]");
    if (B % W != 0) return fail(MPC_E_ARG, "B is not a multiple of W");
    if (A < 0 || A > MPC_MAX_ACTORS) return fail(MPC_E_ARG, "A out of range [0, 16]");
    if (K < 0 || K > MPC_MAX_ACTORS) return fail(MPC_E_ARG, "K out of range [0, 16]");
    if (A + K > MPC_MAX_ACTORS) return fail(MPC_E_ARG, "A + K > 16");
    if (!(lead_range > 0.0)) return fail(MPC_E_ARG, "lead_range must be > 0 (+inf allowed)");
    return MPC_SUCCESS;
}

// ------------------------------------------------------------------------------------------
// the driver
// ------------------------------------------------------------------------------------------
struct ClDriver {
    mpc_ctx* const c;
    const char* const label;        // names the entry in the messages of device and allocation failures
    const int B, max_steps;
    const size_t nb, ns;
    const hipStream_t st;
    const dim3 tb, tg;              // one thread per ego
    DevBufs mem;
    ClState C;
    double* xinit = nullptr;        // [B][5] the start states, for the entry's init kernel

    // the output table: a host output bound to a device array of its own
    struct Out {
        void* host;
        void* dev;
        size_t bytes;
        bool fill;
    };
    // an input copied to the device before the init kernels run
    struct In {
        void* dev;
        const void* host;
        size_t bytes;
    };
    enum { MAX_OUTS = 16, MAX_INS = 4 };
    Out outs[MAX_OUTS];
    In ins[MAX_INS];
    int n_outs = 0, n_ins = 0;

    hipEvent_t ev[SW_EVENTS] = {};
    std::vector<double> ms;         // the step times read so far

    ClDriver(mpc_ctx* ctx, const char* name, int B_, int max_steps_)
        : c(ctx), label(name), B(B_), max_steps(max_steps_), nb((size_t)B_), ns((size_t)max_steps_), st(ctx->stream),
          tb(256), tg((B_ + 255) / 256), C() {}
    ClDriver(const ClDriver&) = delete;
    ClDriver& operator=(const ClDriver&) = delete;
    // every exit path: the stream drains, then the events and (DevBufs) the buffers go
    ~ClDriver() {
        hipStreamSynchronize(st);
        for (auto& e : ev)
            if (e) hipEventDestroy(e);
    }

    std::string msg(const char* what) const { return std::string(label) + " " + what; }

    // Binds the host output `host` of `count` elements (NULL: not asked for, nothing happens) to a device array:
    // allocated here, set to all-ones bytes by begin() when `fill` (NaN / -1: a step that never ran), copied back
    // by fetch().  Returns the device array, the pointer the kernels get
    template <typename T>
    T* out(T* host, size_t count, bool fill = true) {
        if (!host) return nullptr;
        T* dev = mem.alloc<T>(count);
        if (n_outs == MAX_OUTS) mem.failed = true;
        if (!mem.ok()) return nullptr;
        outs[n_outs++] = Out{host, dev, count * sizeof(T), fill};
        return dev;
    }

    // A device array of `count` elements whose first `n_copy` come from `host` in begin()
    template <typename T>
    T* in(const T* host, size_t count, size_t n_copy) {
        T* dev = mem.alloc<T>(count);
        if (n_ins == MAX_INS) mem.failed = true;
        if (!mem.ok()) return nullptr;
        if (n_copy) ins[n_ins++] = In{dev, host, n_copy * sizeof(T)};
        return dev;
    }

    // Device allocations of an entry, all made through the three blocks below and out() / in(): O(B) words per
    // ego for the state (times the slab width `ow` for the slab, times A for the per-actor state), O(1) counters,
    // and the kept histories [n_hist][max_steps ..] ([B][max_steps ..] for mpc_closed_loop).
    //
    // The loop's per-ego state and the solver's packed buffers, with an `ow`-entry slab per ego.  own_fsm: the FSM
    // state of mpc_closed_loop / _sweep lives here too; the scripted entries keep theirs in TrState and leave
    // obs, obs_s, tl_timer and fsm_flags null
    void cl_state(const double* x_init, size_t ow, bool own_fsm) {
        C.x = mem.alloc<double>(nb * 5);
        C.nobs = mem.alloc<int>(nb);
        C.active = mem.alloc<int>(nb);
        C.n_active = mem.alloc<int>(1);
        C.alist = mem.alloc<int>(nb);
        C.n_list = mem.alloc<int>(1);
        C.xa = mem.alloc<double>(nb * 5);
        C.obsa = mem.alloc<double>(nb * ow * 2);
        C.nobsa = mem.alloc<int>(nb);
        C.u0a = mem.alloc<double>(nb * 2);
        C.sta = mem.alloc<int>(nb);
        if (own_fsm) {
            C.obs = mem.alloc<double>(nb * 4);
            C.obs_s = mem.alloc<double>(nb);
            C.tl_timer = mem.alloc<double>(nb);
            C.fsm_flags = mem.alloc<int>(nb * 4);
        }
        xinit = in(x_init, nb * 5, nb * 5);
    }

    // The quantities [MPC_CL_NQ][B], their flags, the history slots and n_steps, and the five histories every
    // entry with named history egos has ([n_hist] rows)
    SwState sw_state(const int* slot, int n_hist, double* hist_x, double* hist_u, double* hist_obs_s, int* hist_tl,
                     int* hist_status) {
        const size_t nh = (size_t)n_hist;
        SwState S = {};
        S.q = mem.alloc<double>(nb * MPC_CL_NQ);
        S.qflags = mem.alloc<int>(nb);
        S.hslot = in(slot, nb, nb);
        S.n_steps = mem.alloc<int>(nb);
        S.hist_x = out(hist_x, nh * (ns + 1) * 5);
        S.hist_u = out(hist_u, nh * ns * 2);
        S.hist_obs_s = out(hist_obs_s, nh * ns);
        S.hist_tl = out(hist_tl, nh * ns);
        S.hist_status = out(hist_status, nh * ns);
        return S;
    }

    // The scripts ([B][A], or [A] when shared), the per-actor state [A][B], the slab [ow][2][B] of every ego, the
    // extras [nx][B] and hist_nobs; hist_slab is left to the entry (its rows are as wide as the entry's slab)
    TrState tr_state(const mpc_actor* actors, int A, int nsc, bool per_ego, size_t ow, int nx, int n_hist,
                     int* hist_nobs) {
        const size_t na = (size_t)A;
        TrState T = {};
        T.actors = in(actors, (per_ego ? nb : 1) * na, (size_t)nsc * na);
        T.per_ego = per_ego ? 1 : 0;
        T.aval = mem.alloc<double>(nb * na);
        T.aflags = mem.alloc<int>(nb * na);
        T.slab = mem.alloc<double>(nb * ow * 2);
        T.ex = mem.alloc<double>(nb * (size_t)nx);
        T.hist_nobs = out(hist_nobs, (size_t)n_hist * ns);
        return T;
    }

    // After the last allocation: the one check of them all, then the pre-fills and the inputs, in stream order
    int begin() {
        if (!mem.ok()) return fail(MPC_E_ALLOC, "hipMalloc " + msg("buffers"));
        bool ok = true;
        for (int i = 0; i < n_outs; ++i)
            if (outs[i].fill) ok = ok && hipMemsetAsync(outs[i].dev, 0xff, outs[i].bytes, st) == hipSuccess;
        for (int i = 0; i < n_ins; ++i)
            ok = ok && hipMemcpyAsync(ins[i].dev, ins[i].host, ins[i].bytes, hipMemcpyHostToDevice, st) == hipSuccess;
        return ok ? MPC_SUCCESS : fail(MPC_E_DEVICE, msg("buffer initialisation"));
    }

    // the solver's list of the egos still in the loop, rebuilt on the device; one host sync
    bool compact(int& nl) {
        hipLaunchKernelGGL(cl_compact_kernel, dim3(1), dim3(1024), 0, st, B, C);
        return hipMemcpyAsync(&nl, C.n_list, 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
               hipStreamSynchronize(st) == hipSuccess;
    }

    void read_times(int upto) {
        for (int i = (int)ms.size(); i < upto; ++i) {
            float t = NAN;
            if (hipEventElapsedTime(&t, ev[i % SW_EVENTS], ev[(i + 1) % SW_EVENTS]) != hipSuccess) t = NAN;
            ms.push_back(t);
        }
    }

    // The loop, after the entry's init kernels.  Per step: pre(step, nl, lg) launches what precedes the solve
    // (FSM, leaders, gather or measurement; lg: the grid of one thread per listed ego), launch_solve runs on the
    // nl listed egos (with the slab when with_obs), plant(step, nl, lg) launches the plant kernel.  The solve
    // runs on the egos still in the loop: the list is rebuilt at the every-8-steps host sync whenever egos have
    // left, so retired egos stop costing solver work (results are per ego, unchanged).  timed: record the ring.
    // Ua [B][N][2], Xpa [B][N+1][5] (device, optional): the solver's U and Xpred of the listed egos, by list
    // position, for the plant callable to use; u0 and the status do not depend on whether they are asked for.
    // ubara [B][N][2] (device, optional): the solver's linearisation point of the listed egos, by list position,
    // which pre() has filled; without it the solver computes the reference warm start for itself
    template <typename Pre, typename Plant>
    int run(const KParams& kp, bool with_obs, bool timed, Pre pre, Plant plant, double* Ua = nullptr,
            double* Xpa = nullptr, const double* ubara = nullptr) {
        if (timed) {
            for (auto& e : ev)
                if (hipEventCreate(&e) != hipSuccess) {
                    e = nullptr;
                    return fail(MPC_E_DEVICE, "hipEventCreate (step timing)");
                }
            if (hipEventRecord(ev[0], st) != hipSuccess) return fail(MPC_E_DEVICE, "hipEventRecord (step timing)");
        }
        int nl = 0;
        if (!compact(nl)) return fail(MPC_E_DEVICE, msg("initial ego list"));
        int rc = MPC_SUCCESS;
        try {
            for (int step = 0; step < max_steps && nl > 0; ++step) {
                const dim3 lg((nl + 255) / 256);
                pre(step, nl, lg);
                rc = launch_solve(c, kp, nl, C.xa, with_obs ? C.obsa : nullptr, with_obs ? C.nobsa : nullptr, ubara,
                                  C.u0a, Ua, Xpa, C.sta, nullptr, st);
                if (rc) break;
                if (hipMemsetAsync(C.n_active, 0, 4, st) != hipSuccess) {
                    rc = fail(MPC_E_DEVICE, msg("active-count reset"));
                    break;
                }
                plant(step, nl, lg);
                if (timed && hipEventRecord(ev[(step + 1) % SW_EVENTS], st) != hipSuccess) {
                    rc = fail(MPC_E_DEVICE, "hipEventRecord (step timing)");
                    break;
                }
                if ((step & 7) == 7 || step == max_steps - 1) {     // every 8 steps: has every ego left the loop?
                    int na = 0;
                    if (hipMemcpyAsync(&na, C.n_active, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                        hipStreamSynchronize(st) != hipSuccess) {
                        rc = fail(MPC_E_DEVICE, msg("step sync"));
                        break;
                    }
                    if (timed) read_times(step + 1);
                    if (na == 0) break;
                    if (na < nl && !compact(nl)) {                  // egos left: shrink the solver's list
                        rc = fail(MPC_E_DEVICE, msg("ego list"));
                        break;
                    }
                }
            }
        } catch (const std::bad_alloc&) {
            rc = fail(MPC_E_ALLOC, msg("host buffers"));
        }
        if (rc == MPC_SUCCESS && hipGetLastError() != hipSuccess) rc = fail(MPC_E_LAUNCH, msg("kernel launch"));
        return rc;
    }

    // every bound output back to its host array (asynchronous: the caller syncs)
    bool fetch() {
        bool ok = true;
        for (int i = 0; i < n_outs; ++i)
            ok = ok && hipMemcpyAsync(outs[i].host, outs[i].dev, outs[i].bytes, hipMemcpyDeviceToHost, st) == hipSuccess;
        return ok;
    }

    void fill_step_ms(double* step_ms) const {
        for (size_t i = 0; i < ns; ++i) step_ms[i] = i < ms.size() ? ms[i] : (double)NAN;
    }

    // Copy-out after a successful run(): n_steps, quant and the `nx`-wide extras (d_ex; extra NULL: not asked for)
    // are column-major on the device and leave as one row per ego; the bound outputs leave as they are; then
    // MPC_CLQ_MAX_STEP_MS from the ring's times, and step_ms.  One host sync
    int finish(const SwState& S, const double* d_ex, int nx, double* quant, double* extra, int* n_steps,
               double* step_ms) {
        try {
            const size_t nq = MPC_CL_NQ, nxs = (size_t)nx;
            std::vector<double> hq(nb * nq), hx(extra ? nb * nxs : 0);
            std::vector<int> hn(nb);
            bool ok = hipMemcpyAsync(hn.data(), S.n_steps, nb * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(hq.data(), S.q, nb * nq * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (extra) ok = ok && hipMemcpyAsync(hx.data(), d_ex, nb * nxs * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && fetch();
            ok = ok && hipStreamSynchronize(st) == hipSuccess;
            if (!ok) return fail(MPC_E_DEVICE, msg("copy-back"));
            for (size_t b = 0; b < nb; ++b) {
                for (size_t k = 0; k < nq; ++k) quant[b * nq + k] = hq[k * nb + b];
                if (extra)
                    for (size_t k = 0; k < nxs; ++k) extra[b * nxs + k] = hx[k * nb + b];
            }
            mpcqp_cpu::sweep_max_step_ms(B, hn.data(), ms, quant);
            if (n_steps) std::memcpy(n_steps, hn.data(), nb * 4);
            if (step_ms) fill_step_ms(step_ms);
        } catch (const std::bad_alloc&) {
            return fail(MPC_E_ALLOC, msg("host buffers"));
        }
        return MPC_SUCCESS;
    }
};

#endif  // MPCQP_CLOSED_LOOP_HOST_H
