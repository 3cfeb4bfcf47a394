"""Shared pieces of the warm-start tests (test_warm_cpu.py on the host backend, test_gpu_warm.py on the device): the
case set, a stepwise restatement of mpc_closed_loop_warm, and the comparisons.

The restatement is noise_cases.driver (a Python loop around Solver.solve_batch on the backend under test) handed a
solver that applies the per-step rule of include/mpcqp.h in numpy: it restates the reference warm start from the
state and the slab of every solve_batch call (repeated addition of v * dt, the sticky brake flag, Solver.lookup for
the reference controls), decides the reset, shifts and clamps the plan it kept, passes the result as ubar= and keeps
what came back.  hist_ubar and warmq follow from what it handed over and got back; the other outputs are the driver's
and trace_cases' gaps.  Copy, compare, abs, max and one running sum are exact, so everything is compared bit for bit
(sweep_cases.same).

The cases are trace_cases' (trajectory1, six egos, N = 5 with 24 steps and N = 20 with 30 steps, ego 2 leaves before
step 8 so that egos 4 and 5 move up the solver's list, ego 3 never runs, hist_egos = [4, 1]) with one script
changed: the car of ego 1 is spawned once the ego is 5 m past its start, 20 m further on and at 1 m/s, so the n_obs
the solver is handed changes mid-run and the car gets in the ego's way.  The noisy cases keep perc_sigma at 0 (as
trace_cases' do): the perceived slab is the true one, which hist_slab records."""
import numpy as np

import noise_cases as NC
import sweep_cases as SC
import trace_cases as TR
import traffic_cases as TC

HIST_EGOS = TR.HIST_EGOS
SPAWN_EGO = 1
FREE_EGO = 0                        # its car and light never come within range: n_obs == 0 throughout
NEVER_RAN = 3
NQ = 4
TRACED = TR.NOISY_HISTS + ("hist_pred", "hist_plan")
# the carried variants: (tail, reset) by the names of mpcqp's constants
VARIANTS = {"ref_tail": ("WTAIL_REFERENCE", ()), "ref_tail_nobs": ("WTAIL_REFERENCE", ("WRESET_NOBS",)),
            "ref_tail_all": ("WTAIL_REFERENCE", ("WRESET_NOBS", "WRESET_INFEASIBLE", "WRESET_MAX_ITER")),
            "hold": ("WTAIL_HOLD", ()), "hold_nobs": ("WTAIL_HOLD", ("WRESET_NOBS",)),
            "hold_all": ("WTAIL_HOLD", ("WRESET_NOBS", "WRESET_INFEASIBLE", "WRESET_MAX_ITER"))}


def warm_of(mpcqp, variant):
    """The MpcWarm of a variant name; "reference": the reference warm start every step."""
    if variant == "reference":
        return mpcqp.default_warm()
    tail, bits = VARIANTS[variant]
    reset = 0
    for b in bits:
        reset |= getattr(mpcqp, b)
    return mpcqp.default_warm(mode=mpcqp.WARM_CARRY, tail=getattr(mpcqp, tail), reset=reset)


def case(mpcqp, traj, N, noisy):
    c = TR.case(mpcqp, traj, N, noisy)
    s = c["x_init"][SPAWN_EGO, 0]
    c["scripts"][SPAWN_EGO] = [mpcqp.car(s + 5.0, s + 25.0, 1.0, TC.FAR), c["scripts"][SPAWN_EGO][1]]
    return c


def run_kw(c, N, **more):
    """The keyword arguments of closed_loop_traced / closed_loop_warm for a case, every trace output requested."""
    return TR.run_kw(c, **dict(dict(lookahead=TR.lookaheads(N), preds=True, plans=True), **more))


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
class Carrying:
    """A Solver as noise_cases.driver uses it that hands every solve_batch call the ubar of include/mpcqp.h's
    per-step rule.  n_steps: the number of steps every ego runs, which says who is in the batch of call t."""

    def __init__(self, slv, mpcqp, warm, n_steps, max_steps):
        self.slv, self.mpcqp, self.warm, self.ns = slv, mpcqp, warm, np.asarray(n_steps)
        B, N = self.ns.size, slv.params.N
        self.calls = []
        self.plan = [None] * B                  # the kept U, status and n_obs of every ego
        self.status = [None] * B
        self.nobs = [None] * B
        self.moves = [[] for _ in range(B)]
        self.resets = np.zeros((B, max_steps), bool)      # the steps whose ubar was the reference warm start
        self.hist_ubar = np.full((B, max_steps, N, 2), np.nan)

    @property
    def params(self):
        return self.slv.params

    def lookup(self, s):
        return self.slv.lookup(s)

    def reference(self, xm, pos):
        """ref[k]: the warm start of trajectory_tracking.py:224-246 as the solver computes it without a ubar."""
        p = self.params
        s, v, brake = xm[0], xm[4], False
        at, flags = [], []
        for k in range(p.N):
            if k > 0:
                s = s + v * p.dt
            for o in pos:
                if (o - s) < p.brake_distance:
                    brake = True
            at.append(s)
            flags.append(brake)
        ref = self.lookup(np.array(at))[1].copy()
        ref[np.array(flags), 1] = p.brake_accel
        return ref

    def reset(self, b, n):
        M, w = self.mpcqp, self.warm
        if w.mode != M.WARM_CARRY or self.plan[b] is None or not np.isfinite(self.plan[b]).all():
            return True
        code = int(self.status[b]) & 15
        return (code == 3 or bool(w.reset & M.WRESET_NOBS and n != self.nobs[b]) or
                bool(w.reset & M.WRESET_INFEASIBLE and code == 2) or bool(w.reset & M.WRESET_MAX_ITER and code == 1))

    def ubar(self, b, t, xm, pos):
        p, M = self.params, self.mpcqp
        ref = self.reference(xm, pos)
        if self.reset(b, len(pos)):
            self.resets[b, t] = True
            return ref
        clamped = np.clip(self.plan[b], list(p.u_min), list(p.u_max))
        ub = np.empty_like(ref)
        ub[:-1] = clamped[1:]
        ub[-1] = clamped[-1] if self.warm.tail == M.WTAIL_HOLD else ref[-1]
        return ub

    def solve_batch(self, xm, slab=None, nobs=None):
        t = len(self.calls)
        idx = np.flatnonzero(self.ns > t)
        assert idx.size == xm.shape[0], (t, idx, xm.shape)
        ns = [0] * idx.size if nobs is None else [int(n) for n in nobs]
        ub = np.array([self.ubar(b, t, xm[i], [slab[i, j, 0] for j in range(ns[i])]) for i, b in enumerate(idx)])
        r = self.slv.solve_batch(xm, ubar=ub) if slab is None else self.slv.solve_batch(xm, slab, nobs, ubar=ub)
        for i, b in enumerate(idx):
            self.hist_ubar[b, t] = ub[i]
            self.plan[b], self.status[b], self.nobs[b] = r["U"][i].copy(), r["status"][i], ns[i]
            self.moves[b].append(np.max(np.abs(r["U"][i] - ub[i])))
        self.calls.append(r)
        return r

    def warmq(self):
        out = np.zeros((self.ns.size, NQ))
        for b, mv in enumerate(self.moves):
            if not mv:
                out[b] = (0.0, np.nan, -1.0, 0.0)
                continue
            acc = 0.0
            for m in mv:
                acc = acc + m
            out[b] = (float(self.resets[b].sum()), np.max(mv), float(np.argmax(mv)), acc)
        return out


def restate(env, N, noisy, variant, c=None, lo=0):
    """The restatement of one case under one variant with every ego's history kept: noise_cases.driver's dict plus
    hist_pred, hist_plan, hist_ubar, resets (every ego), gapq and warmq.  The wrapper has to know who is in each batch before
    the loop has run: the step counts start from the reference loop's and are checked against the outcome."""
    mpcqp = env["mpcqp"]
    c = case(mpcqp, env["traj"], N, noisy) if c is None else c
    B, ms = c["x_init"].shape[0], c["max_steps"]
    ns = env["solver"](N).closed_loop_noisy(c["x_init"], **TR.run_kw(c, hist_egos=()))["n_steps"]
    for _ in range(3):
        kept = {}

        def solver(max_obs=0):
            if max_obs not in kept:
                kept[max_obs] = Carrying(env["solver"](N, max_obs), mpcqp, warm_of(mpcqp, variant), ns, ms)
            return kept[max_obs]

        d = NC.driver(dict(env, solver=solver), c["x_init"], 1, 0, np.inf, c["scripts"], c["noise"], TR.SEED, lo, ms,
                      c["s_stop"])
        if np.array_equal(d["n_steps"], ns):
            break
        ns = d["n_steps"]
    else:
        raise AssertionError("the step counts did not settle")
    (keep,) = kept.values()
    pred = np.full((B, ms, N + 1, 5), np.nan)
    plan = np.full((B, ms, N, 2), np.nan)
    for t, r in enumerate(keep.calls):
        idx = np.flatnonzero(ns > t)
        pred[idx, t], plan[idx, t] = r["Xpred"], r["U"]
    assert len(keep.calls) == ns.max()
    d["hist_pred"], d["hist_plan"], d["hist_ubar"] = pred, plan, keep.hist_ubar
    d["gapq"] = TR.gaps(d["hist_x"], pred, ns, TR.lookaheads(N))
    d["warmq"], d["resets"] = keep.warmq(), keep.resets
    return c, d


def runs(env, N, noisy):
    """(case, traced entry, reference restatement) of one case, computed once per backend and shared by the tests.
    What the case is for is asserted here, on the restatement (a failure means the inputs are wrong)."""
    cache = env.setdefault("_warm_runs", {})
    key = (N, noisy)
    if key not in cache:
        c, d = restate(env, N, noisy, "reference")
        ns, ms = d["n_steps"], c["max_steps"]
        assert 0 < ns[2] < 8 and ns[NEVER_RAN] == 0 and (ns[[0, 1, 4, 5]] == ms).all(), ns
        assert (d["hist_nobs"][FREE_EGO, :ms] == 0).all()
        hn = d["hist_nobs"][SPAWN_EGO, :ms]
        assert hn[0] == 1 and (hn[1:] != hn[:-1]).any(), hn          # the car appears at a step t >= 1
        tr = env["solver"](N).closed_loop_traced(c["x_init"], **run_kw(c, N))
        cache[key] = (c, tr, d)
    return cache[key]


def carried(env, N, noisy, variant):
    """(restatement, entry with everything requested) of a carried variant, computed once per backend."""
    cache = env.setdefault("_warm_carried", {})
    key = (N, noisy, variant)
    if key not in cache:
        c, tr, _ = runs(env, N, noisy)
        _, d = restate(env, N, noisy, variant, c)
        w = env["solver"](N).closed_loop_warm(c["x_init"], warm=warm_of(env["mpcqp"], variant), warmq=True, ubars=True,
                                              **run_kw(c, N))
        cache[key] = (d, w)
    return cache[key]


def assert_traced_arrays_equal(a, b):
    """Every array of the traced entry's dict but the wall-clock ones, bit for bit."""
    TR.assert_noisy_arrays_equal(a, b)
    for name in ("gapq", "hist_pred", "hist_plan"):
        assert SC.same(a[name], b[name]), name


# ---------------------------------------------------------------------------------------------
# the shared test bodies
# ---------------------------------------------------------------------------------------------
def check_anchor_off(env, N, noisy):
    """The reference warm start with nothing requested, by warm = None and by the default struct: the traced entry
    on every output."""
    c, tr, _ = runs(env, N, noisy)
    slv, mpcqp = env["solver"](N), env["mpcqp"]
    for warm in (None, mpcqp.default_warm(), mpcqp.default_warm(tail=mpcqp.WTAIL_HOLD, reset=7)):
        off = slv.closed_loop_warm(c["x_init"], warm=warm, **run_kw(c, N))
        assert set(off) == set(tr)
        assert_traced_arrays_equal(off, tr)
        SC.assert_step_time_column(off)
    bare = slv.closed_loop_warm(c["x_init"], **TR.run_kw(c))
    nz = slv.closed_loop_noisy(c["x_init"], **TR.run_kw(c))
    assert set(bare) == set(nz)
    TR.assert_noisy_arrays_equal(bare, nz)


def check_anchor_on(env, N, noisy):
    """The reference warm start handed over as an explicit ubar: every traced output unchanged, a reset at every
    step, and hist_ubar the U that a sqp_iters = 0 solve of the step's hist_xm and hist_slab returns (the solver's own
    warm start; perc_sigma is 0 in these cases, so the perceived slab is hist_slab's)."""
    c, tr, d = runs(env, N, noisy)
    slv = env["solver"](N)
    ms = c["max_steps"]
    on = slv.closed_loop_warm(c["x_init"], warmq=True, ubars=True, **run_kw(c, N))
    assert set(on) == set(tr) | {"warmq", "hist_ubar"}
    assert_traced_arrays_equal(on, tr)
    SC.assert_step_time_column(on)
    ns = on["n_steps"]
    assert on["warmq"].dtype == np.float64 and on["warmq"].shape == (6, NQ)
    assert on["hist_ubar"].dtype == np.float64 and on["hist_ubar"].shape == (2, ms, N, 2)
    assert np.array_equal(on["warmq"][:, 0], ns.astype(np.float64))
    zero = env["solver"](N, 2, sqp_iters=0)
    for k, b in enumerate(HIST_EGOS):
        n = int(ns[b])
        slab = np.nan_to_num(on["hist_slab"][k, :n])
        r = zero.solve_batch(on["hist_xm"][k, :n], slab, on["hist_nobs"][k, :n])
        assert SC.same(on["hist_ubar"][k, :n], r["U"]), (k, b)
        assert np.isnan(on["hist_ubar"][k, n:]).all()
    # each output alone materialises the warm start too
    only_q = slv.closed_loop_warm(c["x_init"], warmq=True, **run_kw(c, N))
    only_u = slv.closed_loop_warm(c["x_init"], ubars=True, **TR.run_kw(c))
    assert SC.same(only_q["warmq"], on["warmq"]) and SC.same(only_u["hist_ubar"], on["hist_ubar"])
    assert_traced_arrays_equal(only_q, tr)
    # and the restatement under WARM_REFERENCE is the entry's
    assert SC.same(on["warmq"], d["warmq"]), (on["warmq"], d["warmq"])
    for k, b in enumerate(HIST_EGOS):
        assert SC.same(on["hist_ubar"][k], d["hist_ubar"][b]), (k, b)


def check_restatement(env, N, noisy, variant):
    c, tr, _ = runs(env, N, noisy)
    d, w = carried(env, N, noisy, variant)
    ms, ns = c["max_steps"], d["n_steps"]
    assert np.array_equal(w["n_steps"], ns)
    assert w["hist_ubar"].shape == (2, ms, N, 2) and w["warmq"].shape == (6, NQ) and w["gapq"].shape == (6, 3, TR.NQ)
    for k, b in enumerate(HIST_EGOS):
        for name in TRACED + ("hist_ubar",):
            assert SC.same(w[name][k].astype(np.float64), d[name][b].astype(np.float64)), (name, b)
        assert np.isnan(w["hist_ubar"][k, ns[b]:]).all() and not np.isnan(w["hist_ubar"][k, :ns[b]]).any()
    assert SC.same(w["quant"][:, NC.QCOLS], d["quant"][:, NC.QCOLS]), (w["quant"], d["quant"])
    assert SC.same(w["extra"], d["extra"]), (w["extra"], d["extra"])
    assert SC.same(w["gapq"], d["gapq"]), (w["gapq"], d["gapq"])
    assert SC.same(w["warmq"], d["warmq"]), (w["warmq"], d["warmq"])
    SC.assert_step_time_column(w)
    # what the case is for: carrying changes what the egos do (a failure means the inputs are wrong)
    assert any(not SC.same(d["hist_u"][b], tr["hist_u"][k]) for k, b in enumerate(HIST_EGOS))


def check_known_answers(env, N, noisy, variant):
    c, _, _ = runs(env, N, noisy)
    mpcqp = env["mpcqp"]
    d, w = carried(env, N, noisy, variant)
    warm = warm_of(mpcqp, variant)
    p = env["solver"](N).params
    ns, q = w["n_steps"], w["warmq"]
    assert SC.same(q[NEVER_RAN], np.array([0.0, np.nan, -1.0, 0.0]))
    ran = ns > 0
    assert (q[ran, 0] >= 1.0).all() and (q[ran, 0] <= ns[ran]).all()
    assert (q[ran, 1] >= 0.0).all() and (q[ran, 3] >= q[ran, 1]).all()
    assert ((0 <= q[ran, 2]) & (q[ran, 2] < ns[ran])).all()
    if warm.reset == 0:
        # no obstacle, no optional reset, finite plans: the first step's reset is the only one
        assert np.isfinite(d["hist_plan"][FREE_EGO, :ns[FREE_EGO]]).all() and q[FREE_EGO, 0] == 1.0
        assert (d["hist_status"][FREE_EGO, :ns[FREE_EGO]] & 15 != 3).all()
    if warm.reset & mpcqp.WRESET_NOBS:
        assert q[SPAWN_EGO, 0] >= 2.0
    lo_, hi_ = np.array(list(p.u_min)), np.array(list(p.u_max))
    for k, b in enumerate(HIST_EGOS):
        n = int(ns[b])
        ub, plan = w["hist_ubar"][k], w["hist_plan"][k]
        # the restatement says which steps started from the reference warm start
        ref_steps = d["resets"][b, :n]
        carried_steps = np.flatnonzero(~ref_steps)
        assert carried_steps.size > 0 and ref_steps[0]
        for t in carried_steps:
            # the clamp is stated: a plan may leave the box by the solver's tolerance
            assert SC.same(ub[t, :N - 1], np.clip(plan[t - 1, 1:], lo_, hi_)), (b, t)
            if warm.tail == mpcqp.WTAIL_HOLD:
                assert SC.same(ub[t, N - 1], np.clip(plan[t - 1, N - 1], lo_, hi_)), (b, t)
        # the move of the kept steps, from the entry's own histories
        mv = np.abs(plan[:n] - ub[:n]).reshape(n, -1).max(axis=1)
        acc = 0.0
        for m in mv:
            acc = acc + m
        assert SC.same(q[b], np.array([float(ref_steps.sum()), mv.max(), float(np.argmax(mv)), acc])), (b, q[b])


def check_composition(env, N, noisy, variant):
    """The six egos as one batch and as two batches of three with ego_offset: the same warm rows, gaps and histories
    for the named egos; another hist_egos choice: warmq unchanged."""
    c, _, _ = runs(env, N, noisy)
    _, whole = carried(env, N, noisy, variant)
    slv = env["solver"](N)
    warm = warm_of(env["mpcqp"], variant)
    for lo, named in ((0, 1), (3, 4)):
        kw = run_kw(c, N, scripts=c["scripts"][lo:lo + 3], noise=c["noise"][lo:lo + 3], hist_egos=[named - lo], lo=lo)
        half = slv.closed_loop_warm(c["x_init"][lo:lo + 3], warm=warm, warmq=True, ubars=True, **kw)
        assert SC.same(half["warmq"], whole["warmq"][lo:lo + 3]), (half["warmq"], whole["warmq"][lo:lo + 3])
        assert SC.same(half["gapq"], whole["gapq"][lo:lo + 3])
        k = HIST_EGOS.index(named)
        for name in TRACED + ("hist_ubar",):
            assert SC.same(half[name][0].astype(np.float64), whole[name][k].astype(np.float64)), (name, named)
    other = slv.closed_loop_warm(c["x_init"], warm=warm, warmq=True, ubars=True, **TR.run_kw(c, hist_egos=[0, 5, 3]))
    assert SC.same(other["warmq"], whole["warmq"]) and np.isnan(other["hist_ubar"][2]).all()
    bare = slv.closed_loop_warm(c["x_init"], warm=warm, **TR.run_kw(c))          # carrying with no warm output
    TR.assert_noisy_arrays_equal(bare, whole)
    assert "warmq" not in bare and "hist_ubar" not in bare


def check_misuse(env, N=5):
    """Every misuse case of include/mpcqp.h is MPC_E_ARG with a message and writes nothing; the well-formed
    neighbours succeed; hist_ubar is NaN past n_steps."""
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"](N)
    L = mpcqp.lib()
    B, A, steps = 6, 2, 10
    c = case(mpcqp, traj, N, True)
    x = np.ascontiguousarray(c["x_init"])
    arr = (mpcqp.MpcActor * (B * A))(*[a for s in c["scripts"] for a in s])
    nzs = (mpcqp.MpcNoise * B)(*c["noise"])
    MARK = -12345.0
    outs = dict(q=np.full((B, 13), MARK), gapq=np.full((B, 2, TR.NQ), MARK), hist_plan=np.full((2, steps, N, 2), MARK),
                warmq=np.full((B, NQ), MARK), hist_ubar=np.full((2, steps, N, 2), MARK))

    def call(h=slv.h, warm=None, n_hist=0, egos=None, look=(1, 3), gapq="gapq", q="q", hist_plan=None, warmq=None,
             hist_ubar=None, n_noise=B):
        he = None if egos is None else np.asarray(egos, np.int32)
        la = np.asarray(look, np.int32)
        o = lambda k: None if k is None else mpcqp._p(outs[k])
        rc = L.mpc_closed_loop_warm(h, B, 1, 0, np.inf, mpcqp._p(x), arr, A, B, nzs, n_noise, 1, 0, steps, TR.S_STOP,
                                    o(q), None, n_hist, mpcqp._pi(he), None, None, None, None, None, None, None, None,
                                    None, None, None, None, mpcqp._pi(la) if la.size else None, la.size, o(gapq), None,
                                    o(hist_plan), None if warm is None else mpcqp.C.byref(warm), o(warmq), o(hist_ubar))
        return rc, mpcqp.last_error()

    W = mpcqp.default_warm
    CARRY = mpcqp.WARM_CARRY
    named = dict(n_hist=2, egos=[4, 1])
    zero = env["solver"](N, 0, sqp_iters=0)
    bad = (dict(warm=W(mode=2)), dict(warm=W(mode=-1)), dict(warm=W(mode=CARRY, tail=2)), dict(warm=W(tail=-1)),
           dict(warm=W(mode=CARRY, reset=8)), dict(warm=W(reset=-1)), dict(warm=W(mode=CARRY, reset=15)),
           dict(n_hist=0, hist_ubar="hist_ubar"), dict(warm=W(mode=CARRY), n_hist=0, hist_ubar="hist_ubar"),
           dict(h=zero.h, warm=W(mode=CARRY)), dict(h=zero.h, warm=W(mode=CARRY), warmq="warmq"),
           # the traced entry's cases reach this entry too
           dict(q=None), dict(look=(0, 3)), dict(gapq=None), dict(n_hist=0, hist_plan="hist_plan"), dict(n_noise=2),
           dict(warmq="warmq", n_hist=2, egos=[1, 1], hist_ubar="hist_ubar"))
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == -1 and msg, kw
        for name, a in outs.items():
            assert (a == MARK).all(), (kw, name)
    assert call()[0] == 0 and call(warm=W())[0] == 0 and call(h=zero.h)[0] == 0
    assert call(h=zero.h, warmq="warmq")[0] == 0                 # the reference warm start returned as it is
    assert (outs["warmq"][[0, 1, 4, 5], 1] == 0.0).all()
    for tail in (mpcqp.WTAIL_REFERENCE, mpcqp.WTAIL_HOLD):
        for reset in range(8):
            assert call(warm=W(mode=CARRY, tail=tail, reset=reset))[0] == 0, (tail, reset)
    assert call(warm=W(mode=CARRY), warmq="warmq", hist_ubar="hist_ubar", hist_plan="hist_plan", **named)[0] == 0
    assert (outs["warmq"] != MARK).all()
    assert not np.isnan(outs["hist_ubar"]).any()                 # egos 4 and 1 run every step
    one = slv.closed_loop_warm(x[2:3], scripts=c["scripts"][2:3], max_steps=steps, s_stop=TR.S_STOP, hist_egos=[0],
                               warm=W(mode=CARRY), warmq=True, ubars=True)
    n2 = int(one["n_steps"][0])
    assert 0 < n2 < steps and np.isnan(one["hist_ubar"][0, n2:]).all() and not np.isnan(one["hist_ubar"][0, :n2]).any()
    r0 = slv.closed_loop_warm(np.empty((0, 5)), max_steps=steps, s_stop=TR.S_STOP, warm=W(mode=CARRY), warmq=True,
                              ubars=True)
    assert r0["warmq"].shape == (0, NQ) and r0["hist_ubar"].shape == (0, steps, N, 2)
    d = mpcqp.default_warm()
    assert (d.mode, d.tail, d.reset) == (mpcqp.WARM_REFERENCE, mpcqp.WTAIL_REFERENCE, 0)
    assert len(mpcqp.WQ_FIELDS) == mpcqp.WQ_NQ == NQ
    assert (mpcqp.WRESET_NOBS, mpcqp.WRESET_INFEASIBLE, mpcqp.WRESET_MAX_ITER) == (1, 2, 4)
