"""Shared pieces of the plan-trace tests (test_trace_cpu.py on the host backend, test_gpu_trace.py on the device):
the case set, a stepwise restatement of mpc_closed_loop_traced, and the comparisons.

The restatement is noise_cases.driver (a Python loop around Solver.solve_batch on the backend under test) handed a
solver that keeps what every solve_batch call returned: its U and Xpred per step are the expected hist_plan and
hist_pred, and the gap columns are computed afterwards in numpy from the restatement's own hist_x and the kept
predictions.  Subtraction, abs and max are exact, so everything is compared bit for bit (sweep_cases.same).

Trajectory1 (300 m), starts from S0 = 40 m and s_stop 200 m further on, two horizons: N = 5 with 24 steps and
N = 20 with 30 steps, so that lookahead N has pairs after the first list compaction (step 7).  Six egos with the start-state pattern of
tools/record_closed_loop_entries.py (offsets of 9 m and 6 m, v = 9 and 8, small lateral offsets), arranged so that
  ego 0  runs to the cap with a script whose car and light never come within range,
  ego 2  starts 4 m before s_stop and leaves before step 8: egos 4 and 5 move up in the solver's list,
  ego 3  starts past s_stop and never runs,
and hist_egos = [4, 1]: out of order, and ego 4 sits behind the one that leaves."""
import numpy as np

import convoy_cases as CC
import noise_cases as NC
import sweep_cases as SC
import traffic_cases as TC

S0 = 40.0
S_STOP = S0 + 200.0
HORIZONS = {5: 24, 20: 30}          # N -> max_steps
HIST_EGOS = [4, 1]
SEED = 2024
NOISY_HISTS = NC.HISTS              # every history the noisy entry has
NQ = 5


def lookaheads(N):
    return [1, 3, N]


def case(mpcqp, traj, N, noisy):
    """dict(x_init, scripts, noise (one per ego), max_steps, s_stop) of horizon N, with every sigma 0 or with the
    measurement, actuation and process sigmas of noise_cases' per-ego case (mild at twice its scale)."""
    ego = CC.ego
    x = np.array([ego(traj, S0), ego(traj, S0 + 9.0, d=0.01), ego(traj, S_STOP - 4.0), ego(traj, S_STOP + 2.0),
                  ego(traj, S0, v=8.0), ego(traj, S0 + 6.0, v=8.0)])
    script = lambda s, k: [mpcqp.car(S0 - 1.0 + 3.0 * k, s + 25.0 + k, 4.0 - 0.25 * k, TC.FAR),
                           mpcqp.light(S0 + 30.0 + 2.0 * k, 100.0, 0.6 + 0.2 * k)]
    scripts = [script(s, k) for k, s in enumerate(x[:, 0])]
    scripts[0] = [mpcqp.car(TC.FAR, TC.FAR, 4.0, 2.0 * TC.FAR), mpcqp.light(TC.FAR, 100.0, 1.0)]
    one = NC.mild(mpcqp, 2.0)
    make = (lambda: mpcqp.default_noise(meas_sigma=list(one.meas_sigma), act_sigma=list(one.act_sigma),
                                        proc_sigma=list(one.proc_sigma))) if noisy else mpcqp.default_noise
    return dict(x_init=x, scripts=scripts, noise=[make() for _ in range(6)], max_steps=HORIZONS[N], s_stop=S_STOP)


def run_kw(c, **more):
    """The keyword arguments of closed_loop_noisy / closed_loop_traced for a case."""
    return dict(dict(scripts=c["scripts"], max_steps=c["max_steps"], s_stop=c["s_stop"], noise=c["noise"], seed=SEED,
                     hist_egos=HIST_EGOS), **more)


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
class Keeping:
    """A Solver as noise_cases.driver uses it, keeping the result of every solve_batch call."""

    def __init__(self, slv):
        self.slv, self.calls = slv, []

    @property
    def params(self):
        return self.slv.params

    def lookup(self, s):
        return self.slv.lookup(s)

    def solve_batch(self, *args):
        r = self.slv.solve_batch(*args)
        self.calls.append(r)
        return r


def gaps(hist_x, pred, n_steps, look):
    """gapq [B, n_look, 5] from every ego's full hist_x [B, max_steps + 1, 5] and predictions
    [B, max_steps, N + 1, 5]: the definition of include/mpcqp.h, in numpy."""
    B = n_steps.size
    out = np.zeros((B, len(look), NQ))
    for b in range(B):
        for i, j in enumerate(look):
            n = max(0, int(n_steps[b]) - j + 1)
            if n == 0:
                out[b, i] = (0.0, np.nan, np.nan, np.nan, -1.0)
                continue
            t = np.arange(n)
            D = np.abs(pred[b, t, j][:, [0, 1, 4]] - hist_x[b, t + j][:, [0, 1, 4]])
            out[b, i] = (float(n), D[:, 0].max(), D[:, 1].max(), D[:, 2].max(), float(np.argmax(D[:, 1])))
    return out


def restate(env, N, noisy, lo=0):
    """The restatement of one case with every ego's history kept: noise_cases.driver's dict plus hist_pred, hist_plan
    (every ego) and gapq."""
    c = case(env["mpcqp"], env["traj"], N, noisy)
    kept = {}

    def solver(max_obs=0):
        if max_obs not in kept:
            kept[max_obs] = Keeping(env["solver"](N, max_obs))
        return kept[max_obs]

    d = NC.driver(dict(env, solver=solver), c["x_init"], 1, 0, np.inf, c["scripts"], c["noise"], SEED, lo, c["max_steps"],
                  c["s_stop"])
    (keep,) = kept.values()
    ns, ms = d["n_steps"], c["max_steps"]
    pred = np.full((6, ms, N + 1, 5), np.nan)
    plan = np.full((6, ms, N, 2), np.nan)
    for t, r in enumerate(keep.calls):
        idx = np.flatnonzero(ns > t)                      # the egos in the loop at step t, in the driver's order
        assert r["U"].shape[0] == idx.size
        pred[idx, t], plan[idx, t] = r["Xpred"], r["U"]
    assert len(keep.calls) == ns.max()
    d["hist_pred"], d["hist_plan"] = pred, plan
    d["gapq"] = gaps(d["hist_x"], pred, ns, lookaheads(N))
    # what the case is for (a failure here means the inputs are wrong)
    assert 0 < ns[2] < 8 and ns[3] == 0 and (ns[[0, 1, 4, 5]] == ms).all(), ns
    assert (d["hist_nobs"][0, :ms] == 0).all() and d["hist_nobs"][1, 0] == 2
    return c, d


def runs(env, N, noisy):
    """(case, restatement, noisy entry, traced entry with everything requested) of one case, computed once per
    backend and shared by the tests."""
    cache = env.setdefault("_runs", {})
    key = (N, noisy)
    if key not in cache:
        c, d = restate(env, N, noisy)
        slv = env["solver"](N)
        nz = slv.closed_loop_noisy(c["x_init"], **run_kw(c))
        tr = slv.closed_loop_traced(c["x_init"], lookahead=lookaheads(N), preds=True, plans=True, **run_kw(c))
        cache[key] = (c, d, nz, tr)
    return cache[key]


def assert_noisy_arrays_equal(a, b):
    """Every array of the noisy entry's dict but the wall-clock ones, bit for bit."""
    assert np.array_equal(a["n_steps"], b["n_steps"]) and np.array_equal(a["hist_egos"], b["hist_egos"])
    assert SC.same(a["quant"][:, NC.QCOLS], b["quant"][:, NC.QCOLS]) and SC.same(a["quant"][:, 0], b["quant"][:, 0])
    assert SC.same(a["extra"], b["extra"])
    for name in NOISY_HISTS:
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, name
        assert SC.same(a[name].astype(np.float64), b[name].astype(np.float64)), name


# ---------------------------------------------------------------------------------------------
# the shared test bodies
# ---------------------------------------------------------------------------------------------
def check_anchor_off(env, N, noisy):
    """Nothing requested: the noisy entry, on every array."""
    c, _, nz, _ = runs(env, N, noisy)
    off = env["solver"](N).closed_loop_traced(c["x_init"], **run_kw(c))
    assert set(off) == set(nz)
    assert_noisy_arrays_equal(off, nz)
    SC.assert_step_time_column(off)


def check_anchor_on(env, N, noisy):
    """Everything requested: what the noisy entry has is still the noisy entry's."""
    _, _, nz, tr = runs(env, N, noisy)
    assert set(tr) == set(nz) | {"gapq", "hist_pred", "hist_plan"}
    assert_noisy_arrays_equal(tr, nz)
    SC.assert_step_time_column(tr)


def check_restatement(env, N, noisy):
    c, d, _, tr = runs(env, N, noisy)
    ms, ns = c["max_steps"], d["n_steps"]
    assert np.array_equal(tr["n_steps"], ns)
    assert tr["hist_pred"].dtype == np.float64 and tr["hist_pred"].shape == (2, ms, N + 1, 5)
    assert tr["hist_plan"].dtype == np.float64 and tr["hist_plan"].shape == (2, ms, N, 2)
    assert tr["gapq"].dtype == np.float64 and tr["gapq"].shape == (6, 3, NQ)
    for k, b in enumerate(HIST_EGOS):
        assert SC.same(tr["hist_pred"][k], d["hist_pred"][b]), (k, b)
        assert SC.same(tr["hist_plan"][k], d["hist_plan"][b]), (k, b)
        assert np.isnan(tr["hist_pred"][k, ns[b]:]).all() and not np.isnan(tr["hist_pred"][k, :ns[b]]).any()
        # the plan's first control is the commanded one, and the prediction starts from what the solver was given
        assert SC.same(tr["hist_plan"][k, :, 0], tr["hist_u"][k])
        assert SC.same(tr["hist_pred"][k, :, 0], tr["hist_xm"][k])
        if not noisy:
            assert SC.same(tr["hist_pred"][k, :ns[b], 0], tr["hist_x"][k, :ns[b]])
        else:
            assert not SC.same(tr["hist_pred"][k, :ns[b], 0], tr["hist_x"][k, :ns[b]])
    assert SC.same(tr["gapq"], d["gapq"]), (tr["gapq"], d["gapq"])
    # the restatement's other outputs are the entry's too (the noisy entry's own test, on this case set)
    for name in NOISY_HISTS:
        for k, b in enumerate(HIST_EGOS):
            assert SC.same(tr[name][k].astype(np.float64), d[name][b].astype(np.float64)), (name, b)


def check_known_answers(env, N, noisy):
    c, d, _, tr = runs(env, N, noisy)
    g, ns = tr["gapq"], tr["n_steps"]
    for i, j in enumerate(lookaheads(N)):
        assert np.array_equal(g[:, i, 0], np.maximum(0, ns - j + 1).astype(np.float64)), j
    assert SC.same(g[3], np.tile([0.0, np.nan, np.nan, np.nan, -1.0], (3, 1)))          # the ego that never ran
    assert g[2, 0, 0] == ns[2] and g[2, 2, 0] == max(0, ns[2] - N + 1)                  # the one that left early
    ran = ns > 0
    for b in range(6):
        for i, j in enumerate(lookaheads(N)):                     # the step of MAX_DD is one of the compared steps
            assert (0 <= g[b, i, 4] <= ns[b] - j) if ns[b] >= j else g[b, i, 4] == -1.0, (b, j)
    if not noisy:
        # predict's first stage and the plant's Euler step are the same arithmetic (loop_steps.h's plant_step
        # against predict_grp), on the same state and control: lookahead 1 of an ego that is never handed an actor
        assert g[0, 0, 1:4].tolist() == [0.0, 0.0, 0.0] and g[0, 0, 4] == 0.0
        # an actor inside the horizon does not change that: the pair is one model step either way
        assert (g[ran, 0, 1:4] == 0.0).all()
    else:
        assert (g[ran, 0, 1] > 0.0).all(), g[:, 0]


def assert_gap_rows(a, rows_a, b, rows_b):
    assert SC.same(a["gapq"][rows_a], b["gapq"][rows_b]), (a["gapq"][rows_a], b["gapq"][rows_b])


def check_composition(env, N, noisy):
    """The six egos as one batch and as two batches of three with ego_offset: the same gapq rows, the same
    histories for the named egos; another hist_egos choice: gapq unchanged."""
    c, _, _, whole = runs(env, N, noisy)
    slv = env["solver"](N)
    look = lookaheads(N)
    for lo, named in ((0, 1), (3, 4)):
        kw = run_kw(c, scripts=c["scripts"][lo:lo + 3], noise=c["noise"][lo:lo + 3], hist_egos=[named - lo], lo=lo)
        half = slv.closed_loop_traced(c["x_init"][lo:lo + 3], lookahead=look, preds=True, plans=True, **kw)
        assert_gap_rows(half, slice(0, 3), whole, slice(lo, lo + 3))
        k = HIST_EGOS.index(named)
        for name in NOISY_HISTS + ("hist_pred", "hist_plan"):
            assert SC.same(half[name][0].astype(np.float64), whole[name][k].astype(np.float64)), (name, named)
    other = slv.closed_loop_traced(c["x_init"], lookahead=look, preds=True, **run_kw(c, hist_egos=[0, 5, 3]))
    assert_gap_rows(other, slice(0, 6), whole, slice(0, 6))
    assert np.isnan(other["hist_pred"][2]).all()                  # the ego that never ran
    gaps_only = slv.closed_loop_traced(c["x_init"], lookahead=look, **run_kw(c, hist_egos=()))
    assert_gap_rows(gaps_only, slice(0, 6), whole, slice(0, 6))
    assert set(gaps_only) == set(whole) - {"hist_pred", "hist_plan"}
    # the lookaheads in another order and one alone: the rows follow
    swapped = slv.closed_loop_traced(c["x_init"], lookahead=look[::-1], **run_kw(c, hist_egos=()))
    assert SC.same(swapped["gapq"][:, ::-1], whole["gapq"])
    alone = slv.closed_loop_traced(c["x_init"], lookahead=[3], plans=True, **run_kw(c))
    assert SC.same(alone["gapq"][:, 0], whole["gapq"][:, 1]) and SC.same(alone["hist_plan"], whole["hist_plan"])


def check_misuse(env, N=5):
    """Every misuse case of include/mpcqp.h is MPC_E_ARG with a message and writes nothing; the well-formed
    neighbours succeed."""
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"](N)
    L = mpcqp.lib()
    assert L.mpc_version() == 5
    B, A, steps = 6, 2, 10
    c = case(mpcqp, traj, N, True)
    x = np.ascontiguousarray(c["x_init"])
    arr = (mpcqp.MpcActor * (B * A))(*[a for s in c["scripts"] for a in s])
    nzs = (mpcqp.MpcNoise * B)(*c["noise"])
    MARK = -12345.0
    outs = dict(q=np.full((B, 13), MARK), gapq=np.full((B, 4, NQ), MARK), hist_pred=np.full((2, steps, N + 1, 5), MARK),
                hist_plan=np.full((2, steps, N, 2), MARK), hist_x=np.full((2, steps + 1, 5), MARK))

    def call(B=B, K=0, actors=arr, A=A, n_scripts=B, noise=nzs, n_noise=B, ego_offset=0, q="q", n_hist=0, egos=None,
             hist_x=None, look=(1, 3), n_look=None, look_null=False, gapq="gapq", hist_pred=None, hist_plan=None):
        he = None if egos is None else np.asarray(egos, np.int32)
        la = np.asarray(look, np.int32)
        n_look = la.size if n_look is None else n_look
        o = lambda k: None if k is None else mpcqp._p(outs[k])
        rc = L.mpc_closed_loop_traced(slv.h, B, 1, K, np.inf, mpcqp._p(x), actors, A, n_scripts, noise, n_noise, 1,
                                      ego_offset, steps, S_STOP, o(q), None, n_hist, mpcqp._pi(he), o(hist_x), None,
                                      None, None, None, None, None, None, None, None, None, None,
                                      None if look_null or la.size == 0 else mpcqp._pi(la), n_look, o(gapq),
                                      o(hist_pred), o(hist_plan))
        return rc, mpcqp.last_error()

    bad = (mpcqp.MpcActor * (B * A))(*arr)
    bad[3].kind = 3
    neg = (mpcqp.MpcNoise * B)(*c["noise"])
    neg[2].meas_sigma[1] = -1.0
    named = dict(n_hist=2, egos=[4, 1])
    noisy_cases = (dict(A=-1), dict(A=17), dict(n_scripts=2), dict(actors=None, n_scripts=B), dict(actors=bad),
                   dict(q=None), dict(n_hist=-1), dict(n_hist=0, hist_x="hist_x"), dict(K=-1), dict(K=15),
                   dict(n_hist=2, egos=[1, B], hist_x="hist_x"), dict(n_hist=2, egos=[1, 1], hist_x="hist_x"),
                   dict(noise=neg), dict(n_noise=2), dict(noise=None, n_noise=1), dict(ego_offset=-1))
    trace_cases = (dict(n_look=-1), dict(look=(1, 2, 3, 4, 5), gapq="gapq"), dict(n_look=5),
                   dict(look=(0, 3)), dict(look=(1, N + 1)), dict(look=(-2,)), dict(look=(3, 1, 3)), dict(look=(2, 2)),
                   dict(gapq=None), dict(look=(), gapq="gapq"), dict(look_null=True),
                   dict(n_hist=0, hist_pred="hist_pred"), dict(n_hist=0, hist_plan="hist_plan"),
                   dict(look=(), gapq=None, n_hist=0, hist_pred="hist_pred"))
    for kw in noisy_cases + trace_cases:
        rc, msg = call(**kw)
        assert rc == -1 and msg, kw
        for name, a in outs.items():
            assert (a == MARK).all(), (kw, name)
    flat = outs["gapq"].ravel()                                   # two lookaheads: [B][2][NQ] of the buffer
    assert call()[0] == 0 and (flat[:B * 2 * NQ] != MARK).all() and (flat[B * 2 * NQ:] == MARK).all()
    assert call(look=(), gapq=None)[0] == 0 and call(look=(N,))[0] == 0 and call(look=(4, 3, 2, 1))[0] == 0
    assert call(look=(), gapq=None, hist_pred="hist_pred", hist_plan="hist_plan", hist_x="hist_x", **named)[0] == 0
    assert call(hist_pred="hist_pred", **named)[0] == 0 and call(hist_plan="hist_plan", **named)[0] == 0
    assert call(B=0, actors=None, A=0, n_scripts=0, noise=None, n_noise=0)[0] == 0
    r0 = slv.closed_loop_traced(np.empty((0, 5)), max_steps=steps, s_stop=S_STOP, lookahead=[1, 2], preds=True, plans=True)
    assert r0["gapq"].shape == (0, 2, NQ) and r0["hist_pred"].shape == (0, steps, N + 1, 5)
    assert r0["hist_plan"].shape == (0, steps, N, 2)
    assert len(mpcqp.TG_FIELDS) == mpcqp.TG_NQ == NQ and mpcqp.MAX_LOOK == 4
