"""Shared pieces of the gradient tests (test_gradient_cpu.py on the host backend, test_gpu_gradient.py on the device):
mpc_gradient_batch against an independent forward-mode restatement of the reference's predict / cost / constraints,
against central differences through the public evaluator, its summary against numpy on the returned arrays, its
independence of the batch, and the argument contract.

Tolerance of the restatement pin (RESTATE_BOUND).  restate() below, run in float64, was compared with itself run in
np.longdouble (x87 80-bit) on the 60 model_golden cases with the seeded lam of golden_lam(), per case and per output
(grad, gx0, jtl) as max |f64 - longdouble| / max(1, max |longdouble|):
    measured worst  1.071e-13, kept as RESTATE_F64_WORST = 1.08e-13 (test_restatement_error_budget re-measures it
                    and holds it to that)
    chosen bound    RESTATE_BOUND = 16 * RESTATE_F64_WORST = 1.73e-12
16x because the library adds in another order (one reverse sweep) than the restatement (dense forward mode).

env: dict(mpcqp=module, device=-1 or 0, ptr=callable) as in evaluate_cases.py."""
import ctypes as C
import warnings

import numpy as np

import evaluate_cases as EC
from conftest import traj_arrays

RESTATE_F64_WORST = 1.08e-13
RESTATE_BOUND = 16 * RESTATE_F64_WORST

same = EC.same
solver = EC.solver
close_solvers = EC.close_solvers
OUT_KEYS = ("grad", "jtl", "gx0", "costate", "summary")


def default_model():
    """The reference's model parameters (TrajectoryTracker.__init__), which the golden cases were recorded under."""
    return dict(dt=0.2, w_d=10.0, w_o=10.0, w_v=5.0, w_u1=0.5, w_u2=0.5, osd=5.0, tgap=1.5, L=2.8,
                sl=3.0 / 2.0 - 1.0 - 0.1)


# ---------------------------------------------------------------------------------------------
# the restatement: dense forward mode through the Euler steps, in any dtype
# ---------------------------------------------------------------------------------------------
_tables = {}


def _table(traj):
    """(s with the loader's strict-monotone fix, X) of a bundled trajectory, float64."""
    if traj not in _tables:
        X, _ = traj_arrays(traj)
        s = X[:, 0].copy()
        for i in range(1, len(s)):
            if s[i] <= s[i - 1]:
                s[i] = s[i - 1] + 1e-5
        _tables[traj] = (s, X)
    return _tables[traj]


def restate(traj, x0, U, obs, lam, dtype, m=None):
    """cost, d cost / d U [N,2], d cost / d x0 [5], J' lam [N,2] and the rows [N,7+M] of one instance, written from
    the reference's dynamics / predict / cost / constraints: every state carries its dense Jacobian in (U, x0)
    through the Euler steps; the table's values and slopes come from the trajectory arrays by np.searchsorted.
    obs [M,2]; lam [N,7+M] in the layout of `rows`.  Also X [N+1,5], the rollout."""
    T = dtype
    m = default_model() if m is None else m
    c = {k: T(v) for k, v in m.items()}
    s64, X64 = _table(traj)
    sv, tab = s64.astype(T), X64.astype(T)
    smax = sv[-1]
    N, M = U.shape[0], obs.shape[0]
    nv = 2 * N + 5
    U, obs, lam = U.astype(T), obs.astype(T), lam.astype(T)

    def look(s):
        if s >= smax:
            return tab[-1], np.zeros(5, T)
        i = min(max(int(np.searchsorted(sv, s)), 1), len(sv) - 1)
        slope = (tab[i] - tab[i - 1]) / (sv[i] - sv[i - 1])
        return slope * (s - sv[i - 1]) + tab[i - 1], slope

    x = np.asarray(x0).astype(T)
    Xs = [x]
    J = np.zeros((5, nv), T)
    J[:, 2 * N:] = np.eye(5, dtype=T)
    cost, gc, jt = T(0), np.zeros(nv, T), np.zeros(nv, T)
    rows = np.zeros((N, 7 + M), T)
    for k in range(N):
        ref, sl = look(x[0])
        _, d, o, kk, v = x
        xd = np.array([v, v * o, v * (kk - ref[3]), U[k, 0], U[k, 1]], T)
        Jd = np.zeros((5, nv), T)
        Jd[0] = J[4]
        Jd[1] = J[4] * o + v * J[2]
        Jd[2] = J[4] * (kk - ref[3]) + v * (J[3] - sl[3] * J[0])
        Jd[3, 2 * k] = 1
        Jd[4, 2 * k + 1] = 1
        x = x + c["dt"] * xd
        J = J + c["dt"] * Jd
        Xs.append(x)
        s, d, o, _, v = x
        ref, sl = look(s)
        for w, a in ((c["w_d"], 1), (c["w_o"], 2), (c["w_v"], 4)):
            e = x[a] - ref[a]
            cost = cost + w * e ** 2
            gc = gc + 2 * w * e * (J[a] - sl[a] * J[0])
        g = []                                           # (column, value, gradient)
        for i, a in enumerate((T(0), c["L"] / 2, c["L"])):
            e, de = d + a * o, J[1] + a * J[2]
            g += [(2 * i, c["sl"] - e, -de), (2 * i + 1, e + c["sl"], de)]
        for i in range(M):
            gap = v * c["tgap"] > c["osd"]
            safe = v * c["tgap"] if gap else c["osd"]
            g.append((7 + i, obs[i, 0] + obs[i, 1] * ((k + 1) * c["dt"]) - s - safe,
                      -J[0] - (c["tgap"] * J[4] if gap else 0 * J[4])))
        g.append((6, v, J[4]))
        for col, val, dg in g:
            rows[k, col] = val
            jt = jt + lam[k, col] * dg
    for k in range(N):
        cost = cost + c["w_u1"] * U[k, 0] ** 2 + c["w_u2"] * U[k, 1] ** 2
        gc[2 * k] += 2 * c["w_u1"] * U[k, 0]
        gc[2 * k + 1] += 2 * c["w_u2"] * U[k, 1]
    return dict(cost=cost, grad=gc[:2 * N].reshape(N, 2), gx0=gc[2 * N:], jtl=jt[:2 * N].reshape(N, 2), rows=rows,
                X=np.array(Xs))


def rel_err(a, ref):
    """max |a - ref| relative to max(1, max |ref|), in ref's precision."""
    ref = np.asarray(ref)
    return float(np.max(np.abs(np.asarray(a).astype(ref.dtype) - ref)) / max(1.0, float(np.max(np.abs(ref)))))


# ---------------------------------------------------------------------------------------------
# the 60 golden cases
# ---------------------------------------------------------------------------------------------
def golden_lam(N, no, B, key):
    """Seeded random row weights >= 0 of a golden group, [B,N,7+no]."""
    return np.random.default_rng(10000 * key[0] + 100 * key[1] + key[2]).uniform(0.0, 2.0, (B, N, 7 + no))


def group_inputs(key, cs):
    ti, N, no = key
    x0 = np.array([c["x0"] for c in cs])
    U = np.array([c["U"].reshape(N, 2) for c in cs])
    obs = np.array([c["obs"] for c in cs]).reshape(len(cs), no, 2) if no else None
    n_obs = np.full(len(cs), no, np.int32) if no else None
    return dict(x0=x0, U=U, obs=obs, n_obs=n_obs, lam=golden_lam(N, no, len(cs), key))


def gradient_golden(env):
    """[(key, cases, inputs, gradient result, evaluator result)] of the golden groups on env's device, once."""
    cache = env.setdefault("_grad_golden", {})
    if env["device"] not in cache:
        out = []
        for key, cs in sorted(EC.golden_groups().items()):
            ti, N, no = key
            slv = solver(env, ti, N, no)
            w = group_inputs(key, cs)
            r = slv.gradient_batch(w["x0"], w["U"], w["obs"], w["n_obs"], lam=w["lam"], costate=True)
            e = slv.evaluate_batch(w["x0"], w["U"], w["obs"], w["n_obs"], rows=True)
            for v in list(r.values()) + list(e.values()):
                v.setflags(write=False)
            out.append((key, cs, w, r, e))
        cache[env["device"]] = out
    return cache[env["device"]]


_yardstick = {}


def yardstick():
    """restate() in np.longdouble on the 60 cases: {(key, b): result}, computed once."""
    if not _yardstick:
        for key, cs in sorted(EC.golden_groups().items()):
            w = group_inputs(key, cs)
            for b in range(len(cs)):
                obs = np.zeros((0, 2)) if w["obs"] is None else w["obs"][b]
                _yardstick[(key, b)] = restate(key[0], w["x0"][b], w["U"][b], obs, w["lam"][b], np.longdouble)
    return _yardstick


def measure_restatement_error():
    """The worst error of restate() in float64 against the yardstick over the cases and (grad, gx0, jtl)."""
    worst = 0.0
    for key, cs in sorted(EC.golden_groups().items()):
        w = group_inputs(key, cs)
        for b in range(len(cs)):
            obs = np.zeros((0, 2)) if w["obs"] is None else w["obs"][b]
            r64 = restate(key[0], w["x0"][b], w["U"][b], obs, w["lam"][b], np.float64)
            ref = yardstick()[(key, b)]
            worst = max([worst] + [rel_err(r64[k], ref[k]) for k in ("grad", "gx0", "jtl")])
    return worst


def check_restatement_pin(env):
    """grad, gx0 and jtl of the library against the longdouble yardstick on all 60 cases within RESTATE_BOUND, and
    costate[N-1] against q_N formed from the evaluator's Xpred and the table."""
    n, worst = 0, 0.0
    m = default_model()
    for key, cs, w, r, e in gradient_golden(env):
        ti, N, no = key
        sv, X = _table(ti)
        for b in range(len(cs)):
            ref = yardstick()[(key, b)]
            for k in ("grad", "gx0", "jtl"):
                err = rel_err(r[k][b], ref[k])
                worst = max(worst, err)
                assert err <= RESTATE_BOUND, (key, b, k, err)
            s, d, o, _, v = e["Xpred"][b, N]
            if s >= sv[-1]:
                st, sl = X[-1], np.zeros(5)
            else:
                i = min(max(int(np.searchsorted(sv, s)), 1), len(sv) - 1)
                sl = (X[i] - X[i - 1]) / (sv[i] - sv[i - 1])
                st = sl * (s - sv[i - 1]) + X[i - 1]
            gd, go, gv = 2 * m["w_d"] * (d - st[1]), 2 * m["w_o"] * (o - st[2]), 2 * m["w_v"] * (v - st[4])
            qN = np.array([-(gd * sl[1] + go * sl[2] + gv * sl[4]), gd, go, 0.0, gv])
            assert rel_err(r["costate"][b, N - 1], qN) <= RESTATE_BOUND, (key, b, r["costate"][b, N - 1], qN)
            n += 1
    assert n == 60
    print(f"restatement pin: worst error {worst:.3e} (bound {RESTATE_BOUND:.3e})")


def check_cost_bits(env):
    n = 0
    for key, cs, w, r, e in gradient_golden(env):
        assert same(r["summary"][:, 0], e["summary"][:, 0]), key
        for b, c in enumerate(cs):
            assert r["summary"][b, 0] == float(c["cost"]), (key, b)
            n += 1
    assert n == 60


# ---------------------------------------------------------------------------------------------
# 2. central differences through the public evaluator
# ---------------------------------------------------------------------------------------------
FD_H = 1e-5
FD_REL = 1e-6
FD_DIRS = 3
KNOT_MARGIN = 1e-3


def smooth_case(ti, Xpred, m):
    """The evaluator is differentiable around this rollout: every s_k is more than KNOT_MARGIN from a table knot and
    the safe distance is more than KNOT_MARGIN from its kink at every stage."""
    sv, _ = _table(ti)
    s = Xpred[:, 0]
    knot = np.min(np.abs(s[:, None] - sv[None, :]), axis=1)
    kink = np.abs(Xpred[1:, 4] * m["tgap"] - m["osd"])
    return bool((knot > KNOT_MARGIN).all() and (kink > KNOT_MARGIN).all())


def check_finite_differences(env, groups=None, m=None, what="", **kw):
    """(cost(U + hV) - cost(U - hV)) / 2h against grad . V, and per row family the same for one row of the evaluator's
    `rows` against jtl . V with lam the unit vector of that row, for FD_DIRS random unit directions per case: on the
    60 golden cases under the default parameters, or on the `groups` (in gradient_golden's format) recorded under the
    model m, through contexts with the mpc_params fields kw.  Returns (cases used, cases, trajectories, cases used
    with 8 obstacles); the default run asserts its own counts."""
    default = groups is None
    groups = gradient_golden(env) if default else groups
    m = default_model() if m is None else m
    used, total, trajs, with8 = 0, 0, set(), 0
    worst = 0.0
    for key, cs, w, r, e in groups:
        ti, N, no = key
        slv = solver(env, ti, N, no, **kw)
        total += len(cs)
        ok = [b for b in range(len(cs)) if smooth_case(ti, e["Xpred"][b], m)]
        if not ok:
            continue
        used += len(ok)
        trajs.add(ti)
        with8 += len(ok) if no == 8 else 0
        rng = np.random.default_rng(1000 * ti + 10 * N + no)
        nb = len(ok)
        V = rng.normal(size=(nb, FD_DIRS, N, 2))
        V /= np.sqrt((V ** 2).sum(axis=(2, 3), keepdims=True))
        # one unit lam per row family and instance: (stage, column)
        fams = [("lane", lambda: int(rng.integers(0, 6))), ("v", lambda: 6)]
        if no:
            fams.append(("obs", lambda: 7 + int(rng.integers(0, no))))
        picks = [[(int(rng.integers(0, N)), col()) for _, col in fams] for _ in range(nb)]
        rep = lambda a, k: None if a is None else np.repeat(a[ok], k, axis=0)
        lam = np.zeros((nb, len(fams), N, 7 + no))
        for i in range(nb):
            for f, (k, col) in enumerate(picks[i]):
                lam[i, f, k, col] = 1.0
        rl = slv.gradient_batch(rep(w["x0"], len(fams)), rep(w["U"], len(fams)), rep(w["obs"], len(fams)),
                                rep(w["n_obs"], len(fams)), lam=lam.reshape(-1, N, 7 + no))
        jtl = rl["jtl"].reshape(nb, len(fams), N, 2)
        U0 = w["U"][ok][:, None]
        ev = {}
        for sgn in (1.0, -1.0):
            Us = (U0 + sgn * FD_H * V).reshape(-1, N, 2)
            ev[sgn] = slv.evaluate_batch(rep(w["x0"], FD_DIRS), Us, rep(w["obs"], FD_DIRS), rep(w["n_obs"], FD_DIRS),
                                         rows=True)
        dcost = ((ev[1.0]["summary"][:, 0] - ev[-1.0]["summary"][:, 0]) / (2 * FD_H)).reshape(nb, FD_DIRS)
        drows = ((ev[1.0]["rows"] - ev[-1.0]["rows"]) / (2 * FD_H)).reshape(nb, FD_DIRS, N, 7 + no)
        for i, b in enumerate(ok):
            for j in range(FD_DIRS):
                want = float((r["grad"][b] * V[i, j]).sum())
                err = abs(dcost[i, j] - want) / max(1.0, abs(want))
                worst = max(worst, err)
                assert err <= FD_REL, (key, b, j, "cost", dcost[i, j], want)
                for f, (k, col) in enumerate(picks[i]):
                    want = float((jtl[i, f] * V[i, j]).sum())
                    err = abs(drows[i, j, k, col] - want) / max(1.0, abs(want))
                    worst = max(worst, err)
                    assert err <= FD_REL, (key, b, j, fams[f][0], k, col, drows[i, j, k, col], want)
    print(f"finite differences{what}: {used} of {total} cases, worst error {worst:.3e} (bound {FD_REL:.1e})")
    if default:
        assert used >= 50 and trajs == {1, 2, 3} and with8 >= 1, (used, trajs, with8)
    return used, total, trajs, with8


# ---------------------------------------------------------------------------------------------
# 4. summary against numpy on the returned arrays
# ---------------------------------------------------------------------------------------------
def numpy_summary(grad, jtl, U, lam, rows, n_obs, u_min, u_max):
    """Columns 1..5 of the summary restated on the returned arrays of one instance (lam, jtl None without lam)."""
    q = np.full(6, np.nan)
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore")
        r = grad if lam is None else grad - jtl
        q[1] = np.max(np.abs(grad))
        q[2] = np.max(np.abs(r))
        q[3] = np.max(np.abs(np.clip(U - r, np.asarray(u_min), np.asarray(u_max)) - U))
        if lam is not None:
            w = 7 + n_obs
            q[4] = np.max(np.abs(lam[:, :w] * rows[:, :w]))
            q[5] = np.min(lam[:, :w])
    return q


def check_summary(slv, w, r, what=""):
    """Every instance of a gradient_batch result r for the inputs w against numpy_summary."""
    p = slv.params
    e = slv.evaluate_batch(w["x0"], w["U"], w["obs"], w["n_obs"], rows=True)
    mo = e["rows"].shape[2] - 7
    for b in range(w["x0"].shape[0]):
        no = 0 if w["obs"] is None else (mo if w["n_obs"] is None else int(min(max(int(w["n_obs"][b]), 0), mo)))
        lam = None if w.get("lam") is None else w["lam"][b]
        q = numpy_summary(r["grad"][b], None if lam is None else r["jtl"][b], w["U"][b], lam, e["rows"][b], no,
                          list(p.u_min), list(p.u_max))
        assert same(r["summary"][b, 1:], q[1:]), (what, b, r["summary"][b], q)
        assert same(r["summary"][b, 0], e["summary"][b, 0]), (what, b)


def gradient(slv, w, costate=True, **kw):
    w = dict(w, **kw)
    return slv.gradient_batch(w["x0"], w["U"], w["obs"], w["n_obs"], lam=w.get("lam"), costate=costate)


def lam_batch(w, mo, seed):
    """The batch with seeded random lam >= 0 [B,N,7+mo] added."""
    B, N = w["U"].shape[:2]
    return dict(w, lam=np.random.default_rng(seed).uniform(0.0, 2.0, (B, N, 7 + mo)))


def check_golden_summary(env):
    for key, cs, w, r, e in gradient_golden(env):
        check_summary(solver(env, *key), w, r, key)


def check_summary_cases(env):
    """The summary under NaN inputs, lam past n_obs, lam = 0, no lam; and the linearity of jtl in lam."""
    N, mo, B = 10, 2, 7
    slv = solver(env, 2, N, mo)
    w = lam_batch(EC.random_batch(2, N, B, mo, seed=41), mo, 42)
    w["n_obs"][:] = [2, 0, 1, 2, 1, 0, 2]
    base = gradient(slv, w)
    check_summary(slv, w, base, "base")
    assert (base["summary"][:, 3] > 0).all() and np.isfinite(base["summary"]).all()
    # without lam
    r0 = gradient(slv, dict(w, lam=None))
    assert "jtl" not in r0 and same(r0["grad"], base["grad"]) and same(r0["costate"], base["costate"])
    assert same(r0["summary"][:, 2], r0["summary"][:, 1]) and np.isnan(r0["summary"][:, 4:]).all()
    check_summary(slv, dict(w, lam=None), r0, "no lam")
    # lam = 0
    rz = gradient(slv, dict(w, lam=np.zeros_like(w["lam"])))
    assert (rz["jtl"] == 0).all() and same(rz["summary"][:, 2], rz["summary"][:, 1])
    assert (rz["summary"][:, 4] == 0).all() and (rz["summary"][:, 5] == 0).all()
    # NaN past n_obs is never read
    lp = w["lam"].copy()
    for b in range(B):
        lp[b, :, 7 + int(w["n_obs"][b]):] = np.nan
    assert np.isnan(lp).any()
    rp = gradient(slv, dict(w, lam=lp))
    for k in OUT_KEYS:
        assert same(rp[k], base[k]), k
    # a NaN control and a NaN lam inside the read columns stay in their instances
    v = dict(w, U=w["U"].copy(), lam=w["lam"].copy())
    v["U"][1, N // 2, 1] = np.nan
    v["lam"][4, 3, 7] = np.nan                 # instance 4 has one obstacle: column 7 is read
    v["lam"][5, 2, 6] = np.nan
    rn = gradient(slv, v)
    keep = np.ones(B, bool)
    keep[[1, 4, 5]] = False
    for k in OUT_KEYS:
        assert same(rn[k][keep], base[k][keep]), k
    assert np.isnan(rn["summary"][1, :4]).all() and np.isnan(rn["grad"][1]).any()
    for b in (4, 5):
        assert same(rn["grad"][b], base["grad"][b]) and same(rn["summary"][b, :2], base["summary"][b, :2])
        assert np.isnan(rn["jtl"][b]).any() and np.isnan(rn["summary"][b, 2:]).all()
    check_summary(slv, v, rn, "nan")
    # linearity of jtl in lam, at the bound of the restatement pin
    l2 = np.random.default_rng(43).uniform(0.0, 2.0, w["lam"].shape)
    a = 0.375
    j1, j2 = base["jtl"], gradient(slv, dict(w, lam=l2))["jtl"]
    j3 = gradient(slv, dict(w, lam=a * w["lam"] + l2))["jtl"]
    for b in range(B):
        assert rel_err(j3[b], a * j1[b] + j2[b]) <= RESTATE_BOUND, b


# ---------------------------------------------------------------------------------------------
# 5. independence of the batch and of the outputs asked for
# ---------------------------------------------------------------------------------------------
def raw_gradient(env, slv, w, want, B=None):
    """mpc_gradient_batch through ctypes with only the outputs named in `want`; returns (rc, outputs)."""
    mpcqp = env["mpcqp"]
    p = slv.params
    B = w["x0"].shape[0] if B is None else B
    nb = max(B, 0)
    shapes = dict(grad=(nb, p.N, 2), jtl=(nb, p.N, 2), gx0=(nb, 5), costate=(nb, p.N, 5), summary=(nb, mpcqp.GR_NQ))
    out = {k: np.full(shapes[k], -7.0) for k in want}
    dp = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    rc = mpcqp.lib().mpc_gradient_batch(slv.h, B, dp(w["x0"]), dp(w["obs"]), ip(w["n_obs"]), dp(w["U"]),
                                        dp(w.get("lam")), *(dp(out.get(k)) for k in OUT_KEYS))
    return rc, out


def check_independence(env):
    """The same bits for B = 1, for the batch permuted, and for each output asked for alone."""
    N, mo, B = 20, 3, 9
    slv = solver(env, 2, N, mo)
    w = lam_batch(EC.random_batch(2, N, B, mo, seed=51), mo, 52)
    rc, full = raw_gradient(env, slv, w, OUT_KEYS)
    assert rc == 0 and not any((full[k] == -7.0).all() for k in OUT_KEYS)
    take = lambda idx: {k: (None if a is None else a[idx]) for k, a in w.items()}
    for b in range(B):
        rc, one = raw_gradient(env, slv, take(slice(b, b + 1)), OUT_KEYS)
        assert rc == 0
        for k in OUT_KEYS:
            assert same(one[k][0], full[k][b]), (b, k)
    perm = np.random.default_rng(53).permutation(B)
    rc, pr = raw_gradient(env, slv, take(perm), OUT_KEYS)
    assert rc == 0
    for k in OUT_KEYS:
        assert same(pr[k], full[k][perm]), k
    for k in OUT_KEYS:
        rc, out = raw_gradient(env, slv, w, (k,))
        assert rc == 0, (k, env["mpcqp"].last_error())
        assert same(out[k], full[k]), k


# ---------------------------------------------------------------------------------------------
# 6. the argument contract
# ---------------------------------------------------------------------------------------------
def check_contract(env):
    mpcqp = env["mpcqp"]
    N, mo, B = 10, 2, 6
    slv = solver(env, 2, N, mo)
    w = lam_batch(EC.random_batch(2, N, B, mo, seed=61), mo, 62)

    def refused(rc):
        assert rc == -1 and len(mpcqp.last_error()) > 0, (rc, mpcqp.last_error())

    assert raw_gradient(env, slv, w, OUT_KEYS)[0] == 0
    refused(raw_gradient(env, slv, dict(w, U=None), OUT_KEYS)[0])
    refused(raw_gradient(env, slv, dict(w, x0=None), OUT_KEYS, B=B)[0])
    refused(raw_gradient(env, slv, w, OUT_KEYS, B=-1)[0])
    refused(raw_gradient(env, slv, dict(w, lam=None), ("grad", "jtl"))[0])
    assert raw_gradient(env, slv, dict(w, lam=None), ("grad", "gx0", "costate", "summary"))[0] == 0
    with np.testing.assert_raises(ValueError):
        slv.gradient_batch(w["x0"], None)
    s0 = solver(env, 2, N, 0)
    refused(raw_gradient(env, s0, dict(w, lam=None), ("summary",))[0])          # obs with max_obs == 0
    with np.testing.assert_raises(ValueError):
        s0.gradient_batch(w["x0"], w["U"], w["obs"], w["n_obs"])
    # B == 0 succeeds; all outputs NULL launches nothing and succeeds
    assert raw_gradient(env, slv, w, OUT_KEYS, B=0)[0] == 0
    assert raw_gradient(env, slv, w, ())[0] == 0
    # n_obs outside [0, max_obs] is clamped like mpc_evaluate_batch, NULL means all rows
    wild = np.array([5, -3, 2, 0, 1, 99], np.int32)
    a, b = gradient(slv, w, n_obs=wild), gradient(slv, w, n_obs=np.clip(wild, 0, mo))
    full, none = gradient(slv, w, n_obs=np.full(B, mo, np.int32)), gradient(slv, w, n_obs=None)
    for k in OUT_KEYS:
        assert same(a[k], b[k]) and same(full[k], none[k]), k
    # the device entry: misaligned double arrays, n_obs without obs, jtl without lam
    keep = []

    def ptr(a, off=0):
        if a is None:
            return None
        addr, k = env["ptr"](a)
        keep.append(k)
        return addr + off

    L = mpcqp.lib()
    x0p, Up, op, np_, lp = ptr(w["x0"]), ptr(w["U"]), ptr(w["obs"]), ptr(w["n_obs"]), ptr(w["lam"])
    gp, jp, sp = ptr(np.zeros((B, N, 2))), ptr(np.zeros((B, N, 2))), ptr(np.zeros((B, mpcqp.GR_NQ)))
    call = lambda *a: L.mpc_gradient_batch_device(slv.h, B, *a, None)
    assert call(x0p, op, np_, Up, lp, gp, jp, None, None, sp) == 0
    for args in ((x0p + 4, op, np_, Up, lp, gp, jp, None, None, sp), (x0p, op + 4, np_, Up, lp, gp, jp, None, None, sp),
                 (x0p, op, np_, Up + 4, lp, gp, jp, None, None, sp), (x0p, op, np_, Up, lp + 4, gp, jp, None, None, sp),
                 (x0p, op, np_, Up, lp, gp + 4, jp, None, None, sp), (x0p, op, np_, Up, lp, gp, jp + 4, None, None, sp),
                 (x0p, op, np_, Up, lp, gp, jp, None, None, sp + 4), (x0p, op, np_, Up, lp, gp, jp, 4, None, sp),
                 (x0p, op, np_, Up, lp, gp, jp, None, 4, sp), (x0p, None, np_, Up, lp, gp, jp, None, None, sp),
                 (x0p, op, np_, None, lp, gp, jp, None, None, sp), (x0p, op, np_, Up, None, gp, jp, None, None, sp)):
        refused(call(*args))
    assert call(x0p, op, np_, Up, lp, None, None, None, None, None) == 0
    assert L.mpc_gradient_batch_device(slv.h, 0, *([None] * 11)) == 0
    env.get("sync", lambda: None)()          # the buffers in `keep` outlive the asynchronous call


# ---------------------------------------------------------------------------------------------
# 7. the shapes of the GPU == host test
# ---------------------------------------------------------------------------------------------
SHAPE_N = (1, 5, 15, 16, 31, 32, 63)
SHAPE_MO = (0, 3)
SHAPE_B = 5


def shape_runs(N, mo):
    """(what, batch) of one (N, max_obs) on trajectory 1: evaluate_cases' generator (instance 3 rolls past s_max)
    with seeded lam; n_obs mixed over {0, 1, 3} and NULL; without lam."""
    w = lam_batch(EC.random_batch(1, N, SHAPE_B, mo, seed=2000 * N + mo, nobs_mode=None), mo, 3000 * N + mo)
    if mo:
        yield "mixed", dict(w, n_obs=np.array([3, 0, 1, 3, 1], np.int32))
    yield "null", w
    yield "no lam", dict(w, lam=None)
