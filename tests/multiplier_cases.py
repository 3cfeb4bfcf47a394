"""Shared pieces of the multiplier tests (test_multipliers_cpu.py on the host backend, test_gpu_multipliers.py on the
device): mpc_multipliers_batch against a longdouble restatement of its definition, against the tool's numpy estimator,
end to end through certify_batch, its independence of the batch, its consistency with the evaluator and the gradient
entry, and the argument contract.

The yardstick.  restate_jac() is gradient_cases.restate()'s dense forward mode with the rows' Jacobian kept (grad and
rows are checked against restate() itself); solve_listed() is the header's definition (the list, the free test, the
normal equations, the Cholesky in list order with the drop rule, the substitutions) in any dtype.  Run in np.longdouble
it is the yardstick, run in float64 it gives the yardstick's own error.  The bound on lam of a group of instances is 16
times the worst float64 error of the yardstick on that group (the gradient tests' rule, gradient_cases.py), relative
to max(1, |lam|inf) per instance.  An instance is compared only when every pivot ratio of the yardstick lies outside
[rank_tol / 100, rank_tol * 100]: inside, float64 and longdouble may decide the drop differently.

What the band may leave out.  The unit is the run, one instance at one steered m: the pivot ratios belong to a solve,
and an instance has up to seven of them.  Per batch at most one run in ten may fall in the band, on the yardstick
alone.  The generated batches meet that by their seeds, which were chosen on the yardstick alone (SEEDS): about one
run in fourteen has near-dependent rows once m reaches the number of free controls (longdouble pivot ratios 6e-10 ..
1e-8), whatever the seed.  The golden cases are fixed, and two of their batches cannot meet it: BAND_EXCEPTIONS names
them with their measured counts, which they may not exceed.  Every batch must compare a run at every steered m it
has.  A run in the band still has everything checked that the drop decision does not touch: the status, N_ACTIVE,
N_FREE, the `active` list, and that lam is zero off the list.

env: dict(mpcqp=module, device=-1 or 0, ptr=callable) as in evaluate_cases.py."""
import ctypes as C

import numpy as np

import gradient_cases as GC

EC = GC.EC
same, solver = GC.same, GC.solver
ACTIVE_TOL, BOUND_TOL, RANK_TOL = 1e-6, 1e-9, 1e-10
OUT_KEYS = ("lam", "active", "summary")
U_MIN, U_MAX = (-0.6, -5.0), (0.6, 4.0)          # checked against the context's parameters in params_bounds()
STEER_M = lambda N: (0, 1, 5, 2 * N - 1, 2 * N, 64, 65)
MAX_LEFT_OUT = 0.1
# golden batches whose runs in the threshold band exceed MAX_LEFT_OUT on the yardstick alone: {name: (band runs, runs)}
BAND_EXCEPTIONS = {"golden-(3, 20, 2)": (6, 42), "golden-(3, 30, 1)": (7, 42)}
# seeds of the generated batches (slab, no obstacles) where the default 7000 + N / 7100 + N puts more than one run in ten
# in the band on the yardstick alone (N = 31: 3 of 21 and 3 of 21; N = 32: 3 of 18 and 2 of 18; N = 63 slab: 3 of 21)
SEEDS = {(31, 8): 8031, (31, 0): 13131, (32, 8): 9032, (32, 0): 8132, (63, 8): 10063}


# ---------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------
def restate_jac(traj, x0, U, obs, dtype, m=None):
    """grad [2N], rows [N,7+M] and the rows' Jacobian in U, jac [N,7+M,2N], of one instance in `dtype`: the dense
    forward mode of gradient_cases.restate()."""
    T = dtype
    m = GC.default_model() if m is None else m
    c = {k: T(v) for k, v in m.items()}
    s64, X64 = GC._table(traj)
    sv, tab = s64.astype(T), X64.astype(T)
    smax = sv[-1]
    N, M = U.shape[0], obs.shape[0]
    nv = 2 * N + 5
    U, obs = U.astype(T), obs.astype(T)

    def look(s):
        if s >= smax:
            return tab[-1], np.zeros(5, T)
        i = min(max(int(np.searchsorted(sv, s)), 1), len(sv) - 1)
        slope = (tab[i] - tab[i - 1]) / (sv[i] - sv[i - 1])
        return slope * (s - sv[i - 1]) + tab[i - 1], slope

    x = np.asarray(x0).astype(T)
    J = np.zeros((5, nv), T)
    J[:, 2 * N:] = np.eye(5, dtype=T)
    gc = np.zeros(nv, T)
    rows = np.full((N, 7 + M), np.nan, T)
    jac = np.zeros((N, 7 + M, 2 * N), T)
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
        s, d, o, _, v = x
        ref, sl = look(s)
        for w, a in ((c["w_d"], 1), (c["w_o"], 2), (c["w_v"], 4)):
            e = x[a] - ref[a]
            gc = gc + 2 * w * e * (J[a] - sl[a] * J[0])
        g = []
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
            jac[k, col] = dg[:2 * N]
    for k in range(N):
        gc[2 * k] += 2 * c["w_u1"] * U[k, 0]
        gc[2 * k + 1] += 2 * c["w_u2"] * U[k, 1]
    return dict(grad=gc[:2 * N], rows=rows, jac=jac)


def list_order(N, rw, n_obs):
    """(stage - 1) * rw + column of every row of the reference's vector, in its order."""
    cols = list(range(6)) + [7 + i for i in range(n_obs)] + [6]
    return np.array([k * rw + c for k in range(N) for c in cols], np.int64)


def solve_listed(R, U, n_obs, active_tol, bound_tol=BOUND_TOL, rank_tol=RANK_TOL, u_min=U_MIN, u_max=U_MAX):
    """The header's definition on restate_jac's result R, in R's dtype: dict(status, n_active, n_free, n_used, active
    (the list), keep [n_active] bool, lam [n_active], ratio [n_active] (d / G[a][a] of every row as it was tested),
    resid)."""
    T = R["grad"].dtype.type
    N, rw = R["rows"].shape
    n2 = 2 * N
    order = list_order(N, rw, n_obs)
    rows, jac = R["rows"].reshape(-1), R["jac"].reshape(-1, n2)
    with np.errstate(invalid="ignore"):
        act = order[rows[order] <= T(active_tol)]
    u = np.asarray(U, np.float64).reshape(-1)
    lo, hi = np.tile(np.array(u_min), N) + bound_tol, np.tile(np.array(u_max), N) - bound_tol
    free = (lo < u) & (u < hi)
    na, nf = len(act), int(free.sum())
    out = dict(n_active=na, n_free=nf, n_used=0, active=act, keep=np.zeros(min(na, 64), bool),
               lam=np.zeros(min(na, 64), T), ratio=np.zeros(0, T), resid=np.nan)
    grad = R["grad"]
    if na > 64:
        return dict(out, status=1, keep=np.zeros(0, bool), lam=np.zeros(0, T))
    if na > 0 and nf == 0:
        return dict(out, status=2)
    Jf, gf = jac[act][:, free], grad[free]
    if not (np.isfinite(gf.astype(np.float64)).all() and np.isfinite(Jf.astype(np.float64)).all()):
        return dict(out, status=3)
    W = Jf @ Jf.T
    r = Jf @ gf
    g0 = np.diag(W).copy()
    keep, ratio, diag = np.zeros(na, bool), np.zeros(na, T), np.ones(na, T)
    for c in range(na):
        d = W[c, c]
        ratio[c] = d / g0[c] if g0[c] != 0 else T(0)
        keep[c] = d > T(rank_tol) * g0[c]
        if not keep[c]:
            continue
        diag[c] = np.sqrt(d)
        r[c] = r[c] / diag[c]
        col = W[c + 1:, c] / diag[c]
        W[c + 1:, c] = col
        r[c + 1:] -= col * r[c]
        W[c + 1:, c + 1:] -= np.outer(col, col)
    lam = np.zeros(na, T)
    for c in range(na - 1, -1, -1):
        if keep[c]:
            lam[c] = r[c] / diag[c]
            r[:c] -= W[c, :c] * lam[c]
    resid = float(np.max(np.abs(gf - lam[keep] @ Jf[keep]))) if nf else 0.0
    return dict(out, status=0, n_used=int(keep.sum()), keep=keep, lam=lam, ratio=ratio, resid=resid)


def steer(rows, n_obs, m):
    """active_tol midway between the m-th and the (m + 1)-th smallest row of the instance (below the smallest for
    m = 0, above the largest when it has exactly m rows); None when it has fewer rows or the two are closer than
    1e-9."""
    N, rw = rows.shape
    v = np.sort(rows.reshape(-1)[list_order(N, rw, n_obs)])
    if not np.isfinite(v).all() or len(v) < m:
        return None
    if m == 0:
        return float(v[0] - 1.0)
    if len(v) == m:
        return float(v[-1] + 1.0)
    return None if v[m] - v[m - 1] < 1e-9 else float(0.5 * (v[m - 1] + v[m]))


def params_bounds(slv):
    p = slv.params
    assert tuple(p.u_min) == U_MIN and tuple(p.u_max) == U_MAX, (tuple(p.u_min), tuple(p.u_max))


def multipliers(slv, w, active_tol=ACTIVE_TOL, **kw):
    return slv.multipliers_batch(w["x0"], w["U"], w["obs"], w["n_obs"], active_tol=active_tol, **kw)


def take(w, idx):
    return {k: (None if a is None else a[idx]) for k, a in w.items()}


# ---------------------------------------------------------------------------------------------
# 1. the yardstick pin
# ---------------------------------------------------------------------------------------------
PIN_N = (1, 2, 15, 16, 31, 32, 63)


def generated_groups():
    """[(name, traj, N, mo, batch)]: B = 3 per horizon, one batch on the 8-wide slab with n_obs mixed over
    {0, 1, 2, 8} and one without obstacles (the other instantiation)."""
    out = []
    for i, N in enumerate(PIN_N):
        w = EC.random_batch(1, N, 3, 8, seed=SEEDS.get((N, 8), 7000 + N), nobs_mode=None)
        # the generator draws controls wider than the bounds: pull two instances inside so that free controls exist
        w["U"][:2] = np.clip(w["U"][:2], np.array(U_MIN) * 0.9, np.array(U_MAX) * 0.9)
        w["n_obs"] = np.array([[8, 1, 0], [2, 0, 8]][i % 2], np.int32)
        out.append((f"gen-N{N}-obs", 1, N, 8, w))
        v = EC.random_batch(1, N, 3, 0, seed=SEEDS.get((N, 0), 7100 + N), nobs_mode=None)
        v["U"][:2] = np.clip(v["U"][:2], np.array(U_MIN) * 0.9, np.array(U_MAX) * 0.9)
        out.append((f"gen-N{N}", 1, N, 0, v))
    return out


def pin_groups():
    """The 60 golden cases by group, then the generated batches: [(name, traj, N, mo, batch)]."""
    out = []
    for key, cs in sorted(EC.golden_groups().items()):
        w = GC.group_inputs(key, cs)
        out.append((f"golden-{key}", key[0], key[1], key[2], dict(x0=w["x0"], U=w["U"], obs=w["obs"], n_obs=w["n_obs"])))
    return out + generated_groups()


_pin_ref = {}


def pin_reference(name, traj, N, mo, w, rows):
    """Per instance of a group and steered m: (m, active_tol, longdouble solve, float64 solve), computed once."""
    if name not in _pin_ref:
        ref = []
        for b in range(w["x0"].shape[0]):
            no = 0 if w["obs"] is None else (mo if w["n_obs"] is None else int(w["n_obs"][b]))
            obs = np.zeros((0, 2)) if w["obs"] is None else w["obs"][b]
            RL = restate_jac(traj, w["x0"][b], w["U"][b], obs, np.longdouble)
            R64 = restate_jac(traj, w["x0"][b], w["U"][b], obs, np.float64)
            per = []
            for m in sorted(set(STEER_M(N))):
                tol = steer(rows[b], no, m)
                if tol is None:
                    continue
                per.append((m, tol, solve_listed(RL, w["U"][b], no, tol), solve_listed(R64, w["U"][b], no, tol)))
            ref.append(per)
        _pin_ref[name] = ref
    return _pin_ref[name]


def rel_lam(a, ref):
    ref = np.asarray(ref)
    if not len(ref):
        return 0.0
    return float(np.max(np.abs(np.asarray(a).astype(ref.dtype) - ref)) / max(1.0, float(np.max(np.abs(ref)))))


def clear_of_threshold(y):
    r = np.asarray(y["ratio"], np.float64)
    return not ((r >= RANK_TOL / 100) & (r <= RANK_TOL * 100)).any()


def check_pin_group(env, group, library=True):
    """One group against the yardstick; returns (compared, left out, worst yardstick float64 error, worst library
    error).  With library=False only the yardstick is run (its float64 form against its longdouble form)."""
    name, traj, N, mo, w = group
    slv = solver(env, traj, N, mo)
    params_bounds(slv)
    rw = 7 + mo
    rows = slv.evaluate_batch(w["x0"], w["U"], w["obs"], w["n_obs"], rows=True)["rows"]
    ref = pin_reference(name, traj, N, mo, w, rows)
    compared, left, y_worst, worst, todo = 0, 0, 0.0, 0.0, []
    seen, kept_m = set(), set()
    for b, per in enumerate(ref):
        for m, tol, yl, y64 in per:
            assert yl["n_active"] == m, (name, b, m, yl["n_active"])
            seen.add(m)
            band = yl["status"] == 0 and not clear_of_threshold(yl)
            todo.append((b, m, tol, yl, band))
            if band:
                left += 1
                continue
            compared += 1
            kept_m.add(m)
            if yl["status"] == 0 and np.array_equal(yl["keep"], y64["keep"]):
                y_worst = max(y_worst, rel_lam(y64["lam"][y64["keep"]], yl["lam"][yl["keep"]]))
    # the yardstick alone: the quota of the band per batch, and no steered m left without a compared run
    assert seen == kept_m, (name, sorted(seen - kept_m))
    if name in BAND_EXCEPTIONS:
        assert (left, compared + left) == BAND_EXCEPTIONS[name], (name, left, compared)
    else:
        assert left <= MAX_LEFT_OUT * (compared + left), (name, left, compared)
    if not library:
        return compared, left, y_worst, 0.0
    bound = 16 * y_worst
    mpcqp = env["mpcqp"]
    for b, m, tol, yl, band in todo:
        r = multipliers(slv, take(w, slice(b, b + 1)), active_tol=tol)
        s, lam, act = r["summary"][0], r["lam"][0].reshape(-1), r["active"][0]
        what = (name, b, m)
        assert int(s[mpcqp.MUQ_STATUS]) == yl["status"], (what, s)
        assert int(s[mpcqp.MUQ_N_ACTIVE]) == m and int(s[mpcqp.MUQ_N_FREE]) == yl["n_free"], (what, s)
        if band:
            # in the band only what the drop decision does not touch
            listed = np.zeros(N * rw, bool)
            listed[yl["active"]] = True
            assert np.array_equal(act[:m], yl["active"]) and (act[m:] == -1).all(), what
            assert (lam[~listed] == 0).all() and 0 < int(s[mpcqp.MUQ_N_USED]) <= min(m, yl["n_free"]), (what, s)
            continue
        assert int(s[mpcqp.MUQ_N_USED]) == yl["n_used"], (what, s, yl["ratio"])
        if m > 64:
            assert int(s[mpcqp.MUQ_STATUS]) == mpcqp.MU_OVERFLOW and (lam == 0).all() and (act == -1).all(), what
            continue
        assert np.array_equal(act[:m], yl["active"]) and (act[m:] == -1).all(), what
        kept = np.zeros(N * rw, bool)
        if yl["status"] == 0:
            kept[yl["active"][yl["keep"]]] = True
        assert (lam[~kept] == 0).all(), what
        if m and yl["status"] == 0:
            # the kept set: a dropped row's lam is exactly 0, a kept one's is compared
            err = rel_lam(lam[yl["active"][yl["keep"]]], yl["lam"][yl["keep"]])
            worst = max(worst, err)
            assert err <= bound, (what, err, bound)
        if N == 20 and m == 64 and yl["status"] == 0:
            nf = int(s[mpcqp.MUQ_N_FREE])
            assert m - int(s[mpcqp.MUQ_N_USED]) >= m - nf and (nf != 40 or m - int(s[mpcqp.MUQ_N_USED]) >= 24), (what, s)
            L = (lam != 0).reshape(N, rw)
            assert not (L[:, 0] & L[:, 1]).any() and not (L[:, 2] & L[:, 3]).any() and not (L[:, 4] & L[:, 5]).any(), what
    print(f"multiplier pin {name}: {compared} compared, {left} left out, yardstick float64 error {y_worst:.3e}, "
          f"library error {worst:.3e} (bound {bound:.3e})")
    return compared, left, y_worst, worst


def check_pin(env, groups, library=True):
    tot = [0, 0, 0.0, 0.0]
    for g in groups:
        c, l, y, w = check_pin_group(env, g, library)
        tot = [tot[0] + c, tot[1] + l, max(tot[2], y), max(tot[3], w)]
    print(f"multiplier pin: {tot[0]} compared, {tot[1]} left out, worst yardstick float64 error {tot[2]:.3e}, worst "
          f"library error {tot[3]:.3e}")
    return tot


# ---------------------------------------------------------------------------------------------
# 2. against the tool's estimator, 3. end to end
# ---------------------------------------------------------------------------------------------
def check_against_estimator(env, case):
    """On the oracle's SQP answers: where the entry kept every active row its lam is the lstsq solution of
    tools/optimality_report.estimate_multipliers, within 16 times the yardstick's float64 error on the compared
    instances."""
    import gradient_params_cases as GP
    from tools.optimality_report import estimate_multipliers
    mpcqp = env["mpcqp"]
    wl, N, name, _ = case
    wb, pset = GP.stationarity_batch(case)
    r = GP.oracle_answer(case)
    t = GP.measure_stationarity(env, case, r)
    slv = solver(env, wb["traj"], wb["N"], wb["max_obs"], **pset)
    params_bounds(slv)
    U = np.ascontiguousarray(np.asarray(r["U"], np.float64).reshape(-1, N, 2))
    w = dict(x0=wb["x0"], U=U, obs=wb["obs"], n_obs=wb["n_obs"])
    got = multipliers(slv, w)
    want, n_active = estimate_multipliers(slv, w["x0"], U, w["obs"], w["n_obs"], ACTIVE_TOL)
    s = got["summary"]
    assert np.array_equal(s[:, mpcqp.MUQ_N_ACTIVE].astype(int), n_active)
    cmp = np.flatnonzero(t["q"] & (s[:, mpcqp.MUQ_STATUS] == 0) & (s[:, mpcqp.MUQ_N_USED] == s[:, mpcqp.MUQ_N_ACTIVE]))
    with_rows = [b for b in cmp if n_active[b] > 0]
    assert len(with_rows) >= 9, (case, len(with_rows))
    y_worst = 0.0
    for b in with_rows:
        no = 0 if w["obs"] is None else int(w["n_obs"][b])
        obs = np.zeros((0, 2)) if w["obs"] is None else w["obs"][b]
        yl = solve_listed(restate_jac(wb["traj"], w["x0"][b], U[b], obs, np.longdouble), U[b], no, ACTIVE_TOL)
        y64 = solve_listed(restate_jac(wb["traj"], w["x0"][b], U[b], obs, np.float64), U[b], no, ACTIVE_TOL)
        if yl["status"] == 0 and np.array_equal(yl["keep"], y64["keep"]):
            y_worst = max(y_worst, rel_lam(y64["lam"][y64["keep"]], yl["lam"][yl["keep"]]))
    bound, worst = 16 * y_worst, 0.0
    for b in cmp:
        err = float(np.max(np.abs(got["lam"][b] - want[b])) / max(1.0, float(np.max(np.abs(want[b])))))
        worst = max(worst, err)
        assert err <= bound, (case, int(b), err, bound)
    print(f"against estimate_multipliers {GP.stationarity_id(case)}: {len(cmp)} compared, {len(with_rows)} with an "
          f"active row, worst {worst:.3e} (bound {bound:.3e})")


def check_certify(env, case):
    """certify_batch on the library's SQP answers: the existing stationarity bound and population conditions."""
    import gradient_params_cases as GP
    mpcqp = env["mpcqp"]
    wl, N, name, _ = case
    wb, pset = GP.stationarity_batch(case)
    r = GP.library_answer(env, case)
    t = GP.measure_stationarity(env, case, r)
    slv = solver(env, wb["traj"], wb["N"], wb["max_obs"], **pset)
    U = np.ascontiguousarray(np.asarray(r["U"], np.float64).reshape(-1, N, 2))
    c = slv.certify_batch(wb["x0"], U, wb["obs"], wb["n_obs"])
    s = c["summary"]
    fig = np.column_stack([s[:, mpcqp.GRQ_PG_INF], s[:, mpcqp.GRQ_COMPL], -s[:, mpcqp.GRQ_MIN_LAM]])
    t = dict(t, fig=fig, active=c["multipliers"][:, mpcqp.MUQ_N_ACTIVE] > 0)
    GP.check_stationarity_population(case, t)
    bound = GP.STATIONARITY_BOUND[case[2]]
    print(f"certify {GP.stationarity_id(case)}: worst " +
          ", ".join(f"{n} {g:.3e} (bound {b:.3e})" for n, g, b in zip(GP.FIGURES, GP.worst_figures(t), bound)))
    for b in np.flatnonzero(t["q"]):
        assert (fig[b] <= bound).all(), (case, int(b), fig[b], bound)


def check_tracker_certify(env):
    """TrajectoryTracker.certify_batch (obstacle lists of mixed length, an obstacle array, no obstacles) equals
    Solver.certify_batch on the slab it builds, under ==."""
    import trajectory_tracking as TT
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    N, B = 10, 6
    mpc = TT.TrajectoryTracker(TrajectoryLoader(builtin_trajectory(2)), device=env["device"])
    mpc.N = N
    w = EC.random_batch(2, N, B, 2, seed=181)
    w["U"][:4] = np.clip(w["U"][:4], np.array(U_MIN) * 0.9, np.array(U_MAX) * 0.9)
    w["n_obs"][:3] = [2, 0, 1]
    lists = [[dict(s=float(w["obs"][b, i, 0]), v=float(w["obs"][b, i, 1])) for i in range(int(w["n_obs"][b]))]
             for b in range(B)]
    slab = np.zeros_like(w["obs"])
    for b in range(B):
        slab[b, :w["n_obs"][b]] = w["obs"][b, :w["n_obs"][b]]
    runs = [(lists, solver(env, 2, N, 2), slab, w["n_obs"]),
            (w["obs"], solver(env, 2, N, 2), w["obs"], np.full(B, 2, np.int32)),
            (None, solver(env, 2, N, 0), None, None)]
    for obstacles, slv, obs, n_obs in runs:
        got = mpc.certify_batch(w["x0"], w["U"], obstacles)
        want = slv.certify_batch(w["x0"], w["U"], obs, n_obs)
        for k in want:
            assert same(got[k], want[k]), k
        assert same(got["n_obs"], np.zeros(B, np.int32) if n_obs is None else n_obs), (got["n_obs"], n_obs)
        assert (got["multipliers"][:, 0] == 0).any()


# ---------------------------------------------------------------------------------------------
# 4. bit identity and independence
# ---------------------------------------------------------------------------------------------
SHAPE_N = (1, 15, 16, 31, 32, 63)
SHAPE_MO = (0, 3)
SHAPE_B = 5


def shape_batch(N, mo):
    w = EC.random_batch(1, N, SHAPE_B, mo, seed=2500 * N + mo, nobs_mode=None)
    w["U"][:3] = np.clip(w["U"][:3], np.array(U_MIN) * 0.9, np.array(U_MAX) * 0.9)
    if mo:
        w["n_obs"] = np.array([3, 0, 1, 3, 1], np.int32)
    return w


def shape_kinds(summary):
    """Which kinds of list a summary holds: 'empty', 'full' (every active row kept), 'dropped' (N_USED < N_ACTIVE on
    an OK instance), 'overflow'."""
    st, na, nu = summary[:, 0].astype(int), summary[:, 1].astype(int), summary[:, 3].astype(int)
    k = set()
    if ((st == 0) & (na == 0)).any():
        k.add("empty")
    if ((st == 0) & (na > 0) & (nu == na)).any():
        k.add("full")
    if ((st == 0) & (nu < na)).any():
        k.add("dropped")
    if (st == 1).any():
        k.add("overflow")
    return k


def shape_tols(slv, w):
    """active_tol values for this batch: the default; above 10%, 40% and all of its rows (rank-deficient and
    overflowing lists); just above the 1st, 3rd and 8th smallest row of the batch (short lists, kept whole)."""
    rows = slv.evaluate_batch(w["x0"], w["U"], w["obs"], w["n_obs"], rows=True)["rows"]
    v = np.sort(rows[np.isfinite(rows)])
    return [ACTIVE_TOL] + [float(v[min(len(v) - 1, int(q * len(v)))]) + 1e-7 for q in (0.1, 0.4, 1.0)] + \
        [float(v[min(len(v) - 1, i)]) + 1e-7 for i in (0, 2, 7)]


def raw_multipliers(env, slv, w, want, B=None, tols=(ACTIVE_TOL, BOUND_TOL, RANK_TOL)):
    """mpc_multipliers_batch through ctypes with only the outputs named in `want`; returns (rc, outputs)."""
    mpcqp = env["mpcqp"]
    p = slv.params
    B = w["x0"].shape[0] if B is None else B
    nb = max(B, 0)
    out = {}
    if "lam" in want:
        out["lam"] = np.full((nb, p.N, 7 + p.max_obs), -7.0)
    if "active" in want:
        out["active"] = np.full((nb, mpcqp.MAX_ACTIVE), -7, np.int32)
    if "summary" in want:
        out["summary"] = np.full((nb, mpcqp.MU_NQ), -7.0)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    oi = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))
    rc = mpcqp.lib().mpc_multipliers_batch(slv.h, B, dp(w["x0"]), dp(w["obs"]), ip(w["n_obs"]), dp(w["U"]), *tols,
                                           dp(out.get("lam")), oi(out.get("active")), dp(out.get("summary")))
    return rc, out


def check_independence(env):
    """The same bits for B = 1, for the batch permuted and for each output alone; a NaN stays in its instance; every
    control on a bound is MPC_MU_NO_FREE."""
    mpcqp = env["mpcqp"]
    N, mo, B = 20, 3, 9
    slv = solver(env, 2, N, mo)
    w = EC.random_batch(2, N, B, mo, seed=151)
    w["U"][:6] = np.clip(w["U"][:6], np.array(U_MIN) * 0.9, np.array(U_MAX) * 0.9)
    tol = shape_tols(slv, w)[1]
    tols = (tol, BOUND_TOL, RANK_TOL)
    rc, full = raw_multipliers(env, slv, w, OUT_KEYS, tols=tols)
    assert rc == 0 and not any((full[k] == -7).all() for k in OUT_KEYS)
    assert (full["summary"][:, mpcqp.MUQ_N_ACTIVE] > 0).sum() >= 5 and (full["lam"] != 0).any()
    for b in range(B):
        rc, one = raw_multipliers(env, slv, take(w, slice(b, b + 1)), OUT_KEYS, tols=tols)
        assert rc == 0
        for k in OUT_KEYS:
            assert same(one[k][0], full[k][b]), (b, k)
    perm = np.random.default_rng(153).permutation(B)
    rc, pr = raw_multipliers(env, slv, take(w, perm), OUT_KEYS, tols=tols)
    assert rc == 0
    for k in OUT_KEYS:
        assert same(pr[k], full[k][perm]), k
    for k in OUT_KEYS:
        rc, out = raw_multipliers(env, slv, w, (k,), tols=tols)
        assert rc == 0 and same(out[k], full[k]), k
    # a NaN in x0, U or obs of one instance
    v = {k: (None if a is None else a.copy()) for k, a in w.items()}
    v["x0"][1, 1] = np.nan
    v["U"][4, N // 2, 1] = np.nan
    v["obs"][0, 0, 0] = np.nan                      # instance 0 uses all three obstacles
    rc, rn = raw_multipliers(env, slv, v, OUT_KEYS, tols=tols)
    assert rc == 0
    hit = np.zeros(B, bool)
    hit[[0, 1, 4]] = True
    for k in OUT_KEYS:
        assert same(rn[k][~hit], full[k][~hit]), k
    for b in np.flatnonzero(hit):
        s = rn["summary"][b]
        assert int(s[mpcqp.MUQ_STATUS]) == mpcqp.MU_NONFINITE or int(s[mpcqp.MUQ_N_ACTIVE]) == 0, (b, s)
        assert (rn["lam"][b] == 0).all(), b
    # every control on a bound
    z = {k: (None if a is None else a.copy()) for k, a in w.items()}
    z["U"][2] = np.where(np.arange(N)[:, None] % 2 == 0, np.array(U_MIN), np.array(U_MAX))
    rc, rz = raw_multipliers(env, slv, z, OUT_KEYS, tols=(1e3, BOUND_TOL, RANK_TOL))
    assert rc == 0
    s = rz["summary"][2]
    assert int(s[mpcqp.MUQ_STATUS]) in (mpcqp.MU_NO_FREE, mpcqp.MU_OVERFLOW) and int(s[mpcqp.MUQ_N_FREE]) == 0, s
    rc, rz = raw_multipliers(env, slv, take(z, slice(2, 3)), OUT_KEYS, tols=(steer_first(slv, z, 2), BOUND_TOL, RANK_TOL))
    s = rz["summary"][0]
    assert rc == 0 and int(s[mpcqp.MUQ_STATUS]) == mpcqp.MU_NO_FREE and int(s[mpcqp.MUQ_N_ACTIVE]) == 3, s
    assert (rz["lam"] == 0).all() and np.isnan(s[mpcqp.MUQ_RESID]) and np.isnan(s[mpcqp.MUQ_MIN_PIVOT])


def steer_first(slv, w, b, m=3):
    one = take(w, slice(b, b + 1))
    rows = slv.evaluate_batch(one["x0"], one["U"], one["obs"], one["n_obs"], rows=True)["rows"][0]
    no = 0 if one["obs"] is None else int(one["n_obs"][0])
    tol = steer(rows, no, m)
    assert tol is not None
    return tol


# ---------------------------------------------------------------------------------------------
# 5. consistency with the siblings
# ---------------------------------------------------------------------------------------------
def check_siblings(env):
    """`active` is evaluate_batch(rows=True) <= active_tol in the reference's order, and RESID is reproduced under ==
    from the returned lam and the unit-lam jtl of gradient_batch, with the sums in the header's order."""
    mpcqp = env["mpcqp"]
    N, mo, B = 16, 3, 7
    slv = solver(env, 2, N, mo)
    rw = 7 + mo
    w = EC.random_batch(2, N, B, mo, seed=161)
    w["U"][:5] = np.clip(w["U"][:5], np.array(U_MIN) * 0.9, np.array(U_MAX) * 0.9)
    rows = slv.evaluate_batch(w["x0"], w["U"], w["obs"], w["n_obs"], rows=True)["rows"]
    grad = slv.gradient_batch(w["x0"], w["U"], w["obs"], w["n_obs"])["grad"].reshape(B, 2 * N)
    seen = 0
    for tol in shape_tols(slv, w)[:3]:
        r = multipliers(slv, w, active_tol=tol)
        for b in range(B):
            no = int(w["n_obs"][b])
            order = list_order(N, rw, no)
            with np.errstate(invalid="ignore"):
                act = order[rows[b].reshape(-1)[order] <= tol]
            s = r["summary"][b]
            assert int(s[mpcqp.MUQ_N_ACTIVE]) == len(act), (b, s)
            if len(act) > 64:
                assert (r["active"][b] == -1).all()
                continue
            assert np.array_equal(r["active"][b, :len(act)], act) and (r["active"][b, len(act):] == -1).all(), b
            if int(s[mpcqp.MUQ_STATUS]) != 0:
                continue
            u = w["U"][b].reshape(-1)
            free = (np.tile(np.array(U_MIN), N) + BOUND_TOL < u) & (u < np.tile(np.array(U_MAX), N) - BOUND_TOL)
            assert int(s[mpcqp.MUQ_N_FREE]) == int(free.sum())
            lam = r["lam"][b].reshape(-1)
            resid = 0.0
            if len(act):
                unit = np.zeros((len(act), N * rw))
                unit[np.arange(len(act)), act] = 1.0
                rep = lambda a: None if a is None else np.repeat(a[b:b + 1], len(act), axis=0)
                ja = slv.gradient_batch(rep(w["x0"]), rep(w["U"]), rep(w["obs"]), rep(w["n_obs"]),
                                        lam=unit.reshape(-1, N, rw))["jtl"].reshape(len(act), 2 * N)
                seen += 1
            kept = [a for a in range(len(act)) if lam[act[a]] != 0.0]
            assert len(kept) <= int(s[mpcqp.MUQ_N_USED])
            for i in np.flatnonzero(free):
                acc = 0.0
                for a in kept:
                    acc = acc + lam[act[a]] * ja[a, i]
                resid = max(resid, abs(grad[b, i] - acc))
            if len(kept) == int(s[mpcqp.MUQ_N_USED]):          # no kept row with lam exactly 0
                assert resid == s[mpcqp.MUQ_RESID], (b, tol, resid, s)
    assert seen >= 6


# ---------------------------------------------------------------------------------------------
# 6. the argument contract
# ---------------------------------------------------------------------------------------------
def check_contract(env):
    mpcqp = env["mpcqp"]
    N, mo, B = 10, 2, 6
    slv = solver(env, 2, N, mo)
    w = EC.random_batch(2, N, B, mo, seed=171)

    def refused(rc, word):
        assert rc == -1 and word in mpcqp.last_error(), (rc, word, mpcqp.last_error())

    assert raw_multipliers(env, slv, w, OUT_KEYS)[0] == 0
    refused(raw_multipliers(env, slv, dict(w, U=None), OUT_KEYS)[0], "U is NULL")
    nan = float("nan")
    refused(raw_multipliers(env, slv, w, OUT_KEYS, tols=(nan, BOUND_TOL, RANK_TOL))[0], "active_tol")
    refused(raw_multipliers(env, slv, w, OUT_KEYS, tols=(ACTIVE_TOL, -1e-9, RANK_TOL))[0], "bound_tol")
    refused(raw_multipliers(env, slv, w, OUT_KEYS, tols=(ACTIVE_TOL, nan, RANK_TOL))[0], "bound_tol")
    refused(raw_multipliers(env, slv, w, OUT_KEYS, tols=(ACTIVE_TOL, BOUND_TOL, -1.0))[0], "rank_tol")
    refused(raw_multipliers(env, slv, w, OUT_KEYS, tols=(ACTIVE_TOL, BOUND_TOL, nan))[0], "rank_tol")
    assert raw_multipliers(env, slv, w, OUT_KEYS, tols=(-0.5, 0.0, 0.0))[0] == 0          # a negative active_tol is fine
    with np.testing.assert_raises(ValueError):
        slv.multipliers_batch(w["x0"], None)
    s0 = solver(env, 2, N, 0)
    refused(raw_multipliers(env, s0, w, ("summary",))[0], "max_obs == 0")
    assert raw_multipliers(env, slv, w, OUT_KEYS, B=0)[0] == 0
    assert raw_multipliers(env, slv, w, ())[0] == 0
    # the device entry: n_obs without obs, misaligned double arrays
    keep = []

    def ptr(a, off=0):
        if a is None:
            return None
        addr, k = env["ptr"](a)
        keep.append(k)
        return addr + off

    L = mpcqp.lib()
    x0p, Up, op, np_ = ptr(w["x0"]), ptr(w["U"]), ptr(w["obs"]), ptr(w["n_obs"])
    lp, ap, sp = ptr(np.zeros((B, N, 7 + mo))), ptr(np.zeros((B, 64), np.int32)), ptr(np.zeros((B, mpcqp.MU_NQ)))
    call = lambda x, o, n, u, l, a, s: L.mpc_multipliers_batch_device(slv.h, B, x, o, n, u, ACTIVE_TOL, BOUND_TOL,
                                                                      RANK_TOL, l, a, s, None)
    assert call(x0p, op, np_, Up, lp, ap, sp) == 0
    refused(call(x0p, None, np_, Up, lp, ap, sp), "n_obs given but obs is NULL")
    for args in ((x0p + 4, op, np_, Up, lp, ap, sp), (x0p, op + 4, np_, Up, lp, ap, sp), (x0p, op, np_, Up + 4, lp, ap, sp),
                 (x0p, op, np_, Up, lp + 4, ap, sp), (x0p, op, np_, Up, lp, ap, sp + 4)):
        refused(call(*args), "aligned")
    refused(call(x0p, op, np_, None, lp, ap, sp), "U is NULL")
    assert call(x0p, op, np_, Up, None, None, None) == 0
    assert L.mpc_multipliers_batch_device(slv.h, 0, None, None, None, None, ACTIVE_TOL, BOUND_TOL, RANK_TOL, None, None,
                                          None, None) == 0
    env.get("sync", lambda: None)()          # the buffers in `keep` outlive the asynchronous call
