"""Shared pieces of the gradient tests away from the goldens (test_gradient_cpu.py on the host backend,
test_gpu_gradient.py on the device): mpc_gradient_batch under the parameter sets of tests/golden/params_golden.npz, at
the lane-group boundary horizons with several wavefronts and the 64-row slab, and the first-order optimality of the
solver's answers.  The yardstick is gradient_cases.restate() in np.longdouble, with its model taken from mpc_params
(model_of) and pinned to the reference's recorded cost and rows before it judges the library.

Bounds.  Every bound below is gradient_cases.py's rule: restate() in float64 against itself in np.longdouble on the
inputs of the test, per instance and per output (grad, gx0, jtl) as max |f64 - longdouble| / max(1, max |longdouble|),
is the yardstick's own error; the library adds in another order (one reverse sweep against dense forward mode), so it
gets 16 times that.  Measured here (the tests named re-measure each figure and hold it to the recorded one):

  the 72 records of the six sets (PARAMS_F64_WORST, test_params_restatement_is_the_reference):
      A 1.25e-15, B 4.20e-15, W 1.45e-15, U 4.75e-15, G 2.78e-15, T 4.28e-15; worst 4.746e-15, kept as
      PARAMS_F64_WORST = 4.75e-15; PARAMS_BOUND = 16 * PARAMS_F64_WORST = 7.6e-14
      (the library's worst error: A 1.0e-15, B 3.8e-15, W 9.7e-16, U 2.7e-15, G 1.8e-15, T 2.7e-15, both backends)
  the generated batches of the shape tests, per horizon (SHAPE_F64_WORST, test_shape_yardstick_budget):
      N = 1: 1.933e-15, 2: 3.586e-15, 15: 1.507e-15, 16: 2.895e-14 (the 64-row slab), 17: 1.337e-15, 31: 1.122e-15,
      32: 2.707e-15, 33: 1.924e-15, 63: 8.076e-15; the bound at horizon N is 16 * SHAPE_F64_WORST[N]

The stationarity bounds (section 4) are 8 times the oracle's own worst figures, recorded at STATIONARITY_ORACLE.

env: dict(mpcqp=module, device=-1 or 0, ptr=callable) as in evaluate_cases.py."""
import functools

import numpy as np

import evaluate_cases as EC
import gradient_cases as GC
import params_cases as PC

same = EC.same
PIN_KEYS = ("grad", "gx0", "jtl")


def model_of(p):
    """restate()'s model of an mpc_params (or oracle parameters): the names gradient_cases.default_model() uses."""
    return dict(dt=p.dt, w_d=p.w_d, w_o=p.w_o, w_v=p.w_v, w_u1=p.w_u1, w_u2=p.w_u2, osd=p.obstacle_safety_distance,
                tgap=p.max_time_2_obs, L=p.wheelbase, sl=p.lane_width / 2.0 - p.vehicle_radius - p.safe_lane_margin)


@functools.lru_cache(maxsize=None)
def set_model(name):
    """The model of parameter set `name` (None: the defaults), from the oracle's parameter struct."""
    import oracle as O
    return model_of(O.default_params(**(PC.sets()[name] if name else {})))


# ---------------------------------------------------------------------------------------------
# 1. the restatement under the six parameter sets
# ---------------------------------------------------------------------------------------------
PARAMS_F64_WORST = 4.75e-15
PARAMS_BOUND = 16 * PARAMS_F64_WORST
FD_SETS = ("A", "B", "G", "T")
SUMMARY_SETS = ("U", "A", "B")


def set_groups(name):
    """[(key, records, inputs)] of the `model` records of set `name`, batched per (trajectory, N, obstacle count)."""
    return [(key, cs, GC.group_inputs(key, cs)) for key, cs in sorted(EC.golden_groups(PC.cases(name, "model")).items())]


_set_yardstick = {}


def set_yardstick(name):
    """restate() in np.longdouble under set `name` on its records: {(key, b): result}, computed once."""
    if name not in _set_yardstick:
        out = {}
        for key, cs, w in set_groups(name):
            for b in range(len(cs)):
                obs = np.zeros((0, 2)) if w["obs"] is None else w["obs"][b]
                out[(key, b)] = GC.restate(key[0], w["x0"][b], w["U"][b], obs, w["lam"][b], np.longdouble, set_model(name))
        _set_yardstick[name] = out
    return _set_yardstick[name]


def check_yardstick_is_the_reference(name):
    """The longdouble restatement under the set's model reproduces the reference's recorded cost and constraint
    vector to 1e-12, the figure test_oracle_golden holds the oracle to on model_golden, taken relative to
    1 + |cost| and 1 + max |cons| as test_restatement_error_budget takes it under the defaults: the records are
    float64 sums of terms up to 4e3 (one ulp there is 4.5e-13) and the yardstick does not round where they did, so
    1e-12 absolute is below the records' own rounding (measured: up to 3.9e-12 absolute, 1.0e-15 relative).
    Returns the worst error of the float64 restatement against the yardstick."""
    worst, n = 0.0, 0
    for key, cs, w in set_groups(name):
        for b, c in enumerate(cs):
            ref = set_yardstick(name)[(key, b)]
            assert abs(float(ref["cost"]) - float(c["cost"])) <= 1e-12 * (1 + abs(float(c["cost"]))), (name, key, b)
            got = EC.reference_vector(ref["rows"].astype(np.float64), key[2])
            assert got.shape == c["cons"].shape, (name, key, b)
            assert np.abs(got - c["cons"]).max() <= 1e-12 * (1 + np.abs(c["cons"]).max()), (name, key, b)
            obs = np.zeros((0, 2)) if w["obs"] is None else w["obs"][b]
            r64 = GC.restate(key[0], w["x0"][b], w["U"][b], obs, w["lam"][b], np.float64, set_model(name))
            worst = max([worst] + [GC.rel_err(r64[k], ref[k]) for k in PIN_KEYS])
            n += 1
    assert n == 12
    return worst


def set_gradient(env, name):
    """[(key, records, inputs, gradient result, evaluator result)] of set `name` on env's device, once."""
    cache = env.setdefault("_grad_sets", {})
    ck = (env["device"], name)
    if ck not in cache:
        out = []
        for key, cs, w in set_groups(name):
            slv = GC.solver(env, *key, **PC.sets()[name])
            r = slv.gradient_batch(w["x0"], w["U"], w["obs"], w["n_obs"], lam=w["lam"], costate=True)
            e = slv.evaluate_batch(w["x0"], w["U"], w["obs"], w["n_obs"], rows=True)
            for v in list(r.values()) + list(e.values()):
                v.setflags(write=False)
            out.append((key, cs, w, r, e))
        cache[ck] = out
    return cache[ck]


def check_set_pin(env, name):
    """grad, gx0 and jtl of the library under set `name` against the longdouble yardstick on every record within
    PARAMS_BOUND; COST with MPC_EVQ_COST's bits, which are the reference's recorded cost."""
    worst, n = 0.0, 0
    for key, cs, w, r, e in set_gradient(env, name):
        assert same(r["summary"][:, 0], e["summary"][:, 0]), (name, key)
        for b, c in enumerate(cs):
            ref = set_yardstick(name)[(key, b)]
            for k in PIN_KEYS:
                err = GC.rel_err(r[k][b], ref[k])
                worst = max(worst, err)
                assert err <= PARAMS_BOUND, (name, key, b, k, err)
            assert r["summary"][b, 0] == float(c["cost"]), (name, key, b)
            n += 1
    assert n == 12
    print(f"restatement pin, set {name}: worst error {worst:.3e} (bound {PARAMS_BOUND:.3e})")


def check_set_summary(env, name):
    """The summary under set `name` against numpy_summary on the records, and with every record's controls moved
    below, onto and above the set's own u_min / u_max: PG_INF then shows a swapped or a literal bound."""
    pset = PC.sets()[name]
    for key, cs, w, r, e in set_gradient(env, name):
        slv = GC.solver(env, *key, **pset)
        GC.check_summary(slv, w, r, (name, key))
        lo, hi = np.array(list(slv.params.u_min)), np.array(list(slv.params.u_max))
        assert list(lo) == pset["u_min"] and list(hi) == pset["u_max"]
        B, N = w["U"].shape[:2]
        rng = np.random.default_rng([key[0], key[1], key[2], 7])
        # per instance and control one of: below u_min, on u_min, inside, on u_max, above u_max
        kind = np.stack([np.stack([rng.permutation(N) % 5 for _ in range(2)], axis=1) for _ in range(B)])
        off = rng.uniform(0.05, 0.5, (B, N, 2))
        U = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                      [lo - off, lo + 0 * off, lo + (hi - lo) * off, hi + 0 * off, hi + off])
        for b in range(B):
            for a in range(2):
                assert set(np.unique(kind[b, :, a])) == {0, 1, 2, 3, 4}, (name, key, b, a)
        v = dict(w, U=np.ascontiguousarray(U))
        rv = GC.gradient(slv, v)
        GC.check_summary(slv, v, rv, (name, key, "bounds"))
        assert (rv["summary"][:, 3] > 0).all()


def check_set_finite_differences(env, name):
    """check_finite_differences on the records of set `name`, through contexts with that set; smooth_case judges by
    the set's own tgap and osd and may leave out at most one record in ten."""
    used, total, _, _ = GC.check_finite_differences(env, set_gradient(env, name), set_model(name), f", set {name}",
                                                    **PC.sets()[name])
    assert total == 12 and 10 * (total - used) <= total, (name, used, total)


# ---------------------------------------------------------------------------------------------
# 2. boundary horizons, several wavefronts and the slab against the yardstick
# ---------------------------------------------------------------------------------------------
SHAPE_N = (1, 2, 15, 16, 17, 31, 32, 33, 63)
SHAPE_F64_WORST = {1: 1.94e-15, 2: 3.59e-15, 15: 1.51e-15, 16: 2.90e-14, 17: 1.34e-15, 31: 1.13e-15, 32: 2.71e-15,
                   33: 1.93e-15, 63: 8.08e-15}
SHAPE_B = {16: 9, 32: 5, 64: 3}          # lane group -> two full wavefronts (GL 16, 32, 64: 4, 2, 1 a wave) and one more
BRANCH_MARGIN = 1e-9


def lane_group(N):
    return 16 if N + 1 <= 16 else (32 if N + 1 <= 32 else 64)


def shape_cases():
    """(trajectory, N, max_obs, set name | None): every horizon on trajectory 1 and N = 16, 32, 63 on 2 and 3 with a
    slab of 8; sets A and B at N = 16, 32, 63; the 64-row slab at N = 16 and 32; no obstacles at N = 16 and 33."""
    out = [(1, N, 8, None) for N in SHAPE_N] + [(t, N, 8, None) for t in (2, 3) for N in (16, 32, 63)]
    out += [(2, N, 8, name) for name in ("A", "B") for N in (16, 32, 63)]
    out += [(3, N, 64, None) for N in (16, 32)] + [(1, N, 0, None) for N in (16, 33)]
    return out


def case_id(case):
    t, N, mo, name = case
    return f"traj{t}-N{N}-obs{mo}-{name or 'default'}"


@functools.lru_cache(maxsize=None)
def shape_batch(case):
    """The seeded batch of one case: x0 on the table at seeded stations with offsets in d, o and v, U within the
    set's bounds, obstacles ahead of the ego, lam >= 0.  Instance 0 starts before the table (s < 0), instance 1 so
    close to s_max that its rollout passes it; the instances alternate between speeds below and above the safe
    distance's kink osd / tgap; n_obs cycles through max_obs, 0 and the two counts between."""
    import oracle as O
    t, N, mo, name = case
    m, p = set_model(name), O.default_params(**(PC.sets()[name] if name else {}))
    B = SHAPE_B[lane_group(N)]
    sv, X = GC._table(t)
    smax = sv[-1]
    rng = np.random.default_rng([t, N, mo, 1 + PC.SET_NAMES.index(name) if name else 0, 2024])
    s = rng.uniform(0.05 * smax, 0.8 * smax, B)
    vk = m["osd"] / m["tgap"]
    fast = np.arange(B) % 4 != 2
    v = np.where(fast, rng.uniform(1.5 * vk, 3.0 * vk, B), rng.uniform(0.3 * vk, 0.6 * vk, B))
    s[0] = -rng.uniform(0.5, 3.0)
    s[1] = smax - rng.uniform(0.1, 0.25) * N * m["dt"] * v[1]
    i = np.clip(np.searchsorted(sv, s), 1, len(sv) - 1)
    ref = X[i - 1] + (X[i] - X[i - 1]) * ((s - sv[i - 1]) / (sv[i] - sv[i - 1]))[:, None]
    x0 = np.column_stack([s, ref[:, 1] + rng.normal(0, 0.2, B), ref[:, 2] + rng.normal(0, 0.03, B), ref[:, 3], v])
    lo, hi = np.array(list(p.u_min)), np.array(list(p.u_max))
    U = lo + (hi - lo) * rng.uniform(0.3, 0.7, (B, N, 2))
    lam = rng.uniform(0.0, 2.0, (B, N, 7 + mo))
    obs = n_obs = None
    if mo:
        between = (1, 2) if mo == 8 else (1, 33)
        n_obs = np.array([(mo, 0) + between][0], np.int32)[np.arange(B) % 4]
        obs = np.stack([s[:, None] + rng.uniform(5.0, 90.0, (B, mo)), rng.uniform(0.0, 8.0, (B, mo))], axis=2)
    return dict(x0=x0, U=np.ascontiguousarray(U), obs=obs, n_obs=n_obs, lam=lam)


def _instance(case, w, b, dtype):
    no = 0 if w["obs"] is None else int(w["n_obs"][b])
    obs = np.zeros((0, 2)) if not no else w["obs"][b, :no]
    lam = np.concatenate([w["lam"][b][:, :7], w["lam"][b][:, 7:7 + no]], axis=1)
    return GC.restate(case[0], w["x0"][b], w["U"][b], obs, lam, dtype, set_model(case[3]))


@functools.lru_cache(maxsize=None)
def shape_yardstick(case):
    """restate() in np.longdouble on every instance of the case's batch (its first n_obs obstacles), once."""
    w = shape_batch(case)
    return [_instance(case, w, b, np.longdouble) for b in range(w["x0"].shape[0])]


def check_shape_inputs(case):
    """What the batch is there for, by the yardstick's own values: an instance that starts at s < 0, one whose
    rollout passes s_max, stages on both sides of v tgap > osd (among the instances with obstacles, where the
    slab has any), and no stage within BRANCH_MARGIN of a table knot or of the kink."""
    t, N, mo, name = case
    w, ys, m = shape_batch(case), shape_yardstick(case), set_model(name)
    sv, _ = GC._table(t)
    svl, B = sv.astype(np.longdouble), w["x0"].shape[0]
    G = 64 // lane_group(N)                  # instances per wavefront: more than one wave, the last one partial
    assert B == SHAPE_B[lane_group(N)] and B > G and (G == 1 or B % G == 1)
    assert any(y["X"][0, 0] < 0 for y in ys)
    assert any(y["X"][0, 0] < svl[-1] and (y["X"][1:, 0] >= svl[-1]).any() for y in ys)
    above = below = False
    for b, y in enumerate(ys):
        knot = np.abs(y["X"][:, 0][:, None] - svl[None, :]).min()
        kink = y["X"][1:, 4] * np.longdouble(m["tgap"]) - np.longdouble(m["osd"])
        assert knot > BRANCH_MARGIN and np.abs(kink).min() > BRANCH_MARGIN, (case, b, float(knot), kink)
        if mo == 0 or w["n_obs"][b] > 0:
            above, below = above or bool((kink > 0).any()), below or bool((kink < 0).any())
    assert above and below, case
    if mo:
        assert set(w["n_obs"]) >= {0, mo} and len(set(w["n_obs"])) >= 3


def measure_shape_error(N):
    """The worst error of restate() in float64 against the yardstick over the cases at horizon N."""
    worst = 0.0
    for case in shape_cases():
        if case[1] == N:
            w = shape_batch(case)
            for b, ref in enumerate(shape_yardstick(case)):
                r64 = _instance(case, w, b, np.float64)
                worst = max([worst] + [GC.rel_err(r64[k], ref[k]) for k in PIN_KEYS])
    return worst


def _past(w, value):
    """The batch with `value` in the obstacle rows and lam columns at and past each instance's n_obs."""
    if w["obs"] is None:
        return w
    mo = w["obs"].shape[1]
    gone = np.arange(mo)[None, :] >= w["n_obs"][:, None]
    obs, lam = w["obs"].copy(), w["lam"].copy()
    obs[gone] = value
    lam[:, :, 7:][np.broadcast_to(gone[:, None, :], lam[:, :, 7:].shape)] = value
    return dict(w, obs=obs, lam=lam)


def check_shape(env, case):
    """One case on env's device: NaN at and past n_obs changes no bit against zeros there; grad, gx0 and jtl are
    within 16 x SHAPE_F64_WORST[N] of the yardstick; the summary is numpy's; every instance alone (B = 1) has the
    bits it has in the batch."""
    t, N, mo, name = case
    slv = GC.solver(env, t, N, mo, **(PC.sets()[name] if name else {}))
    w = shape_batch(case)
    r = GC.gradient(slv, _past(w, 0.0))
    rn = GC.gradient(slv, _past(w, np.nan))
    assert mo == 0 or np.isnan(_past(w, np.nan)["lam"]).any()
    for k in GC.OUT_KEYS:
        assert same(rn[k], r[k]), (case, k)
    bound, worst = 16 * SHAPE_F64_WORST[N], 0.0
    for b, ref in enumerate(shape_yardstick(case)):
        for k in PIN_KEYS:
            err = GC.rel_err(r[k][b], ref[k])
            worst = max(worst, err)
            assert err <= bound, (case, b, k, err, bound)
    print(f"shape pin {case_id(case)}: worst error {worst:.3e} (bound {bound:.3e})")
    GC.check_summary(slv, _past(w, np.nan), rn, case)
    for b in range(w["x0"].shape[0]):
        one = GC.gradient(slv, {k: (None if a is None else a[b:b + 1]) for k, a in _past(w, np.nan).items()})
        for k in GC.OUT_KEYS:
            assert same(one[k][0], r[k][b]), (case, b, k)


# ---------------------------------------------------------------------------------------------
# 4. first-order optimality of the solver's answers
# ---------------------------------------------------------------------------------------------
ACTIVE_TOL = 1e-6
SQP_TOL = 1e-10
FIGURES = ("PG_INF", "COMPL", "-MIN_LAM")
# The oracle's SQP at the same settings on the same batches through the same measure on the host backend's gradient
# entry: the worst PG_INF, COMPL and -MIN_LAM over the qualifying instances, per parameter set (the default set over
# its four batches).  Measured 2026-10-21 on the tree of commit 8c90f0e with these tests added:
#   C2 N=20 default 7.723e-10 4.657e-12 0     C3 N=20 default 3.805e-10 1.356e-11 0
#   C2 N=20 A       3.668e-11 1.129e-14 0     C3 N=20 A       1.099e-11 3.072e-12 0
#   C2 N=20 B       8.486e-09 5.177e-12 0     C3 N=20 B       1.836e-09 7.776e-11 0
#   C2 N=33 default 1.629e-08 6.810e-12 0     C3 N=33 default 1.138e-08 1.995e-11 0
# (no qualifying instance has a negative least-squares multiplier, so -MIN_LAM is 0 and stays bounded by 0).
# test_stationarity_oracle_figures re-measures them.  The bound of a set is 8 times its figures: the SQP stops on the
# step length, not on the gradient, and the two sides may differ by up to 1e-8 in U.
STATIONARITY_ORACLE = {None: (1.629e-08, 1.995e-11, 0.0), "A": (3.668e-11, 3.073e-12, 0.0), "B": (8.486e-09, 7.776e-11, 0.0)}
STATIONARITY_BOUND = {k: tuple(8 * f for f in v) for k, v in STATIONARITY_ORACLE.items()}
# (workload, N, set, seed of workloads.make_batch): the 203-ego batches of test_gpu_horizons.sweep_batch (seeds 71 and
# 73); C2 under set A and C3 under set B take other egos of the same workload, because those batches hold only 6
# qualifying instances with an active row (C2, A) and 6 with a control on a bound (C3, B) where 9 are asked for
STATIONARITY_B = 203
STATIONARITY_CASES = [("C2", 20, None, 71), ("C2", 20, "A", 171), ("C2", 20, "B", 71), ("C2", 33, None, 71),
                      ("C3", 20, None, 73), ("C3", 20, "A", 73), ("C3", 20, "B", 171), ("C3", 33, None, 73)]


def stationarity_id(case):
    wl, N, name, seed = case
    return f"{wl}-N{N}-{name or 'default'}"


@functools.lru_cache(maxsize=None)
def _egos(wl, seed):
    import workloads as W
    return W.make_batch(wl, B=STATIONARITY_B, seed=seed)


def stationarity_batch(case):
    """(workload batch at the case's horizon, parameter set) of one case; the arrays are shared and never written."""
    wl, N, name, seed = case
    return dict(_egos(wl, seed), N=int(N)), (PC.sets()[name] if name else {})


@functools.lru_cache(maxsize=None)
def oracle_answer(case):
    """The oracle's SQP on the case's batch at the drop-in default settings, in solve_batch's format."""
    import oracle as O
    import trajectory_tracking as TT
    from conftest import traj_arrays
    wb, pset = stationarity_batch(case)
    po = O.default_params(N=wb["N"], max_obs=wb["max_obs"], sqp_iters=TT.SQP_ITERS, sqp_tol=SQP_TOL, **pset)
    return O.Oracle(*traj_arrays(wb["traj"])).solve_batch(po, wb["x0"], wb["obs"], wb["n_obs"])


def library_answer(env, case, **kw):
    """The library's SQP on env's device at the drop-in default settings (kw: other solver knobs)."""
    import trajectory_tracking as TT
    wb, pset = stationarity_batch(case)
    slv = GC.solver(env, wb["traj"], wb["N"], wb["max_obs"], **dict(dict(pset, sqp_iters=TT.SQP_ITERS, sqp_tol=SQP_TOL), **kw))
    return slv.solve_batch(wb["x0"], wb["obs"], wb["n_obs"])


def measure_stationarity(env, case, r):
    """The answer r (U, Xpred, status) of the case's batch through the measure of tools/optimality_report.py on env's
    device: multipliers by least squares on the rows <= ACTIVE_TOL, then mpc_gradient_batch's PG_INF, COMPL and
    -MIN_LAM.  Returns dict(fig [B, 3], ok: MPC_OK and converged, q: qualifies (ok and smooth along Xpred),
    active / bound / obstacles: the instance has an active row / a control on a bound / obstacles)."""
    from tools.optimality_report import estimate_multipliers
    mpcqp = env["mpcqp"]
    wl, N, name, _ = case
    wb, pset = stationarity_batch(case)
    slv = GC.solver(env, wb["traj"], wb["N"], wb["max_obs"], **pset)
    p, m = slv.params, set_model(name)
    U = np.ascontiguousarray(np.asarray(r["U"], np.float64).reshape(-1, N, 2))
    lam, n_active = estimate_multipliers(slv, wb["x0"], U, wb["obs"], wb["n_obs"], ACTIVE_TOL)
    s = slv.gradient_batch(wb["x0"], U, wb["obs"], wb["n_obs"], lam=lam)["summary"]
    fig = np.column_stack([s[:, mpcqp.GRQ_PG_INF], s[:, mpcqp.GRQ_COMPL], -s[:, mpcqp.GRQ_MIN_LAM]])
    st = np.asarray(r["status"])
    ok = ((st & mpcqp.MPC_STATUS_MASK) == mpcqp.MPC_OK) & ((st & mpcqp.MPC_SQP_UNCONVERGED) == 0)
    X = np.asarray(r["Xpred"]).reshape(-1, N + 1, 5)
    smooth = np.array([GC.smooth_case(wb["traj"], X[b], m) for b in range(len(X))])
    lo, hi = np.array(list(p.u_min)), np.array(list(p.u_max))
    bound = ((U <= lo + 1e-9) | (U >= hi - 1e-9)).any(axis=(1, 2))
    obstacles = np.zeros(len(X), bool) if wb["n_obs"] is None else wb["n_obs"] > 0
    return dict(fig=fig, ok=ok, q=ok & smooth, active=n_active > 0, bound=bound, obstacles=obstacles)


def check_stationarity_population(case, t):
    """The conditions that keep the stationarity test from passing on nothing."""
    B, q = len(t["q"]), t["q"]
    assert 2 * q.sum() >= B, (case, int(q.sum()))
    assert 10 * (t["ok"] & ~q).sum() <= t["ok"].sum(), (case, int((t["ok"] & ~q).sum()), int(t["ok"].sum()))
    counts = (int((q & t["active"]).sum()), int((q & t["bound"]).sum()), int((q & t["obstacles"]).sum()))
    assert counts[0] >= 9 and counts[1] >= 9 and (counts[2] >= 9 or case[0] == "C2"), (case, counts)
    return counts


def worst_figures(t, mask=None):
    mask = t["q"] if mask is None else mask
    return tuple(float(v) for v in t["fig"][mask].max(axis=0))


def check_stationarity(env, case):
    """The library's drop-in SQP on env's device: the batch holds what it is there for, and PG_INF, COMPL and
    -MIN_LAM of every qualifying instance stay within 8 times the oracle's worst under the same parameter set."""
    t = measure_stationarity(env, case, library_answer(env, case))
    counts = check_stationarity_population(case, t)
    got, bound = worst_figures(t), STATIONARITY_BOUND[case[2]]
    print(f"stationarity {stationarity_id(case)}: {int(t['q'].sum())} of {len(t['q'])} qualify (active row, on a bound, "
          f"obstacles: {counts}); worst " + ", ".join(f"{n} {g:.3e} (bound {b:.3e})" for n, g, b in zip(FIGURES, got, bound)))
    for b in np.flatnonzero(t["q"]):
        assert (t["fig"][b] <= bound).all(), (case, int(b), t["fig"][b], bound)


def print_single_qp(env, case):
    """The single-QP answers (sqp_iters = 1) of one batch through the same measure, printed and not judged: they are
    not stationary points of the nonlinear problem, and the measure says so."""
    t = measure_stationarity(env, case, library_answer(env, case, sqp_iters=1))
    ok = t["ok"]
    print(f"single QP {stationarity_id(case)}: {int(ok.sum())} MPC_OK; worst " +
          ", ".join(f"{n} {g:.3e}" for n, g in zip(FIGURES, worst_figures(t, ok))) + "; median " +
          ", ".join(f"{n} {g:.3e}" for n, g in zip(FIGURES, np.median(t["fig"][ok], axis=0))))
    return t
