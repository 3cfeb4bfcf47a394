"""Shared pieces of the evaluator tests (test_evaluate_cpu.py on the host backend, test_gpu_evaluate.py on the
device): mpc_evaluate_batch against the reference's own predict / cost / constraints (tests/golden/model_golden.npz),
its summary against numpy on the returned rows, its rollout against the solver's, and the argument contract.

env: dict(mpcqp=module, device=-1 or 0, ptr=callable) where ptr(array) -> (address, keepalive) puts a numpy array
where the context's device entry reads it (host memory for device = -1, device memory for a GPU context)."""
import ctypes as C
import warnings

import numpy as np

from conftest import golden_cases, traj_arrays

_solvers = {}


def solver(env, traj, N, mo, device=None, **kw):
    """A cached context per (device, trajectory, N, max_obs, mpc_params fields given in kw)."""
    device = env["device"] if device is None else device
    key = (device, traj, N, mo, tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items())))
    if key not in _solvers:
        mpcqp = env["mpcqp"]
        _solvers[key] = mpcqp.Solver(*traj_arrays(traj), mpcqp.default_params(N=N, max_obs=mo, **kw), device=device)
    return _solvers[key]


def close_solvers():
    for s in _solvers.values():
        s.close()
    _solvers.clear()


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def reference_vector(rows, n_obs):
    """[N, 7 + M] rows -> the reference's vector: per stage the lane rows, the obstacle rows, then v."""
    return np.concatenate([rows[:, :6], rows[:, 7:7 + n_obs], rows[:, 6:7]], axis=1).ravel()


# ---------------------------------------------------------------------------------------------
# 1. reference pin
# ---------------------------------------------------------------------------------------------
def golden_groups(cases=None):
    """The 60 model_golden cases (or the given `cases` in model_golden's record format) batched per
    (trajectory, N, obstacle count)."""
    if cases is None:
        cases, _ = golden_cases("model_golden")
        assert len(cases) == 60
    groups = {}
    for c in cases:
        groups.setdefault((int(c["traj"]), int(c["N"]), int(c["obs"].shape[0])), []).append(c)
    return groups


def evaluate_golden(env, cases=None, tag=None, **kw):
    """[(key, cases, result)] of the golden groups on env's device, computed once per device; with `cases`, of those
    records under the mpc_params fields kw (cached per device and `tag`)."""
    cache = env.setdefault("_golden", {})
    ckey = env["device"] if cases is None else (env["device"], tag)
    if ckey not in cache:
        out = []
        for (ti, N, no), cs in sorted(golden_groups(cases).items()):
            slv = solver(env, ti, N, no, **kw)
            x0 = np.array([c["x0"] for c in cs])
            U = np.array([c["U"].reshape(N, 2) for c in cs])
            obs = np.array([c["obs"] for c in cs]).reshape(len(cs), no, 2) if no else None
            r = slv.evaluate_batch(x0, U, obs, None if not no else np.full(len(cs), no, np.int32), rows=True)
            for v in r.values():
                v.setflags(write=False)
            out.append(((ti, N, no), cs, r))
        cache[ckey] = out
    return cache[ckey]


def check_reference_pin(env, cases=None, tag=None, **kw):
    """Xpred, the cost and the rows are bit-equal to the reference's own predict / cost / constraints on all 60
    cases (or on all the given `cases`, recorded under the mpc_params fields kw), with the golden's exact row shape.  (The issue's bounds, 1e-12 (1 + |cost|) and 1e-12 per row, the ones
    tests/test_oracle_golden.py:41-44 holds the C oracle to, turned out to hold with no error at all on both
    backends, so equality is asserted.)"""
    TT = env["TT"]
    n = 0
    for (ti, N, no), cs, r in evaluate_golden(env, cases, tag, **kw):
        assert r["rows"].shape == (len(cs), N, 7 + no)
        for b, c in enumerate(cs):
            assert np.array_equal(r["Xpred"][b], c["X"]), (ti, N, no, b)
            assert r["summary"][b, 0] == float(c["cost"]), (ti, N, no, b, r["summary"][b, 0], float(c["cost"]))
            g = TT.constraint_rows(r["rows"], b, n_obs=no)
            assert g.shape == c["cons"].shape
            assert same(g, reference_vector(r["rows"][b], no))
            assert np.array_equal(g, c["cons"]), (ti, N, no, b, float(np.abs(g - c["cons"]).max()))
            n += 1
    assert n == (60 if cases is None else len(cases))


# ---------------------------------------------------------------------------------------------
# 2. summary against numpy
# ---------------------------------------------------------------------------------------------
def numpy_summary(rows, n_obs, U, u_min, u_max):
    """Columns 1..9 of the summary (everything but the cost) restated on the returned rows [N, 7 + M] and U [N, 2]."""
    q = np.full(10, np.nan)
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore")
        w = 7 + n_obs
        vec = reference_vector(rows, n_obs)
        q[1] = np.min(vec)
        i = int(np.argmin(vec))
        q[2] = i // w + 1
        pos = i % w
        q[3] = pos if pos < 6 else (6 if pos == w - 1 else 7 + (pos - 6))
        total = 0.0
        for stage in vec.reshape(-1, w):                       # the stated order, one addition at a time
            part = 0.0
            for g in stage:
                part = part + np.maximum(-g, 0.0)
            total = total + part
        q[4] = total
        q[5] = np.sum(vec < 0)
        q[6] = np.min(rows[:, :6])
        q[7] = np.min(rows[:, 7:7 + n_obs]) if n_obs else np.nan
        q[8] = np.min(rows[:, 6])
        lo, hi = np.asarray(u_min), np.asarray(u_max)
        q[9] = np.max(np.maximum(np.maximum(lo - U, U - hi), 0.0))
    return q


def check_summary(r, U, n_obs, params, what=""):
    """Every instance of an evaluate_batch result r (with rows) against numpy_summary; terms against plain sums."""
    B = U.shape[0]
    mo = r["rows"].shape[2] - 7
    for b in range(B):
        no = mo if n_obs is None else int(min(max(int(n_obs[b]), 0), mo))
        assert np.isnan(r["rows"][b, :, 7 + no:]).all(), (what, b)
        q = numpy_summary(r["rows"][b], no, U[b], list(params.u_min), list(params.u_max))
        assert same(r["summary"][b, 1:], q[1:]), (what, b, r["summary"][b], q)


def check_golden_summary(env):
    for (ti, N, no), cs, r in evaluate_golden(env):
        slv = solver(env, ti, N, no)
        U = np.array([c["U"].reshape(N, 2) for c in cs])
        check_summary(r, U, None, slv.params, (ti, N, no))
        p = slv.params
        # the cost shares: plain sums of the reference's terms on the returned rollout, 1e-12 relative
        for b, c in enumerate(cs):
            ref = np.array([_state(env, ti, s) for s in r["Xpred"][b, 1:, 0]])
            X = r["Xpred"][b, 1:]
            want = np.array([np.sum(p.w_d * (X[:, 1] - ref[:, 1]) ** 2), np.sum(p.w_o * (X[:, 2] - ref[:, 2]) ** 2),
                             np.sum(p.w_v * (X[:, 4] - ref[:, 4]) ** 2), np.sum(p.w_u1 * U[b, :, 0] ** 2),
                             np.sum(p.w_u2 * U[b, :, 1] ** 2)])
            assert np.all(np.abs(r["terms"][b] - want) <= 1e-12 * np.abs(want)), (ti, N, no, b, r["terms"][b], want)
            assert abs(r["terms"][b].sum() - r["summary"][b, 0]) <= 1e-12 * (1 + abs(r["summary"][b, 0]))


_loaders = {}


def _state(env, ti, s):
    if ti not in _loaders:
        from trajectory_loader import TrajectoryLoader, builtin_trajectory
        _loaders[ti] = TrajectoryLoader(builtin_trajectory(ti))
    return _loaders[ti].get_state(s)


# ---------------------------------------------------------------------------------------------
# 3. consistency with the solver
# ---------------------------------------------------------------------------------------------
def random_batch(traj, N, B, mo, seed, nobs_mode="mixed"):
    """A seeded batch on trajectory `traj`: states along the table (every fifth so close to s_max that the rollout
    passes it), controls drawn wider than the bounds (BOX > 0 occurs), obstacles around the ego.
    nobs_mode: None (n_obs NULL), 'zero', 'mixed' (0..mo per instance)."""
    X, _ = traj_arrays(traj)
    rng = np.random.default_rng(seed)
    smax = X[-1, 0]
    s = rng.uniform(0.0, 0.9 * smax, B)
    s[3::5] = smax - rng.uniform(0.0, 3.0, len(s[3::5]))
    idx = np.clip(np.searchsorted(X[:, 0], s), 0, len(X) - 1)
    x0 = np.column_stack([s, rng.normal(0, 0.3, B), rng.normal(0, 0.05, B), X[idx, 3] + rng.normal(0, 0.01, B),
                          rng.uniform(0.5, 15.0, B)])
    U = np.stack([rng.uniform(-0.8, 0.8, (B, N)), rng.uniform(-6.0, 5.0, (B, N))], axis=2)
    obs = n_obs = None
    if mo:
        obs = np.stack([s[:, None] + rng.uniform(-5.0, 80.0, (B, mo)), rng.uniform(0.0, 10.0, (B, mo))], axis=2)
        if nobs_mode == "zero":
            n_obs = np.zeros(B, np.int32)
        elif nobs_mode == "mixed":
            n_obs = rng.integers(0, mo + 1, B).astype(np.int32)
            n_obs[0] = mo
    return dict(x0=x0, U=np.ascontiguousarray(U), obs=obs, n_obs=n_obs)


def check_solver_consistency(env):
    """evaluate_batch(x0, U*) returns the Xpred bits solve_batch returned with U*: 37 instances, N = 10,
    trajectory2, a slab of 2 with mixed n_obs including 0."""
    slv = solver(env, 2, 10, 2)
    w = random_batch(2, 10, 37, 2, seed=5)
    w["obs"][:, :, 0] = w["x0"][:, :1] + np.array([25.0, 60.0])
    assert (w["n_obs"] == 0).any() and (w["n_obs"] == 2).any()
    r = slv.solve_batch(w["x0"], w["obs"], w["n_obs"])
    e = slv.evaluate_batch(w["x0"], r["U"], w["obs"], w["n_obs"], rows=True)
    assert np.array_equal(e["Xpred"], r["Xpred"])
    check_summary(e, r["U"], w["n_obs"], slv.params, "solver consistency")
    # the solver respects the bounds it is given
    assert (e["summary"][:, 9] <= 1e-9).all()


# ---------------------------------------------------------------------------------------------
# 4. shapes: every lane-group boundary, partial tail groups, slab widths, NaN isolation
# ---------------------------------------------------------------------------------------------
SHAPE_N = (1, 15, 16, 31, 32, 63)
SHAPE_B = (1, 5, 67)
SHAPE_MO = (0, 1, 64)
KEYS = ("Xpred", "summary", "terms", "rows")


def shape_runs(N, mo):
    """(B, nobs_mode, batch) for the shape tests of one (N, max_obs)."""
    for B in SHAPE_B:
        for mode in ((None,) if mo == 0 else (None, "zero", "mixed")):
            yield B, mode, random_batch(2, N, B, mo, seed=1000 * N + 10 * B + mo, nobs_mode=mode)


def with_nans(w, B):
    """The batch with a NaN in x0 of instance 1 and a NaN control in the last instance; returns (batch, mask of the
    untouched instances)."""
    v = {k: (None if a is None else a.copy()) for k, a in w.items()}
    v["x0"][1, 0] = np.nan
    v["U"][B - 1, v["U"].shape[1] // 2, 1] = np.nan
    keep = np.ones(B, bool)
    keep[[1, B - 1]] = False
    return v, keep


def check_nan_isolation(slv, w, B, base):
    """NaN instances must not disturb their wave partners: the partners equal the run without the NaNs; the NaN
    instances report NaN."""
    v, keep = with_nans(w, B)
    r = slv.evaluate_batch(v["x0"], v["U"], v["obs"], v["n_obs"], rows=True)
    for k in KEYS:
        assert same(r[k][keep], base[k][keep]), k
    assert np.isnan(r["summary"][1, [0, 1, 4]]).all() and np.isnan(r["summary"][B - 1, [0, 9]]).all()
    check_summary(r, v["U"], v["n_obs"], slv.params, "nan")
    return v, r


# ---------------------------------------------------------------------------------------------
# 5. output selection and misuse
# ---------------------------------------------------------------------------------------------
def raw_evaluate(env, slv, w, want, B=None):
    """mpc_evaluate_batch through ctypes with only the outputs named in `want`; returns (rc, outputs)."""
    mpcqp = env["mpcqp"]
    p = slv.params
    B = w["x0"].shape[0] if B is None else B
    nb = max(B, 0)
    shapes = dict(Xpred=(nb, p.N + 1, 5), summary=(nb, mpcqp.EV_NQ), terms=(nb, 5), rows=(nb, p.N, 7 + p.max_obs))
    out = {k: np.full(shapes[k], -7.0) for k in want}
    dp = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    rc = mpcqp.lib().mpc_evaluate_batch(slv.h, B, dp(w["x0"]), dp(w["obs"]), ip(w["n_obs"]), dp(w["U"]),
                                        *(dp(out.get(k)) for k in KEYS))
    return rc, out


def check_output_selection(env):
    """Every subset of NULL outputs gives the same values in the others; all-NULL and B == 0 succeed."""
    slv = solver(env, 2, 10, 2)
    w = random_batch(2, 10, 9, 2, seed=77)
    rc, full = raw_evaluate(env, slv, w, KEYS)
    assert rc == 0
    assert not any((full[k] == -7.0).all() for k in KEYS)
    for mask in range(16):
        want = tuple(k for i, k in enumerate(KEYS) if mask >> i & 1)
        rc, out = raw_evaluate(env, slv, w, want)
        assert rc == 0, (want, env["mpcqp"].last_error())
        for k in want:
            assert same(out[k], full[k]), (want, k)
    rc, _ = raw_evaluate(env, slv, w, KEYS, B=0)
    assert rc == 0


def check_misuse(env):
    """The documented codes, each with a message; n_obs outside [0, max_obs] is clamped like mpc_solve_batch."""
    mpcqp = env["mpcqp"]
    slv = solver(env, 2, 10, 2)
    w = random_batch(2, 10, 6, 2, seed=78)

    def refused(rc):
        assert rc == -1 and len(mpcqp.last_error()) > 0, (rc, mpcqp.last_error())

    refused(raw_evaluate(env, slv, dict(w, U=None), KEYS)[0])
    refused(raw_evaluate(env, slv, dict(w, x0=None), KEYS, B=6)[0])
    refused(raw_evaluate(env, slv, w, KEYS, B=-1)[0])
    with np.testing.assert_raises(ValueError):
        slv.evaluate_batch(w["x0"], None)
    s0 = solver(env, 2, 10, 0)
    refused(raw_evaluate(env, s0, w, ("summary",))[0])
    with np.testing.assert_raises(ValueError):
        s0.evaluate_batch(w["x0"], w["U"], w["obs"], w["n_obs"])
    # out-of-range counts: the solver clamps them to [0, max_obs], and so does the evaluator
    wild = np.array([5, -3, 2, 0, 1, 99], np.int32)
    a = slv.evaluate_batch(w["x0"], w["U"], w["obs"], wild, rows=True)
    b = slv.evaluate_batch(w["x0"], w["U"], w["obs"], np.clip(wild, 0, 2), rows=True)
    for k in KEYS:
        assert same(a[k], b[k]), k
    # the device entry: a misaligned double array, and n_obs without obs
    keep = []

    def ptr(a, off=0):
        if a is None:
            return None
        addr, k = env["ptr"](a)
        keep.append(k)
        return addr + off

    out = np.zeros((6, mpcqp.EV_NQ))
    L = mpcqp.lib()
    x0p, Up, op, np_, sp = ptr(w["x0"]), ptr(w["U"]), ptr(w["obs"]), ptr(w["n_obs"]), ptr(out)
    assert L.mpc_evaluate_batch_device(slv.h, 6, x0p, op, np_, Up, None, sp, None, None, None) == 0
    for args in ((x0p + 4, op, np_, Up, None, sp), (x0p, op + 4, np_, Up, None, sp), (x0p, op, np_, Up + 4, None, sp),
                 (x0p, op, np_, Up, None, sp + 4), (x0p, None, np_, Up, None, sp), (x0p, op, np_, None, None, sp)):
        refused(L.mpc_evaluate_batch_device(slv.h, 6, *args, None, None, None))
    assert L.mpc_evaluate_batch_device(slv.h, 6, x0p, op, np_, Up, None, None, None, None, None) == 0
    assert L.mpc_evaluate_batch_device(slv.h, 0, None, None, None, None, None, None, None, None, None) == 0
    env.get("sync", lambda: None)()          # the buffers in `keep` outlive the asynchronous call
