"""mpc_evaluate_batch on the host backend (device = -1): the reference's predict / cost / constraint rows for any
control sequence, pinned to the reference's own values (model_golden), its summary pinned to numpy on the returned
rows, its rollout to the solver's, and the argument contract.  The test bodies are shared with
tests/test_gpu_evaluate.py (evaluate_cases.py)."""
import numpy as np
import pytest

import evaluate_cases as EC


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import mpcqp
    import trajectory_tracking as TT
    yield dict(mpcqp=mpcqp, TT=TT, device=-1, ptr=lambda a: (a.ctypes.data, a))
    EC.close_solvers()


def test_symbols_and_version(env):
    L = env["mpcqp"].lib()
    assert L.mpc_version() == 5
    assert hasattr(L, "mpc_evaluate_batch") and hasattr(L, "mpc_evaluate_batch_device")


def test_reference_pin(env):
    EC.check_reference_pin(env)


def test_summary_against_numpy(env):
    EC.check_golden_summary(env)


def test_consistency_with_the_solver(env):
    EC.check_solver_consistency(env)


@pytest.mark.parametrize("mo", EC.SHAPE_MO)
@pytest.mark.parametrize("N", EC.SHAPE_N)
def test_shapes_and_nan_isolation(env, N, mo):
    """The shapes of the GPU == host test on the host alone: the summary against numpy, NaN instances isolated."""
    slv = EC.solver(env, 2, N, mo)
    box = False
    for B, mode, w in EC.shape_runs(N, mo):
        r = slv.evaluate_batch(w["x0"], w["U"], w["obs"], w["n_obs"], rows=True)
        EC.check_summary(r, w["U"], w["n_obs"], slv.params, (N, mo, B, mode))
        box = box or bool((r["summary"][:, 9] > 0).any())
        if B >= 5:
            EC.check_nan_isolation(slv, w, B, r)
    assert box                       # the generator's out-of-bounds controls show up as BOX > 0


def test_tracker_surface(env):
    """TrajectoryTracker.evaluate_batch with solve_batch's obstacle forms, against the tracker's own one-instance
    cost / constraints (the numpy loops existing tests pin)."""
    TT = env["TT"]
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    traj = TrajectoryLoader(builtin_trajectory(2))
    mpc = TT.TrajectoryTracker(traj, device=-1)
    mpc.N = 10
    w = EC.random_batch(2, 10, 4, 2, seed=3)
    lists = [[dict(s=float(o[0]), v=float(o[1])) for o in w["obs"][b, :n]] for b, n in enumerate([2, 0, 1, 2])]
    r = mpc.evaluate_batch(w["x0"], w["U"], lists)
    assert list(r["n_obs"]) == [2, 0, 1, 2]
    for b in range(4):
        g = mpc.constraints(w["x0"][b], lists[b])["fun"](w["U"][b].ravel())
        got = TT.constraint_rows(r, b)
        assert got.shape == g.shape and np.abs(got - g).max() <= 1e-12
        c = mpc.cost(w["U"][b].ravel(), w["x0"][b])
        assert abs(r["summary"][b, 0] - c) <= 1e-12 * (1 + abs(c))
        assert np.array_equal(r["Xpred"][b], mpc.predict(w["x0"][b], w["U"][b].ravel()))
    ra = mpc.evaluate_batch(w["x0"], w["U"], w["obs"])
    assert ra["rows"].shape == (4, 10, 9) and (ra["n_obs"] == 2).all()
    r0 = mpc.evaluate_batch(w["x0"], w["U"])
    assert r0["rows"].shape == (4, 10, 7) and np.isnan(r0["summary"][:, 7]).all()
    assert np.array_equal(r0["Xpred"], ra["Xpred"])


def test_output_selection(env):
    EC.check_output_selection(env)


def test_misuse(env):
    EC.check_misuse(env)
