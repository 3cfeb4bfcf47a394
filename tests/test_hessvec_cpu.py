"""mpc_hessvec_batch on the host backend (device = -1): Hessian-vector products of cost - lam . g and the rows' tangents,
pinned to an independent second-order forward-mode restatement run in np.longdouble, to central differences of
mpc_gradient_batch, its structure, curv and summary to numpy on the returned arrays; independence of the other
directions and of the batch; the argument contract.  The test bodies are shared with tests/test_gpu_hessvec.py
(hessvec_cases.py)."""
import numpy as np
import pytest

import hessvec_cases as HC


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import mpcqp
    yield dict(mpcqp=mpcqp, device=-1, ptr=lambda a: (a.ctypes.data, a))
    HC.close_solvers()


def test_symbols_and_fields(env):
    mpcqp = env["mpcqp"]
    L = mpcqp.lib()
    assert hasattr(L, "mpc_hessvec_batch") and hasattr(L, "mpc_hessvec_batch_device")
    assert len(mpcqp.HVQ_FIELDS) == mpcqp.HV_NQ == 5 and mpcqp.HV_MAX_DIRS == 128
    assert "mpc_hessvec_batch" in mpcqp.EXPORTS and "mpc_hessvec_batch_device" in mpcqp.EXPORTS


def test_restatement_error_budget(env):
    """The float64 run of the restatement against its longdouble run stays within the worst that the bound was
    derived from (hessvec_cases.py's header); the restatement's first-order part is gradient_cases' yardstick."""
    assert np.finfo(np.longdouble).eps < 1e-18
    worst = HC.measure_restatement_error()
    print(f"restatement float64 vs longdouble: worst {worst:.3e}")
    assert worst <= HC.RESTATE_F64_WORST
    import evaluate_cases as EC
    for key, cs in EC.golden_groups().items():
        ti, N, no = key
        w = HC.GC.group_inputs(key, cs)
        for b in range(len(cs)):
            ref, first = HC.yardstick()[(key, b)], HC.GC.yardstick()[(key, b)]
            jtl = np.einsum("kc,kci->i", w["lam"][b].astype(np.longdouble), ref["J"])
            assert HC.rel_err(jtl.reshape(N, 2), first["jtl"]) <= 1e-17, (key, b)


def test_restatement_pin(env):
    HC.check_restatement_pin(env)


def test_finite_differences_of_the_gradient(env):
    HC.check_finite_differences(env)


def test_structure(env):
    HC.check_structure(env)


def test_summary_cases(env):
    HC.check_summary_cases(env)


@pytest.mark.parametrize("N", (20, 63))
def test_independence(env, N):
    HC.check_independence(env, N)


def test_contract(env):
    HC.check_contract(env)


@pytest.mark.parametrize("mo", HC.SHAPE_MO)
@pytest.mark.parametrize("N", HC.SHAPE_N)
def test_shapes_curv_and_summary(env, N, mo):
    """The shapes of the GPU == host test on the host alone: curv and the summary against numpy."""
    slv = HC.solver(env, 1, N, mo)
    for what, w, V, M, mode in HC.shape_runs(N, mo):
        HC.check_curv_and_summary(HC.hessvec(slv, w, V, M, mode), V, (N, mo, what))


def test_shim_hessian_batch(env):
    """TrajectoryTracker.hessian_batch (obstacle lists of mixed length, no obstacles) equals Solver.hessian_batch on the
    slab it builds, under ==."""
    import trajectory_tracking as TT
    import evaluate_cases as EC
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    N, B = 10, 4
    mpc = TT.TrajectoryTracker(TrajectoryLoader(builtin_trajectory(2)), device=env["device"])
    mpc.N = N
    w = HC.GC.lam_batch(EC.random_batch(2, N, B, 2, seed=171), 2, 172)
    w["n_obs"][:] = [2, 0, 1, 2]
    lists = [[dict(s=float(w["obs"][b, i, 0]), v=float(w["obs"][b, i, 1])) for i in range(int(w["n_obs"][b]))]
             for b in range(B)]
    slab = np.zeros_like(w["obs"])
    for b in range(B):
        slab[b, :w["n_obs"][b]] = w["obs"][b, :w["n_obs"][b]]
    for obstacles, slv, obs, n_obs, lam in ((lists, HC.solver(env, 2, N, 2), slab, w["n_obs"], w["lam"]),
                                           (None, HC.solver(env, 2, N, 0), None, None, None)):
        for mode in HC.MODES:
            got = mpc.hessian_batch(w["x0"], w["U"], lam, obstacles, mode)
            want = slv.hessian_batch(w["x0"], w["U"], lam, obs, n_obs, mode)
            for k in want:
                assert HC.same(got[k], want[k]), (mode, k)
            assert got["H"].shape == (B, 2 * N, 2 * N)
