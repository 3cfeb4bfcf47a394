"""mpc_closed_loop_convoy on the host backend (device = -1): the egos of a world follow each other.  References,
all bit for bit: mpc_closed_loop_traffic for worlds of one ego and for K = 0; a stepwise restatement with a numpy
brute-force leader choice (convoy_cases.driver); the brute force on the run's own states at the world sizes where
the device kernel changes shape; one-world runs for the batch indexing.  The test bodies are shared with
tests/test_gpu_convoy.py (convoy_cases.py).  Trajectory2, N = 20."""
import numpy as np
import pytest

import convoy_cases as CC
import sweep_cases as SC


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import mpcqp
    import shard
    import trajectory_tracking as TT
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    traj = TrajectoryLoader(builtin_trajectory(2))
    solvers = {}

    def solver(max_obs=0):
        if max_obs not in solvers:
            solvers[max_obs] = mpcqp.Solver(traj.X_ref, traj.U_ref, mpcqp.default_params(N=20, max_obs=max_obs),
                                            device=-1)
        return solvers[max_obs]

    yield dict(mpcqp=mpcqp, shard=shard, TT=TT, traj=traj, solver=solver)
    for s in solvers.values():
        s.close()


def test_anchor_to_the_traffic_entry(env):
    CC.check_anchor(env)


@pytest.mark.parametrize("name", sorted(CC.PLAIN))
def test_platoons_equal_the_restatement(env, name):
    CC.check_plain(env, name, CC.plain_driver(env, name))


def test_queue_at_a_light_equals_the_restatement(env):
    CC.check_queue(env, CC.queue_case(env))


def test_cars_and_leaders_fill_the_slab(env):
    CC.check_full(env, CC.full_case(env))


@pytest.mark.parametrize("n_worlds", [1, 2])
@pytest.mark.parametrize("W", [2, 63, 64, 65, 128, 255, 256])
def test_wave_and_workgroup_boundaries(env, W, n_worlds):
    CC.check_boundaries(env, W, n_worlds)


def test_worlds_are_isolated(env):
    CC.check_isolation(env)


def test_verdicts(env):
    CC.check_verdicts(env)


def test_misuse_and_bookkeeping(env):
    CC.check_misuse(env)


def test_pack_sweep_round_trip(env):
    CC.check_pack_sweep(env)


def test_long_cap_short_run(env):
    CC.check_long_cap(env)


def test_run_convoy_sweep_and_starts(env):
    """convoy_starts places the worlds; run_convoy_sweep's rows equal Solver.closed_loop_convoy's and carry the
    verdict columns."""
    mpcqp, TT, traj = env["mpcqp"], env["TT"], env["traj"]
    mpc = TT.TrajectoryTracker(traj, device=-1)
    mpc.N, mpc.sqp_iters = 20, 1
    x_init = TT.convoy_starts(traj, 2, 4, 12.0, 8.0, s0=CC.S0)
    assert x_init.shape == (8, 5) and SC.same(x_init[:4], x_init[4:])
    assert x_init[:4, 0].tolist() == [CC.S0 + 12.0 * i for i in range(4)] and (x_init[:, 4] == 8.0).all()
    assert x_init[2, 3] == traj.get_state(CC.S0 + 24.0)[3] and not x_init[:, 1:3].any()
    scripts = [None] * 7 + [[mpcqp.light(CC.S0 + 60.0, 100.0, 1.0)]]
    r = TT.run_convoy_sweep(mpc, traj, x_init, 4, 2, lead_range=30.0, scripts=scripts, max_steps=60, hist_egos=[5],
                            s_stop=SC.S_STOP)
    assert r["quant"].shape == (8, 13) and r["extra"].shape == (8, 6) and r["hist_slab"].shape == (1, 60, 3, 2)
    rows = [[mpcqp.MpcActor()]] * 7 + [scripts[7]]
    ref = mpc.solver(max_obs=0).closed_loop_convoy(x_init, 4, 2, lead_range=30.0, scripts=rows, max_steps=60,
                                                   s_stop=SC.S_STOP, hist_egos=[5])
    assert SC.same(r["quant"][:, CC.QCOLS], ref["quant"][:, CC.QCOLS]) and SC.same(r["extra"], ref["extra"])
    assert SC.same(r["hist_slab"], ref["hist_slab"]) and np.array_equal(r["hist_lead"], ref["hist_lead"])
    assert r["hist_lead"][0, 0].tolist() == [6, 7] and r["extra"][0, mpcqp.CVX_MAX_LEADERS] == 2.0
    assert r["verdicts"].shape == (8,) and r["on_road"].dtype == bool and r["counts"]["destination"] == 0
    plain = TT.run_convoy_sweep(mpc, traj, x_init, 4, 1, max_steps=20, s_stop=SC.S_STOP)
    assert plain["hist_slab"].shape == (0, 20, 1, 2) and plain["extra"][3, mpcqp.CVX_MIN_LEAD_EGO] == -1.0
    with pytest.raises(ValueError):
        TT.run_convoy_sweep(mpc, traj, x_init, 4, 2, scripts=scripts[:2], max_steps=10)
