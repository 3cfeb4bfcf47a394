"""mpc_closed_loop_traffic on the device: tr_init_kernel / tr_fsm_kernel / tr_gather_kernel around the unchanged
solver, compaction and plant kernels.  The references run the same solver kernels on the same inputs and every
comparison is bit for bit: mpc_closed_loop_sweep for scripts that restate an mpc_fsm, a stepwise restatement
built from the pinned ObstaclesFSM shim, Solver.solve_batch (a second context with max_obs = A) and numpy for
many actors, one-ego traffic runs for the batch indexing.  The bodies are shared with tests/test_traffic_cpu.py
(traffic_cases.py).  Trajectory2, N = 20, the solver's default single QP per step."""
import pytest

import traffic_cases as TC

pytestmark = pytest.mark.gpu


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
                                            device=0)
        return solvers[max_obs]

    yield dict(mpcqp=mpcqp, shard=shard, TT=TT, traj=traj, solver=solver)
    for s in solvers.values():
        s.close()


def test_anchor_to_the_sweep(env):
    TC.check_anchor(env)


def test_many_actors_equal_the_restatement(env):
    TC.check_many(env, TC.many_driver(env))


def test_257_egos_equal_single_runs(env):
    TC.check_indexing(env)


def test_verdicts(env):
    TC.check_verdicts(env)


def test_misuse_and_bookkeeping(env):
    TC.check_misuse(env)


def test_pack_sweep_round_trip(env):
    TC.check_pack_sweep(env)


def test_long_cap_short_run(env):
    TC.check_long_cap(env, 512)
