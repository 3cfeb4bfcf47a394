"""mpc_closed_loop_convoy on the device: cv_lead_kernel (a workgroup per world: the egos ranked through LDS, the
nearest leaders appended to the slab) between the traffic entry's unchanged kernels.  The references run the same
solver kernels on the same inputs and every comparison is bit for bit: mpc_closed_loop_traffic for worlds of one
ego and for K = 0, a stepwise restatement with a numpy brute-force leader choice and Solver.solve_batch on a
context with max_obs = A + K, the brute force on the run's own states at the wave and workgroup boundaries, and
one-world runs for the batch indexing.  The bodies are shared with tests/test_convoy_cpu.py (convoy_cases.py).
Trajectory2, N = 20, the solver's default single QP per step."""
import pytest

import convoy_cases as CC

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
