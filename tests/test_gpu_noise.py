"""mpc_closed_loop_noisy and mpc_noise_draw on the device: nz_measure_kernel and nz_plant_kernel in the convoy
loop's gather and plant places, nz_draw_kernel for the draws (csrc/noise_kernels.h).  Every comparison is bit for
bit: Philox4x32-10 known answers and the numpy restatement of Philox4x32-10 and the variate; mpc_closed_loop_convoy
for every all-zero form of the noise (the struct forms run the new kernels, which pins the restated plant
arithmetic); a stepwise restatement with Solver.solve_batch on a context with max_obs = A + K; single egos and half
batches for the (seed, global index) contract.  The bodies are shared with tests/test_noise_cpu.py
(noise_cases.py).  Trajectory2, N = 20, the solver's default single QP per step, step caps of 24."""
import pytest

import noise_cases as NC

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


def test_known_answers_and_the_numpy_restatement(env):
    NC.check_known_answers(env)


def test_distribution_sanity(env):
    NC.check_distribution(env)


def test_anchor_to_the_convoy_entry(env):
    NC.check_anchor(env)


@pytest.mark.parametrize("name", NC.CASES)
def test_noisy_loop_equals_the_restatement(env, name):
    NC.check_restatement(env, name)


def test_composition_invariance(env):
    NC.check_composition(env)


def test_truth_versus_perception(env):
    NC.check_truth_and_perception(env)


def test_misuse(env):
    NC.check_misuse(env)


def test_host_and_device_draw_the_same_noise(env):
    """The same (seed, ego, step, channel) on a host context: the same words and variates."""
    import numpy as np
    mpcqp, traj = env["mpcqp"], env["traj"]
    host = mpcqp.Solver(traj.X_ref, traj.U_ref, mpcqp.default_params(N=20), device=-1)
    ego = np.arange(1000, dtype=np.int64) * (2 ** 33 + 1)
    wd, zd = env["solver"]().noise_draw(2 ** 63 + 11, ego, np.arange(1000) % 24, np.arange(1000) % 48)
    wh, zh = host.noise_draw(2 ** 63 + 11, ego, np.arange(1000) % 24, np.arange(1000) % 48)
    host.close()
    assert np.array_equal(wd, wh) and np.array_equal(zd, zh)
