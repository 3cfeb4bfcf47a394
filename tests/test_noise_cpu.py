"""mpc_closed_loop_noisy and mpc_noise_draw on the host backend (device = -1): the convoy loop with seeded Philox
noise between the world and the solver.  References, all bit for bit: Philox4x32-10 known answers and a numpy
restatement of the noise source; mpc_closed_loop_convoy for every all-zero form of the noise; a stepwise
restatement (noise_cases.driver); runs of single egos and half batches for the (seed, global index) contract.  The
test bodies are shared with tests/test_gpu_noise.py (noise_cases.py).  Trajectory2, N = 20."""
import numpy as np
import pytest

import noise_cases as NC
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


def test_default_noise_and_fields(env):
    mpcqp = env["mpcqp"]
    z = mpcqp.default_noise()
    assert all(v == 0.0 for f, _ in NC.FIELDS for v in getattr(z, f))
    n = mpcqp.default_noise(meas_sigma=0.5, act_sigma=[0.1, 0.2])
    assert list(n.meas_sigma) == [0.5] * 5 and list(n.act_sigma) == [0.1, 0.2] and list(n.perc_sigma) == [0.0, 0.0]
    assert mpcqp.NZX_FIELDS[:6] == mpcqp.CVX_FIELDS and mpcqp.NZX_FIELDS[mpcqp.NZX_N_CLAMPED] == "n_clamped"
    import ctypes
    assert ctypes.sizeof(mpcqp.MpcNoise) == 14 * 8


def test_run_noisy_sweep(env):
    """run_noisy_sweep replicates a world per seed: replica s equals Solver.closed_loop_noisy as global egos
    s*W .., whether its seed shares a library call with its neighbours or not; pass rates are counts / egos."""
    mpcqp, TT, traj = env["mpcqp"], env["TT"], env["traj"]
    mpc = TT.TrajectoryTracker(traj, device=-1)
    mpc.N, mpc.sqp_iters = 20, 1
    W, K = 2, 1
    x_world = TT.convoy_starts(traj, 1, W, 9.0, 8.0, s0=NC.S0)
    noise = NC.mild(mpcqp)
    seeds = [3, 4, 5, 9, 0]
    kw = dict(W=W, K=K, max_steps=NC.STEPS, s_stop=NC.S_STOP)
    r = TT.run_noisy_sweep(mpc, traj, x_world, noise, seeds, hist_egos=[0, 7, 9], seed=77, **kw)
    assert r["quant"].shape == (10, 13) and r["extra"].shape == (10, 11) and r["seeds"].tolist() == seeds
    assert r["hist_egos"].tolist() == [0, 7, 9] and r["hist_xm"].shape == (3, NC.STEPS, 5)
    assert r["quant"][:, 0].tolist() == [s * W + i for s in seeds for i in range(W)]
    slv = mpc.solver(max_obs=0)
    for k, s in enumerate(seeds):
        solo = slv.closed_loop_noisy(x_world, W, K, max_steps=NC.STEPS, s_stop=NC.S_STOP, noise=noise, seed=77,
                                     lo=s * W, hist_egos=range(W))
        assert SC.same(r["quant"][k * W:(k + 1) * W, NC.QCOLS], solo["quant"][:, NC.QCOLS]), s
        assert SC.same(r["extra"][k * W:(k + 1) * W], solo["extra"]), s
    assert SC.same(r["hist_xm"][1], solo_row(slv, x_world, W, K, noise, 9, 1)["hist_xm"][0])
    assert r["hist_lead"][0, 0, 0] == 1 and r["hist_lead"][1, 0, 0] == -1
    assert len(set(r["quant"][::W, 2].tolist())) == len(seeds)                    # the replicas differ
    assert r["verdicts"].shape == (10,) and r["on_road"].dtype == bool
    assert set(r["pass_rate"]) == set(mpcqp.CLV_NAMES)
    assert all(r["pass_rate"][k] == r["counts"][k] / 10.0 for k in mpcqp.CLV_NAMES)
    one = TT.run_noisy_sweep(mpc, traj, x_world[:1], None, range(4), max_steps=8, s_stop=NC.S_STOP)
    assert SC.same(one["quant"][:, NC.QCOLS], np.tile(one["quant"][:1, NC.QCOLS], (4, 1)))    # no noise: all alike
    with pytest.raises(ValueError):
        TT.run_noisy_sweep(mpc, traj, x_world, noise, [], **kw)
    with pytest.raises(ValueError):
        TT.run_noisy_sweep(mpc, traj, x_world, noise, [1], W=1, max_steps=4)


def solo_row(slv, x_world, W, K, noise, s, i):
    return slv.closed_loop_noisy(x_world, W, K, max_steps=NC.STEPS, s_stop=NC.S_STOP, noise=noise, seed=77,
                                 lo=s * W, hist_egos=[i])
