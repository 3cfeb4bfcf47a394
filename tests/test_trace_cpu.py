"""mpc_closed_loop_traced on the host backend (device = -1): the noisy loop that keeps the plan behind each applied
control (hist_pred, hist_plan) and accumulates the plan-vs-outcome gaps of every ego (gapq).  References, all bit
for bit: mpc_closed_loop_noisy for everything the noisy entry has, with and without trace outputs; a stepwise
restatement around Solver.solve_batch on the same backend that keeps each step's U and Xpred, with the gap columns
computed from them in numpy; halves of the batch with ego_offset.  The bodies are shared with
tests/test_gpu_trace.py (trace_cases.py).  Trajectory1, N = 5 and N = 20."""
import numpy as np
import pytest

import sweep_cases as SC
import trace_cases as TRC

CASES = [(N, noisy) for N in TRC.HORIZONS for noisy in (False, True)]


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import mpcqp
    import shard
    import trajectory_tracking as TT
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    traj = TrajectoryLoader(builtin_trajectory(1))
    solvers = {}

    def solver(N, max_obs=0):
        if (N, max_obs) not in solvers:
            solvers[N, max_obs] = mpcqp.Solver(traj.X_ref, traj.U_ref, mpcqp.default_params(N=N, max_obs=max_obs),
                                               device=-1)
        return solvers[N, max_obs]

    yield dict(mpcqp=mpcqp, shard=shard, TT=TT, traj=traj, solver=solver)
    for s in solvers.values():
        s.close()


@pytest.mark.parametrize("N,noisy", CASES)
def test_nothing_requested_is_the_noisy_entry(env, N, noisy):
    TRC.check_anchor_off(env, N, noisy)


@pytest.mark.parametrize("N,noisy", CASES)
def test_traces_leave_the_noisy_outputs_alone(env, N, noisy):
    TRC.check_anchor_on(env, N, noisy)


@pytest.mark.parametrize("N,noisy", CASES)
def test_traces_equal_the_restatement(env, N, noisy):
    TRC.check_restatement(env, N, noisy)


@pytest.mark.parametrize("N,noisy", CASES)
def test_known_answers(env, N, noisy):
    TRC.check_known_answers(env, N, noisy)


@pytest.mark.parametrize("N,noisy", [(5, True), (20, False)])
def test_composition_invariance(env, N, noisy):
    TRC.check_composition(env, N, noisy)


def test_misuse(env):
    TRC.check_misuse(env)


def test_run_simulation_traced(env):
    """Two scenarios in one traced call: per named ego the reference's run_simulation tuple, whose hist_x, hist_u,
    hist_obs_s and hist_tl_state are what closed_loop_sweep gives for those scenarios, and one (N + 1, 5) prediction
    per step."""
    TT, traj = env["TT"], env["traj"]
    mpc = TT.TrajectoryTracker(traj, device=-1)
    mpc.N, mpc.sqp_iters = 5, 1
    steps = 40
    mk = lambda **kw: _fsm(TT, **kw)
    fsms = [mk(dynamic_obstacle=True, traffic_light=True), mk(dynamic_obstacle=False, traffic_light=True, tl_pos=4.0)]
    x_init = np.tile(np.array([0.0, 0.0, 0.0, 0.0, 0.5]), (2, 1))
    sw = TT.run_scenario_sweep(mpc, fsms, traj, x_init, max_steps=steps, hist_egos=[0, 1])
    out = TT.run_simulation_traced(mpc, fsms, traj, max_steps=steps)
    assert len(out) == 2
    for k, tup in enumerate(out):
        hist_x, hist_u, hist_t, hist_preds, hist_obs_s, hist_tl_state, trajectory = tup
        n = int(sw["n_steps"][k])
        assert n == steps and trajectory is traj
        assert SC.same(hist_x, sw["hist_x"][k, :n + 1]) and SC.same(hist_u, sw["hist_u"][k, :n])
        assert SC.same(np.array(hist_obs_s), sw["hist_obs_s"][k, :n])
        assert hist_tl_state == ["GREEN" if g else "RED" for g in sw["hist_tl"][k, :n]]
        assert hist_t.shape == (n,) and (hist_t >= 0).all()
        assert len(hist_preds) == n and all(p.shape == (mpc.N + 1, 5) for p in hist_preds)
        assert all(SC.same(p[0], hist_x[t]) for t, p in enumerate(hist_preds))
    assert not np.isnan(out[0][4]).all()                          # the car of scenario 0 was on the road
    only = TT.run_simulation_traced(mpc, fsms, traj, hist_egos=[1], max_steps=steps)
    assert len(only) == 1 and SC.same(only[0][0], out[1][0])
    assert all(SC.same(p, q) for p, q in zip(only[0][3], out[1][3]))


def _fsm(TT, **kw):
    """An ObstaclesFSM whose car and light lie just ahead of the reference start."""
    f = TT.ObstaclesFSM(kw.pop("dynamic_obstacle"), kw.pop("traffic_light"))
    f.obs_trigger_s, f.obs_start_s, f.obs_v, f.obs_end_s = 1.0, 20.0, 2.0, 1.0e6
    f.obs_s = f.obs_start_s
    f.tl_pos, f.tl_trigger_s, f.tl_stop_duration = 8.0, 100.0, 1.0
    for k, v in kw.items():
        setattr(f, k, v)
    return f
