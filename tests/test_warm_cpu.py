"""mpc_closed_loop_warm on the host backend (device = -1): the traced loop whose solver may be handed the ego's
previous plan, shifted by one stage, as the next linearisation point.  References, all bit for bit:
mpc_closed_loop_traced for the reference warm start, with and without warm outputs, and a sqp_iters = 0 solve for the
warm start that is then handed over; a stepwise restatement around Solver.solve_batch(..., ubar=...) on the same
backend that applies the carry rule in numpy, for both tails and three reset masks; halves of the batch with
ego_offset.  The bodies are shared with tests/test_gpu_warm.py (warm_cases.py).  Trajectory1, N = 5 and N = 20."""
import pytest

import warm_cases as WC
import trace_cases as TRC

CASES = [(N, noisy) for N in TRC.HORIZONS for noisy in (False, True)]
CARRIED = [(N, noisy, v) for N, noisy in CASES for v in WC.VARIANTS]


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

    def solver(N, max_obs=0, sqp_iters=1):
        key = (N, max_obs, sqp_iters)
        if key not in solvers:
            solvers[key] = mpcqp.Solver(traj.X_ref, traj.U_ref,
                                        mpcqp.default_params(N=N, max_obs=max_obs, sqp_iters=sqp_iters), device=-1)
        return solvers[key]

    yield dict(mpcqp=mpcqp, shard=shard, TT=TT, traj=traj, solver=solver)
    for s in solvers.values():
        s.close()


@pytest.mark.parametrize("N,noisy", CASES)
def test_reference_with_nothing_requested_is_the_traced_entry(env, N, noisy):
    WC.check_anchor_off(env, N, noisy)


@pytest.mark.parametrize("N,noisy", CASES)
def test_materialised_reference_leaves_the_traced_outputs_alone(env, N, noisy):
    WC.check_anchor_on(env, N, noisy)


@pytest.mark.parametrize("N,noisy,variant", CARRIED)
def test_carried_loop_equals_the_restatement(env, N, noisy, variant):
    WC.check_restatement(env, N, noisy, variant)


@pytest.mark.parametrize("N,noisy,variant", CARRIED)
def test_known_answers(env, N, noisy, variant):
    WC.check_known_answers(env, N, noisy, variant)


@pytest.mark.parametrize("N,noisy,variant", [(5, True, "hold_nobs"), (20, False, "ref_tail")])
def test_composition_invariance(env, N, noisy, variant):
    WC.check_composition(env, N, noisy, variant)


def test_misuse(env):
    WC.check_misuse(env)


def test_carry_with_sqp(env):
    """MPC_WARM_CARRY with sqp_iters = 3: ubar is the first QP's linearisation point, and the restatement, which runs
    the same solver with the same ubar, agrees."""
    sqp = {k: v for k, v in env.items() if not k.startswith("_")}            # its own cache of runs
    sqp["solver"] = lambda N, max_obs=0, sqp_iters=3: env["solver"](N, max_obs, 3)
    WC.check_restatement(sqp, 5, False, "ref_tail")


def test_run_simulation_carried(env):
    """run_simulation_traced's tuples with the carried loop: what closed_loop_warm gives for those scenarios, and
    not what the reference warm start gives."""
    import sweep_cases as SC
    import test_trace_cpu as TTC
    TT, traj = env["TT"], env["traj"]
    mpcqp = env["mpcqp"]
    mpc = TT.TrajectoryTracker(traj, device=-1)
    mpc.N, mpc.sqp_iters = 5, 1
    steps = 40
    fsms = [TTC._fsm(TT, dynamic_obstacle=True, traffic_light=True),
            TTC._fsm(TT, dynamic_obstacle=False, traffic_light=True, tl_pos=4.0)]
    traced = TT.run_simulation_traced(mpc, fsms, traj, max_steps=steps)
    out = TT.run_simulation_carried(mpc, fsms, traj, max_steps=steps, tail=mpcqp.WTAIL_HOLD, reset=mpcqp.WRESET_NOBS)
    x_init = [[0.0, 0.0, 0.0, 0.0, 0.5]] * 2
    w = mpc.solver(max_obs=0).closed_loop_warm(
        x_init, scripts=[TT.TrafficScript.from_fsm(f).actors for f in fsms], max_steps=steps, s_max=traj.s_max,
        hist_egos=[0, 1], preds=True,
        warm=mpcqp.default_warm(mode=mpcqp.WARM_CARRY, tail=mpcqp.WTAIL_HOLD, reset=mpcqp.WRESET_NOBS))
    assert len(out) == 2
    for k, tup in enumerate(out):
        hist_x, hist_u, hist_t, hist_preds, hist_obs_s, hist_tl_state, trajectory = tup
        n = int(w["n_steps"][k])
        assert trajectory is traj and hist_t.shape == (n,)
        assert SC.same(hist_x, w["hist_x"][k, :n + 1]) and SC.same(hist_u, w["hist_u"][k, :n])
        assert len(hist_preds) == n and all(SC.same(p, w["hist_pred"][k, t]) for t, p in enumerate(hist_preds))
        assert len(hist_obs_s) == n and len(hist_tl_state) == n
    assert any(not SC.same(a[1], b[1]) for a, b in zip(out, traced))
    only = TT.run_simulation_carried(mpc, fsms, traj, hist_egos=[1], max_steps=steps, tail=mpcqp.WTAIL_HOLD,
                                     reset=mpcqp.WRESET_NOBS)
    assert len(only) == 1 and SC.same(only[0][0], out[1][0])
