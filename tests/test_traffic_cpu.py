"""mpc_closed_loop_traffic on the host backend (device = -1): a script of up to 16 actors per ego, each a car or
a light with ObstaclesFSM's per-obstacle state machine.  References, all bit for bit: mpc_closed_loop_sweep for
scripts that restate an mpc_fsm; a stepwise restatement built from the pinned ObstaclesFSM shim, Solver.solve_batch
and numpy (traffic_cases.driver) for many actors; one-ego traffic runs for the batch indexing.  The test bodies
are shared with tests/test_gpu_traffic.py (traffic_cases.py).  Trajectory2, N = 20."""
import numpy as np
import pytest

import sweep_cases as SC
import traffic_cases as TC


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


@pytest.fixture(scope="module")
def many(env):
    return TC.many_driver(env)


def test_anchor_to_the_sweep(env):
    TC.check_anchor(env)


def test_many_actors_equal_the_restatement(env, many):
    TC.check_many(env, many)


def test_257_egos_equal_single_runs(env):
    TC.check_indexing(env)


def test_verdicts(env):
    TC.check_verdicts(env)


def test_misuse_and_bookkeeping(env):
    TC.check_misuse(env)


def test_pack_sweep_round_trip(env):
    TC.check_pack_sweep(env)


def test_long_cap_short_run(env):
    TC.check_long_cap(env, 600)


def test_traffic_script_update_equals_the_restatement(env, many):
    """TrafficScript.update and the test driver's per-actor ObstaclesFSM instances, fed the (s, v) sequence the
    many-actor run recorded, produce the same obstacle lists and light states."""
    mpcqp, TT = env["mpcqp"], env["TT"]
    d, dt = many["d"], env["solver"]().params.dt
    for b, script in enumerate(many["scripts"]):
        ts = TT.TrafficScript(script)
        fsms = [TC.shim_fsm(TT, mpcqp, a) for a in script]
        seen = 0
        for step in range(int(d["n_steps"][b])):
            s, v = d["hist_x"][b, step, 0], d["hist_x"][b, step, 4]
            obs, states = ts.update(dt, s, v)
            exp, green = TC.fsm_step(mpcqp, fsms, dt, s, v)
            assert [(o["s"], o["v"], o["type"]) for o in obs] == [(e[0], e[1], e[3]) for e in exp], (b, step)
            assert sum(1 << a for a, st in enumerate(states) if st == "GREEN") == green == d["hist_tl"][b, step]
            assert len(obs) == d["hist_nobs"][b, step]
            assert [st is None for st in states] == [a.kind == mpcqp.ACTOR_NONE for a in script]
            seen = max(seen, len(obs))
        assert seen == d["extra"][b, mpcqp.TRX_MAX_NOBS]
    names = many["names"]
    ts = TT.TrafficScript(many["scripts"][names.index("three_cars")])
    assert ts.update(dt, TC.S0, 9.0)[1][:3] == ["WAITING"] * 3
    with pytest.raises(ValueError):
        TT.TrafficScript([mpcqp.MpcActor()] * 17)
    with pytest.raises(ValueError):
        TT.TrafficScript([mpcqp.MpcActor(kind=5)])


def test_run_traffic_sweep(env, many):
    """run_traffic_sweep: scripts of different lengths (padded), None, a TrafficScript from an ObstaclesFSM; the
    rows equal Solver.closed_loop_traffic's and the verdict columns are run_scenario_sweep's."""
    mpcqp, TT, traj = env["mpcqp"], env["TT"], env["traj"]
    mpc = TT.TrajectoryTracker(traj, device=-1)
    mpc.N, mpc.sqp_iters = 20, 1
    fsm = TT.ObstaclesFSM(dynamic_obstacle=True, traffic_light=True)
    fsm.obs_trigger_s, fsm.obs_start_s, fsm.obs_end_s = TC.S0 + 35.0, TC.S0 + 70.0, TC.FAR
    fsm.tl_pos, fsm.tl_stop_duration = TC.S0 + 30.0, 1.0
    from_fsm = TT.TrafficScript.from_fsm(fsm)
    assert [a.kind for a in from_fsm.actors] == [mpcqp.ACTOR_CAR, mpcqp.ACTOR_LIGHT]
    assert (from_fsm.actors[0].pos_s, from_fsm.actors[1].pos_s) == (fsm.obs_start_s, fsm.tl_pos)
    three = many["scripts"][0][:3]
    scripts = [three, None, from_fsm, [mpcqp.light(TC.S0 + 30.0, 100.0, 1.0)]]
    x_init = SC.starts(traj, 4)
    r = TT.run_traffic_sweep(mpc, scripts, traj, x_init, max_steps=120, hist_egos=[2], s_stop=SC.S_STOP)
    assert r["quant"].shape == (4, 13) and r["extra"].shape == (4, 3) and r["hist_slab"].shape == (1, 120, 3, 2)
    rows = [TC.pad(mpcqp, s, 3) for s in (three, [], from_fsm.actors, scripts[3])]
    ref = mpc.solver(max_obs=0).closed_loop_traffic(x_init, rows, 120, s_stop=SC.S_STOP, hist_egos=[2])
    assert SC.same(r["quant"][:, TC.QCOLS], ref["quant"][:, TC.QCOLS]) and SC.same(r["extra"], ref["extra"])
    assert SC.same(r["hist_slab"], ref["hist_slab"]) and np.isfinite(r["hist_slab"]).any()
    sw = TT.run_scenario_sweep(mpc, [fsm], traj, x_init[2:3], max_steps=120, hist_egos=[0], s_stop=SC.S_STOP)
    assert SC.same(r["quant"][2, TC.QCOLS], sw["quant"][0, TC.QCOLS]) and SC.same(r["hist_x"], sw["hist_x"])
    assert r["verdicts"].shape == (4,) and r["on_road"].dtype == bool and r["counts"]["destination"] == 0
    assert np.isnan(r["quant"][1, 9]) and r["extra"][1].tolist() == [0.0, 0.0, -1.0]
    with pytest.raises(ValueError):
        TT.run_traffic_sweep(mpc, scripts[:2], traj, x_init, max_steps=10)
