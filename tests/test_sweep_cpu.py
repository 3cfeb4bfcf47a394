"""mpc_closed_loop_sweep and mpc_cl_verdicts on the host backend (device = -1): a scenario per ego, the check
quantities accumulated while the loop runs, histories for the named egos only.  The reference throughout is
the library's mpc_closed_loop, one ego and one scenario per call, and shard.closed_loop_quantities /
sanity_checks.check_verdicts on its full histories: bit for bit."""
import numpy as np
import pytest

import sweep_cases as SC

N = 5
MAX_STEPS = 400


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import mpcqp
    import shard
    import trajectory_tracking as TT
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    traj = TrajectoryLoader(builtin_trajectory(2))
    slv = mpcqp.Solver(traj.X_ref, traj.U_ref, mpcqp.default_params(N=N), device=-1)
    yield dict(mpcqp=mpcqp, shard=shard, TT=TT, traj=traj, slv=slv)
    slv.close()


@pytest.fixture(scope="module")
def six(env):
    """The six-scenario sweep with every ego's history kept, and the six one-ego reference runs (shared,
    read-only)."""
    names, fsms = SC.scenarios(env["mpcqp"])
    x_init = SC.starts(env["traj"], 6)
    sw = env["slv"].closed_loop_sweep(x_init, fsms, MAX_STEPS, s_stop=SC.S_STOP, hist_egos=range(6))
    singles = [SC.single_run(env["slv"], x_init[b], fsms[b], MAX_STEPS, SC.S_STOP) for b in range(6)]
    return dict(names=names, fsms=fsms, x_init=x_init, sw=sw, singles=singles)


def test_shared_scenario_equals_closed_loop(env):
    """n_fsm = 1 (the trajectory2 preset, both on), the two existing trajectory2 starts and a perturbed one,
    all selected: n_steps, every history and step_ms' NaN pattern are mpc_closed_loop's."""
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["slv"]
    fsm = mpcqp.default_fsm(dynamic_obstacle=1, traffic_light=1)
    x_init = np.array([[440.0, 0.0, 0.0, traj.get_state(440.0)[3], 9.0],
                       [690.0, 0.02, 0.0, traj.get_state(690.0)[3], 8.0],
                       [441.0, -0.03, 0.01, traj.get_state(441.0)[3], 8.5]])
    old = slv.closed_loop(x_init, fsm, max_steps=600, s_stop=730.0)
    sw = slv.closed_loop_sweep(x_init, fsm, 600, s_stop=730.0, hist_egos=[0, 1, 2])
    assert np.array_equal(sw["n_steps"], old["n_steps"]) and 0 < old["n_steps"].min() and old["n_steps"].max() < 600
    for k in ("hist_x", "hist_u", "hist_obs_s"):
        assert SC.same(sw[k], old[k]), k
    assert np.array_equal(sw["hist_tl"], old["hist_tl"]) and np.array_equal(sw["hist_status"], old["hist_status"])
    assert np.array_equal(np.isnan(sw["step_ms"]), np.isnan(old["step_ms"]))
    # both state machines switched in this run: the light went GREEN for ego 0, the car appeared for ego 1
    assert old["hist_tl"][0].max() == 1 and np.isfinite(old["hist_obs_s"][1]).any()
    q = env["shard"].closed_loop_quantities(old, 0, True, True, fsm.tl_pos)
    cols = [0, 1, 2, 3, 4, 5, 6, 7, 9, 10]
    assert SC.same(sw["quant"][:, cols], q[:, cols])
    SC.assert_step_time_column(sw)


def test_per_ego_scenarios_equal_single_runs(env, six):
    sw, singles, fsms = six["sw"], six["singles"], six["fsms"]
    assert np.array_equal(sw["quant"][:, 0], np.arange(6.0))
    for b in range(6):
        assert int(sw["n_steps"][b]) == int(singles[b]["n_steps"][0]) and 0 < sw["n_steps"][b] < MAX_STEPS
        SC.assert_history_row(sw, b, singles[b])
        SC.assert_quant_row(sw["quant"][b], SC.expected_quant(env["shard"], singles[b], fsms[b]))
    SC.assert_step_time_column(sw)
    # the scenarios did what their names say, so the comparisons above covered the transitions
    by = dict(zip(six["names"], range(6)))
    for k in ("car_a", "car_b", "both"):
        assert np.isfinite(sw["hist_obs_s"][by[k]]).any() and np.isfinite(sw["quant"][by[k], 9])
    for k in ("light_1s", "light_3s", "both"):
        assert sw["hist_tl"][by[k]].max() == 1
    assert sw["n_steps"][by["light_3s"]] > sw["n_steps"][by["light_1s"]]
    assert not np.array_equal(sw["hist_obs_s"][by["car_a"]], sw["hist_obs_s"][by["car_b"]])
    assert np.isnan(sw["hist_obs_s"][by["never"]]).all() and np.isnan(sw["quant"][by["never"], 9])
    assert sw["hist_tl"][by["never"], :sw["n_steps"][by["never"]]].max() == 0


def test_verdicts_are_not_all_pass(env):
    x_init, fsms, s_stop = SC.verdict_case(env["mpcqp"], env["traj"])
    sw = env["slv"].closed_loop_sweep(x_init, fsms, 200, s_stop=s_stop)
    SC.check_verdict_case(env["mpcqp"], env["slv"], env["traj"], sw)


def test_selection(env, six):
    mpcqp, slv, full = env["mpcqp"], env["slv"], six["sw"]
    sw = slv.closed_loop_sweep(six["x_init"], six["fsms"], MAX_STEPS, s_stop=SC.S_STOP, hist_egos=[4, 1])
    assert sw["hist_egos"].tolist() == [4, 1] and sw["hist_x"].shape == (2, MAX_STEPS + 1, 5)
    for k, b in enumerate((4, 1)):
        for name in ("hist_x", "hist_u", "hist_obs_s", "hist_tl", "hist_status"):
            assert SC.same(sw[name][k].astype(np.float64), full[name][b].astype(np.float64)), (name, b)
    cols = [c for c in range(13) if c != 8]
    assert SC.same(sw["quant"][:, cols], full["quant"][:, cols]) and np.array_equal(sw["n_steps"], full["n_steps"])
    # n_hist = 0 with every history NULL, and n_steps / step_ms NULL
    arr = (mpcqp.MpcFsm * 6)(*six["fsms"])
    quant = np.empty((6, 13))
    x = np.ascontiguousarray(six["x_init"])
    rc = mpcqp.lib().mpc_closed_loop_sweep(slv.h, 6, mpcqp._p(x), arr, 6, MAX_STEPS, SC.S_STOP, mpcqp._p(quant), 0,
                                           None, None, None, None, None, None, None, None)
    assert rc == 0, mpcqp.last_error()
    assert SC.same(quant[:, cols], full["quant"][:, cols])
    assert np.array_equal(quant[:, 1], full["n_steps"].astype(np.float64))
    # the Python entry with a shard offset and no history
    sw0 = slv.closed_loop_sweep(six["x_init"][:2], six["fsms"][:2], MAX_STEPS, s_stop=SC.S_STOP, lo=100)
    assert sw0["quant"][:, 0].tolist() == [100.0, 101.0] and sw0["hist_x"].shape[0] == 0


def test_misuse(env, six):
    mpcqp, slv = env["mpcqp"], env["slv"]
    L = mpcqp.lib()
    B = 6
    x = np.ascontiguousarray(six["x_init"])
    arr = (mpcqp.MpcFsm * B)(*six["fsms"])
    quant = np.empty((B, 13))
    hx = np.empty((2, 11, 5))

    def call(fsm=arr, n_fsm=B, q=quant, n_hist=0, egos=None, hist_x=None):
        he = None if egos is None else np.asarray(egos, np.int32)
        rc = L.mpc_closed_loop_sweep(slv.h, B, mpcqp._p(x), fsm, n_fsm, 10, SC.S_STOP, mpcqp._p(q), n_hist,
                                     mpcqp._pi(he), mpcqp._p(hist_x), None, None, None, None, None, None)
        return rc, mpcqp.last_error()

    assert call()[0] == 0                                        # the well-formed call these cases depart from
    for kw in (dict(n_fsm=3), dict(n_fsm=0), dict(fsm=None, n_fsm=1), dict(fsm=None, n_fsm=B),
               dict(q=None), dict(n_hist=-1), dict(n_hist=0, hist_x=hx),
               dict(n_hist=2, egos=[1, B], hist_x=hx), dict(n_hist=2, egos=[-1, 2], hist_x=hx),
               dict(n_hist=2, egos=[3, 3], hist_x=hx)):
        rc, msg = call(**kw)
        assert rc == -1 and msg, kw
    assert call(fsm=None, n_fsm=0)[0] == 0 and call(n_fsm=1)[0] == 0


def test_shard_path(env):
    """pack_sweep -> unpack_closed_loop -> closed_loop_report on a sweep == the report from mpc_closed_loop's
    result (shared scenario).  The step-time column is a wall-clock measurement of two separate runs and is
    left out; everything else, the verdict counts included, is equal."""
    mpcqp, shard, traj, slv = env["mpcqp"], env["shard"], env["traj"], env["slv"]
    fsm = mpcqp.default_fsm(dynamic_obstacle=1, traffic_light=1, tl_pos=SC.S0 + 30.0, tl_stop_duration=1.0,
                            obs_trigger_s=SC.S0 + 35.0, obs_start_s=SC.S0 + 70.0)
    x_init = SC.starts(traj, 5, spread=7.0)
    ms, rows, he = 300, 8, 2
    old = slv.closed_loop(x_init, fsm, max_steps=ms, s_stop=SC.S_STOP)
    q_old = shard.closed_loop_quantities(old, 10, True, True, fsm.tl_pos)
    sw = slv.closed_loop_sweep(x_init, fsm, ms, s_stop=SC.S_STOP, hist_egos=range(he), lo=10)
    p = slv.params
    args = (rows, he, ms, list(p.u_min), list(p.u_max), traj.s_max)
    r_old = shard.closed_loop_report([shard.pack_closed_loop(q_old, old, rows, he, ms)], *args)
    r_new = shard.closed_loop_report([shard.pack_sweep(sw, rows, he, ms)], *args)
    for k in ("egos", "ranks", "ego_steps", "checks_passed"):
        assert r_old[k] == r_new[k], k
    assert SC.same(r_old["hist"], r_new["hist"]) and r_new["hist"].shape[0] == he
    cols = [c for c in range(11) if c != 8]
    assert SC.same(r_old["quantities"][:, cols], r_new["quantities"][:, cols])
    assert len(set(old["n_steps"].tolist())) >= 3


def test_scenario_grid_and_run(env):
    TT, traj = env["TT"], env["traj"]
    base = TT.ObstaclesFSM(dynamic_obstacle=True, traffic_light=False)
    base.obs_trigger_s, base.obs_start_s, base.obs_end_s = SC.S0 + 5.0, SC.S0 + 35.0, 1.0e6
    grid = TT.scenario_grid(base, obs_v=[2.0, 4.0], obs_start_s=[SC.S0 + 30.0, SC.S0 + 40.0])
    # itertools.product order: the last axis varies fastest
    assert [(f.obs_v, f.obs_start_s) for f in grid] == [(2.0, SC.S0 + 30.0), (2.0, SC.S0 + 40.0),
                                                         (4.0, SC.S0 + 30.0), (4.0, SC.S0 + 40.0)]
    assert all(f.obs_trigger_s == SC.S0 + 5.0 and f.dynamic_obstacle and f is not base for f in grid)
    with pytest.raises(ValueError):
        TT.scenario_grid(base, no_such_field=[1])
    mpc = TT.TrajectoryTracker(traj, device=-1)
    mpc.N, mpc.sqp_iters = N, 1
    x_init = np.tile(SC.starts(traj, 1), (4, 1))
    r = TT.run_scenario_sweep(mpc, grid, traj, x_init, max_steps=MAX_STEPS, hist_egos=[3], s_stop=SC.S_STOP)
    assert r["quant"].shape == (4, 13) and r["verdicts"].shape == (4,) and r["hist_x"].shape[0] == 1
    slv = mpc.solver(max_obs=0)
    for b, f in enumerate(grid):
        r1 = SC.single_run(slv, x_init[b], TT.fsm_params(f), MAX_STEPS, SC.S_STOP)
        SC.assert_quant_row(r["quant"][b], SC.expected_quant(env["shard"], r1, TT.fsm_params(f)))
    SC.assert_history_row(r, 0, SC.single_run(slv, x_init[3], TT.fsm_params(grid[3]), MAX_STEPS, SC.S_STOP))
    # same start, four different cars: four different runs
    assert len({tuple(row[[2, 9]]) for row in r["quant"]}) == 4
    assert r["counts"]["destination"] == 0 and not r["passed"].any() and r["on_road"].dtype == bool
    # None entries: no scenario at all
    r0 = TT.run_scenario_sweep(mpc, [None, None], traj, x_init[:2], max_steps=MAX_STEPS, s_stop=SC.S_STOP)
    assert np.isnan(r0["quant"][:, 9]).all() and (r0["quant"][:, 10] == 0).all()
