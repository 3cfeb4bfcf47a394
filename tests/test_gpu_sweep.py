"""mpc_closed_loop_sweep on the device: ego b's loop is mpc_closed_loop's loop with scenario b, the check
quantities come from the FSM and plant kernels, histories exist only for the named egos.  The reference is
mpc_closed_loop on the same device (one ego, or one group of egos sharing a scenario, per call) and
shard.closed_loop_quantities on its full histories: bit for bit.  The solver settings are the tracker's
(the bench's closed-loop leg), like tests/test_gpu_closed_loop.py."""
import numpy as np
import pytest

import sweep_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import mpcqp
    import shard
    import trajectory_tracking as TT
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    trajs, solvers = {}, {}

    def solver(i, N):
        if i not in trajs:
            trajs[i] = TrajectoryLoader(builtin_trajectory(i))
        if (i, N) not in solvers:
            p = mpcqp.default_params(N=N, sqp_iters=TT.SQP_ITERS)
            solvers[(i, N)] = mpcqp.Solver(trajs[i].X_ref, trajs[i].U_ref, p, device=0)
        return trajs[i], solvers[(i, N)]

    yield dict(mpcqp=mpcqp, shard=shard, solver=solver)
    for s in solvers.values():
        s.close()


def test_seven_scenarios_equal_single_runs(env):
    """B = 7, N = 10, trajectory2: the six scenarios and one ego with both switches off, in one batch.  The
    both-off ego of this mixed batch is solved by the obstacle kernels with no obstacle, like an ego whose
    scenario is on but never triggers: that one-ego run is its reference.  Whether it also equals a run on the
    obstacle-free kernels is printed, not asserted."""
    traj, slv = env["solver"](2, 10)
    names, fsms = SC.scenarios(env["mpcqp"], both_off=True)
    x_init = SC.starts(traj, 7)
    ms = 300
    sw = slv.closed_loop_sweep(x_init, fsms, ms, s_stop=SC.S_STOP, hist_egos=range(7))
    never = fsms[names.index("never")]
    for b in range(7):
        r1 = SC.single_run(slv, x_init[b], never if names[b] == "off" else fsms[b], ms, SC.S_STOP)
        assert int(sw["n_steps"][b]) == int(r1["n_steps"][0]) and 0 < sw["n_steps"][b] < ms, names[b]
        SC.assert_history_row(sw, b, r1)
        SC.assert_quant_row(sw["quant"][b], SC.expected_quant(env["shard"], r1, fsms[b]))
    SC.assert_step_time_column(sw)
    by = dict(zip(names, range(7)))
    for k in ("car_a", "car_b", "both"):
        assert np.isfinite(sw["hist_obs_s"][by[k]]).any()
    for k in ("light_1s", "light_3s", "both"):
        assert sw["hist_tl"][by[k]].max() == 1
    for k in ("never", "off"):
        assert np.isnan(sw["quant"][by[k], 9]) and sw["quant"][by[k], 10] == 0
    r_off = SC.single_run(slv, x_init[by["off"]], None, ms, SC.S_STOP)
    print("both-off ego in a mixed batch == both-off run on the obstacle-free kernels:",
          SC.same(sw["hist_x"][by["off"]], r_off["hist_x"][0]) and SC.same(sw["hist_u"][by["off"]], r_off["hist_u"][0]))


def test_257_egos_five_scenario_types(env):
    """One ego past a 256-thread block, N = 5, 60 steps at most; the scenario types cycle and the starts are
    spread over the whole stretch, so egos leave at clearly different steps (the compaction runs).  Reference:
    one mpc_closed_loop call per scenario type over that type's egos."""
    traj, slv = env["solver"](2, 5)
    names, fsms = SC.scenarios(env["mpcqp"])
    types = [names.index(k) for k in ("car_a", "car_b", "light_1s", "both", "never")]
    B, ms = 257, 60
    x_init = SC.starts(traj, B, spread=(SC.S_STOP - SC.S0) / B)
    kind = np.arange(B) % 5
    keep = [0, 128, 256]
    sw = slv.closed_loop_sweep(x_init, [fsms[types[k]] for k in kind], ms, s_stop=SC.S_STOP, hist_egos=keep)
    assert len(set(sw["n_steps"].tolist())) >= 5 and sw["n_steps"].min() < 5 and sw["n_steps"].max() > 30
    cols = [1, 2, 3, 4, 5, 6, 7, 9, 10]
    for k in range(5):
        egos = np.flatnonzero(kind == k)
        f = fsms[types[k]]
        old = slv.closed_loop(x_init[egos], f, max_steps=ms, s_stop=SC.S_STOP)
        assert np.array_equal(sw["n_steps"][egos], old["n_steps"])
        q = env["shard"].closed_loop_quantities(old, 0, bool(f.dynamic_obstacle), bool(f.traffic_light), f.tl_pos)
        assert SC.same(sw["quant"][egos][:, cols], q[:, cols]), names[types[k]]
        code = old["hist_status"] & 15
        live = old["hist_status"] >= 0
        assert np.array_equal(sw["quant"][egos, 11], ((code == 2) & live).sum(1))
        assert np.array_equal(sw["quant"][egos, 12], ((code != 0) & live).sum(1))
        for row, b in enumerate(keep):
            if kind[b] == k:
                j = int(np.flatnonzero(egos == b)[0])
                SC.assert_history_row(sw, row, {n: v[j:j + 1] for n, v in old.items() if n.startswith("hist_")})
    SC.assert_step_time_column(sw)


def test_shared_sweep_equals_closed_loop(env):
    """B = 5, N = 20, trajectory1, no scenario: the setup of test_batch_equals_single_runs."""
    traj, slv = env["solver"](1, 20)
    rng = np.random.default_rng(5)
    x_init = np.column_stack([rng.uniform(0, 20, 5), rng.normal(0, 0.05, 5), np.zeros(5), np.zeros(5),
                              rng.uniform(0.5, 3, 5)])
    old = slv.closed_loop(x_init, None, max_steps=80, s_max=traj.s_max)
    sw = slv.closed_loop_sweep(x_init, None, 80, s_max=traj.s_max, hist_egos=range(5))
    assert np.array_equal(sw["n_steps"], old["n_steps"])
    for k in ("hist_x", "hist_u", "hist_obs_s"):
        assert SC.same(sw[k], old[k]), k
    assert np.array_equal(sw["hist_tl"], old["hist_tl"]) and np.array_equal(sw["hist_status"], old["hist_status"])
    assert np.array_equal(np.isnan(sw["step_ms"]), np.isnan(old["step_ms"]))
    q = env["shard"].closed_loop_quantities(old, 0, False, False, 0.0)
    cols = [0, 1, 2, 3, 4, 5, 6, 7, 9, 10]
    assert SC.same(sw["quant"][:, cols], q[:, cols])
    SC.assert_step_time_column(sw)


def test_long_cap_short_run(env):
    """B = 4096 (more than one 1024-lane compaction chunk), max_steps = 50 000, s_stop a few metres ahead and
    no history: the cap costs nothing (mpc_closed_loop would need about 14 GB of histories on each side for
    this call).  Eight egos are checked against one-ego mpc_closed_loop runs capped at 60 steps."""
    traj, slv = env["solver"](2, 5)
    names, fsms = SC.scenarios(env["mpcqp"])
    types = [names.index(k) for k in ("car_a", "car_b", "never")]
    B, s_stop = 4096, SC.S0 + 8.0
    x_init = SC.starts(traj, B, spread=6.0 / B)
    x_init[:, 4] = np.linspace(5.0, 9.0, B)
    scen = [fsms[types[b % 3]] for b in range(B)]
    sw = slv.closed_loop_sweep(x_init, scen, 50000, s_stop=s_stop)
    assert sw["hist_x"].shape[0] == 0 and sw["step_ms"].shape == (50000,)
    assert (sw["n_steps"] > 0).all() and (sw["n_steps"] < 60).all()
    assert np.isfinite(sw["step_ms"][:sw["n_steps"].max()]).all() and np.isnan(sw["step_ms"][64:]).all()
    for b in (0, 1, 2, 1023, 1024, 2500, 4094, 4095):
        r1 = SC.single_run(slv, x_init[b], scen[b], 60, s_stop)
        assert int(sw["n_steps"][b]) == int(r1["n_steps"][0])
        SC.assert_quant_row(sw["quant"][b], SC.expected_quant(env["shard"], r1, scen[b]))
    SC.assert_step_time_column(sw)


def test_verdicts_on_the_device(env):
    traj, slv = env["solver"](2, 5)
    x_init, fsms, s_stop = SC.verdict_case(env["mpcqp"], traj)
    sw = slv.closed_loop_sweep(x_init, fsms, 200, s_stop=s_stop)
    SC.check_verdict_case(env["mpcqp"], slv, traj, sw)
