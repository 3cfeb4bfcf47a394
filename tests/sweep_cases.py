"""Shared pieces of the scenario-sweep tests (test_sweep_cpu.py on the host backend, test_gpu_sweep.py on the
device): the scenario set, one-ego mpc_closed_loop reference runs, and the comparisons.

The reference for every sweep result is the library's own mpc_closed_loop with that ego's scenario, and
shard.closed_loop_quantities on its full histories: bit for bit (np.array_equal, NaN positions equal)."""
import numpy as np

S0 = 440.0            # trajectory2: the existing closed-loop tests' start before the light
S_STOP = S0 + 60.0    # a few tens of metres: the events below all lie inside


def scenarios(mpcqp, both_off=False):
    """The six scenarios of the sweep tests, placed just ahead of S0 so that each switches within a short run
    (car only with two speeds / start positions; light only with two stop durations; both; switched on but
    never triggering), plus optionally one with both switches off.  Returns (names, [MpcFsm])."""
    far = 1.0e6
    car = dict(dynamic_obstacle=1, obs_end_s=far)
    light = dict(traffic_light=1, tl_pos=S0 + 30.0, tl_trigger_s=100.0)
    table = [
        ("car_a", dict(car, obs_trigger_s=S0 + 10.0, obs_start_s=S0 + 40.0, obs_v=4.0)),
        ("car_b", dict(car, obs_trigger_s=S0 + 5.0, obs_start_s=S0 + 30.0, obs_v=2.0)),
        ("light_1s", dict(light, tl_stop_duration=1.0)),
        ("light_3s", dict(light, tl_stop_duration=3.0)),
        ("both", dict(car, **light, obs_trigger_s=S0 + 35.0, obs_start_s=S0 + 70.0, obs_v=4.0, tl_stop_duration=1.0)),
        ("never", dict(dynamic_obstacle=1, traffic_light=1, obs_trigger_s=far, tl_pos=far, tl_trigger_s=100.0)),
    ]
    if both_off:
        table.append(("off", dict()))
    return [n for n, _ in table], [mpcqp.default_fsm(**kw) for _, kw in table]


def starts(traj, n, v=9.0, spread=1.0):
    """n start states on the reference line of `traj` (a TrajectoryLoader) from S0 on, `spread` metres apart,
    with a small lateral offset that differs per ego."""
    s = S0 + spread * np.arange(n)
    return np.array([[si, 0.01 * (i % 3), 0.0, traj.get_state(si)[3], v] for i, si in enumerate(s)])


def single_run(slv, x0, fsm, max_steps, s_stop):
    """One-ego mpc_closed_loop with this scenario (None: no scenario)."""
    return slv.closed_loop(np.asarray(x0).reshape(1, 5), fsm, max_steps=max_steps, s_stop=s_stop)


def same(a, b):
    """Bit-for-bit equality of float arrays, NaN positions included."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def assert_history_row(sw, k, r1):
    """Row k of a sweep's histories == the one-ego run r1 (all of it: the NaN / -1 tails too)."""
    assert same(sw["hist_x"][k], r1["hist_x"][0])
    assert same(sw["hist_u"][k], r1["hist_u"][0])
    assert same(sw["hist_obs_s"][k], r1["hist_obs_s"][0])
    assert np.array_equal(sw["hist_tl"][k], r1["hist_tl"][0])
    assert np.array_equal(sw["hist_status"][k], r1["hist_status"][0])


def expected_quant(shard, r1, fsm):
    """The 13 columns for one ego from its one-ego run: shard.closed_loop_quantities on the full histories
    (columns 0-10; 0 and 8 are compared separately by the callers) and the two status counters."""
    on = (0, 0, 0.0) if fsm is None else (fsm.dynamic_obstacle, fsm.traffic_light, fsm.tl_pos)
    q = shard.closed_loop_quantities(r1, 0, bool(on[0]), bool(on[1]), on[2])[0]
    n = int(r1["n_steps"][0])
    code = r1["hist_status"][0, :n] & 15
    return np.concatenate([q, [float((code == 2).sum()), float((code != 0).sum())]])


def assert_quant_row(row, exp):
    """Every column but the ego id (0) and the step time (8, a wall-clock measurement of another run)."""
    cols = [1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12]
    assert same(row[cols], exp[cols]), (row, exp)


def assert_step_time_column(sw):
    """Column 8 == max(step_ms[:n]) of the sweep's own step times, exactly (0 for an ego that never ran)."""
    for b, n in enumerate(sw["n_steps"]):
        exp = np.max(sw["step_ms"][:n]) if n else 0.0
        assert same(sw["quant"][b, 8], exp)


def verdict_case(mpcqp, traj):
    """Four egos whose verdicts are fixed by construction, whatever the controller does."""
    s0, v0, dt = S0, 9.0, 0.2
    x_init = np.array([[s0, 0.0, 0.0, traj.get_state(s0)[3], v0]] * 4)
    x_init[3] = list(traj.get_state(s0)[:5])          # on the reference, no scenario
    fsms = [mpcqp.default_fsm(dynamic_obstacle=1, obs_trigger_s=s0 - 1.0, obs_start_s=s0 + 0.5, obs_v=0.0,
                              obs_end_s=1.0e6),                                 # a car 0.5 m ahead at step 0
            mpcqp.default_fsm(traffic_light=1, tl_pos=s0 + 0.5 * v0 * dt),      # a light the ego cannot stop for
            mpcqp.default_fsm(),
            mpcqp.default_fsm()]
    return x_init, fsms, s0 + 20.0


def check_verdict_case(mpcqp, slv, traj, sw):
    from sanity_checks import check_verdicts
    from shard import CL_FIELDS
    p = slv.params
    v, counts = slv.cl_verdicts(sw["quant"], traj.s_max)
    exp = [check_verdicts(dict(zip(CL_FIELDS, row[:11])), list(p.u_min), list(p.u_max), traj.s_max)
           for row in sw["quant"]]
    for b, e in enumerate(exp):
        for k, name in enumerate(mpcqp.CLV_NAMES):
            assert bool(v[b] & (1 << k)) == bool(e[name]), (b, name)
    assert counts.tolist() == [sum(bool(e[name]) for e in exp) for name in mpcqp.CLV_NAMES]
    assert (sw["n_steps"] >= 2).all()
    bit = {name: 1 << k for k, name in enumerate(mpcqp.CLV_NAMES)}
    assert not v[0] & bit["obstacle_ok"] and sw["quant"][0, 9] <= 0.5
    assert sw["quant"][1, 10] == 1.0 and not v[1] & bit["light_ok"]
    assert not (v & bit["destination"]).any() and not (v & bit["passed"]).any()
    assert v[3] == bit["passed"] - 1 - bit["destination"]      # unperturbed: everything but the destination
