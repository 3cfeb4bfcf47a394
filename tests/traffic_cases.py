"""Shared pieces of the traffic-script tests (test_traffic_cpu.py on the host backend, test_gpu_traffic.py on the
device): the scripts, a stepwise restatement of mpc_closed_loop_traffic built from pinned code, and the
comparisons.  Every comparison is bit for bit (sweep_cases.same): the references run the same solver kernels on
the same inputs.

The restatement (`driver`) keeps, per actor, one instance of the package's ObstaclesFSM shim (pinned to the
reference's golden histories by tests/test_fsm_golden.py) with exactly one switch on and that actor's fields.
Per step it updates the instances in actor order, concatenates their obstacle lists into a [B][A][2] slab, calls
Solver.solve_batch on a context with max_obs = A, and does the Euler step in numpy with k_ref from Solver.lookup.
The quantities and extras come from its full histories with numpy."""
import numpy as np

import sweep_cases as SC

S0 = SC.S0
A_MANY = 8
MAX_STEPS_MANY = 150
S_STOP_MANY = S0 + 80.0
FAR = 1.0e6
QCOLS = [1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12]     # every column but the ego id and the step time


def pad(mpcqp, actors, A):
    return list(actors) + [mpcqp.MpcActor() for _ in range(A - len(actors))]


def many_scripts(mpcqp):
    """The six scripts of the many-actor test, A = 8, placed ahead of S0 so that each does what its name says
    within MAX_STEPS_MANY steps.  Returns (names, scripts)."""
    car, light, none = mpcqp.car, mpcqp.light, mpcqp.MpcActor
    table = [
        # three cars, different triggers and speeds; the second reaches its end_s inside the run and vanishes
        ("three_cars", [car(S0 + 5.0, S0 + 40.0, 4.0, FAR), car(S0 + 10.0, S0 + 60.0, 6.0, S0 + 75.0),
                        car(S0 + 20.0, S0 + 90.0, 3.0, FAR)]),
        # two lights 30 m and 55 m ahead; the second shows only from 20 m on (with the preset's 100 m the ego,
        # standing 8 m before the first light when it turns GREEN, stays there for the rest of the run: every
        # later QP is infeasible on the host backend, so the second light would never be reached)
        ("two_lights", [light(S0 + 30.0, 100.0, 1.0), light(S0 + 55.0, 20.0, 0.6)]),
        # eight cars, all active from the first step on
        ("eight_cars", [car(S0 - 1.0, S0 + 30.0 + 6.0 * k, 5.0 + 0.5 * k, FAR) for k in range(8)]),
        # light, car, light, car with placeholders between them
        ("interleaved", [light(S0 + 30.0, 100.0, 2.0), none(), car(S0 + 35.0, S0 + 75.0, 7.0, FAR), none(),
                         light(S0 + 60.0, 20.0, 0.4), car(S0 + 40.0, S0 + 95.0, 6.0, FAR), none(), none()]),
        ("all_none", []),
        ("never", [car(FAR, S0 + 30.0, 4.0, FAR), light(FAR, 100.0, 1.0), car(FAR, S0 + 50.0, 2.0, FAR)]),
    ]
    return [n for n, _ in table], [pad(mpcqp, a, A_MANY) for _, a in table]


def shim_fsm(TT, mpcqp, actor):
    """The ObstaclesFSM shim restating one actor: exactly one switch on and that actor's fields (None for a
    placeholder)."""
    if actor.kind == mpcqp.ACTOR_CAR:
        f = TT.ObstaclesFSM(dynamic_obstacle=True, traffic_light=False)
        f.obs_trigger_s, f.obs_start_s, f.obs_v, f.obs_end_s = actor.trigger_s, actor.pos_s, actor.v, actor.end_s
        f.obs_s = f.obs_start_s
        return f
    if actor.kind == mpcqp.ACTOR_LIGHT:
        f = TT.ObstaclesFSM(dynamic_obstacle=False, traffic_light=True)
        f.tl_pos, f.tl_trigger_s, f.tl_stop_duration = actor.pos_s, actor.trigger_s, actor.stop_duration
        return f
    return None


def fsm_step(mpcqp, fsms, dt, s, v):
    """One step of an ego's per-actor shim instances, in actor order: ([(s, v, actor index, type)], green
    bitmask after the update)."""
    out, green = [], 0
    for a, f in enumerate(fsms):
        if f is None:
            continue
        obs, tl = f.update(dt, s, v)
        out += [(o["s"], o["v"], a, o["type"]) for o in obs]
        if f.traffic_light and tl == "GREEN":
            green |= 1 << a
    return out, green


def driver(TT, mpcqp, shard, slv_obs, x_init, scripts, max_steps, s_stop):
    """The stepwise restatement for B egos with a script each (all of one length A == slv_obs.params.max_obs).
    Returns closed_loop_traffic's dict with every ego's history kept (step_ms excepted, quant columns 0 and 8
    left at 0), plus 'green' [B, max_steps] per-step bitmasks for the callers' own assertions."""
    x = np.array(x_init, np.float64).reshape(-1, 5)
    B, A, dt = x.shape[0], len(scripts[0]), slv_obs.params.dt
    assert A == slv_obs.params.max_obs and all(len(s) == A for s in scripts)
    fsms = [[shim_fsm(TT, mpcqp, a) for a in scr] for scr in scripts]
    hx = np.full((B, max_steps + 1, 5), np.nan); hu = np.full((B, max_steps, 2), np.nan)
    hc = np.full((B, max_steps), np.nan); hl = np.full((B, max_steps, A, 2), np.nan)
    ht = np.full((B, max_steps), -1, np.int32); hs = np.full((B, max_steps), -1, np.int32)
    hn = np.full((B, max_steps), -1, np.int32)
    who = np.full((B, max_steps, A), -1, np.int32)           # actor behind each slab entry; cars only
    ns = np.zeros(B, np.int32)
    hx[:, 0] = x
    active = x[:, 0] <= s_stop
    for step in range(max_steps):
        idx = np.flatnonzero(active)
        if idx.size == 0:
            break
        slab = np.zeros((idx.size, A, 2)); nobs = np.zeros(idx.size, np.int32)
        for i, b in enumerate(idx):
            obs, green = fsm_step(mpcqp, fsms[b], dt, x[b, 0], x[b, 4])
            for j, (os_, ov, a, typ) in enumerate(obs):
                slab[i, j] = (os_, ov)
                if typ == "car":
                    who[b, step, j] = a
            nobs[i] = len(obs)
            cars = [o[0] for o in obs if o[3] == "car"]
            hc[b, step] = cars[0] if cars else np.nan
            ht[b, step], hn[b, step] = green, len(obs)
            hl[b, step, :len(obs)] = slab[i, :len(obs)]
        r = slv_obs.solve_batch(x[idx], slab, nobs)
        k_ref = slv_obs.lookup(x[idx, 0])[0][:, 3]
        for i, b in enumerate(idx):
            s, d, o, k, v = x[b]
            u = r["u0"][i]
            x[b] = x[b] + dt * np.array([v, v * o, v * (k - k_ref[i]), u[0], u[1]])
            hx[b, step + 1], hu[b, step], hs[b, step] = x[b], u, r["status"][i]
            ns[b] = step + 1
            if not x[b, 0] <= s_stop:
                active[b] = False
    out = dict(n_steps=ns, hist_x=hx, hist_u=hu, hist_car_s=hc, hist_tl=ht, hist_status=hs, hist_nobs=hn,
               hist_slab=hl, green=ht)
    out["quant"], out["extra"] = quantities(mpcqp, shard, out, who, scripts)
    return out


def quantities(mpcqp, shard, r, who, scripts):
    """quant [B,13] (columns 0 and 8 left at 0) and extra [B,3] from full histories: the plant-side columns by
    shard.closed_loop_quantities, the generalised ones (gap over every car, a pass per light) directly."""
    B = r["n_steps"].size
    plain = dict(r, hist_obs_s=r["hist_car_s"], step_ms=np.zeros(r["hist_u"].shape[1]))
    q11 = shard.closed_loop_quantities(plain, 0, False, False, 0.0)
    quant, extra = np.zeros((B, 13)), np.zeros((B, 3))
    quant[:, 1:8] = q11[:, 1:8]
    for b in range(B):
        n = int(r["n_steps"][b])
        s = r["hist_x"][b, :n + 1, 0]
        gap = np.where(who[b, :n] >= 0, r["hist_slab"][b, :n, :, 0] - s[:n, None], np.inf).ravel()
        if n and np.isfinite(gap).any():
            k = int(np.argmin(gap))                          # first occurrence: earliest step, then slab order
            quant[b, 9], extra[b, 2] = gap[k], who[b, :n].ravel()[k]
        else:
            quant[b, 9], extra[b, 2] = np.nan, -1.0
        for a, act in enumerate(scripts[b]):
            if act.kind != mpcqp.ACTOR_LIGHT:
                continue
            past = np.flatnonzero(s > act.pos_s)
            if past.size and past[0] < n and not (r["hist_tl"][b, past[0]] >> a) & 1:
                extra[b, 1] += 1.0
        quant[b, 10] = 1.0 if extra[b, 1] else 0.0
        extra[b, 0] = r["hist_nobs"][b, :n].max() if n else 0.0
        code = r["hist_status"][b, :n] & 15
        quant[b, 11], quant[b, 12] = (code == 2).sum(), (code != 0).sum()
    return quant, extra


def assert_case_shape(names, d, mpcqp):
    """The restatement itself shows what the many-actor case is for (a failure here means the inputs are wrong,
    not the library)."""
    by = dict(zip(names, range(len(names))))
    ns = d["n_steps"]
    assert (ns >= 20).all(), ns
    assert d["hist_nobs"][by["eight_cars"]].max() == 8
    b = by["three_cars"]
    assert d["hist_nobs"][b, :ns[b]].max() == 3
    # the vanishing car: it is in the slab (speed 6.0) at some step and gone at a later one
    has = (d["hist_slab"][b, :ns[b], :, 1] == 6.0).any(axis=1)
    assert has.any() and not has[np.flatnonzero(has)[-1] + 1:].any() and np.flatnonzero(has)[-1] < ns[b] - 1
    b = by["two_lights"]
    assert d["hist_tl"][b, ns[b] - 1] == 0b11, d["hist_tl"][b, :ns[b]]
    b = by["interleaved"]
    assert d["hist_tl"][b, :ns[b]].max() > 0 and np.isfinite(d["hist_car_s"][b, :ns[b]]).any()
    for k in ("all_none", "never"):
        assert d["hist_nobs"][by[k], :ns[by[k]]].max() == 0 and np.isnan(d["quant"][by[k], 9])


def assert_equals_driver(tr, d, rows=None):
    """Every output of closed_loop_traffic (history rows `rows` of tr against the driver's egos tr['hist_egos'])
    equals the restatement: histories, n_steps, quant without columns 0 and 8, extra."""
    egos = tr["hist_egos"] if rows is None else rows
    assert np.array_equal(tr["n_steps"], d["n_steps"])
    for k, b in enumerate(egos):
        for name in ("hist_x", "hist_u", "hist_car_s", "hist_slab"):
            assert SC.same(tr[name][k], d[name][b]), (name, b)
        for name in ("hist_tl", "hist_status", "hist_nobs"):
            assert np.array_equal(tr[name][k], d[name][b]), (name, b)
    assert SC.same(tr["quant"][:, QCOLS], d["quant"][:, QCOLS]), (tr["quant"], d["quant"])
    assert SC.same(tr["extra"], d["extra"]), (tr["extra"], d["extra"])


def assert_anchor(mpcqp, sw, tr, light_bit):
    """A traffic run of scripts made by actors_from_fsm against the sweep of the same scenarios and egos."""
    assert SC.same(tr["quant"][:, QCOLS], sw["quant"][:, QCOLS])
    assert np.array_equal(tr["n_steps"], sw["n_steps"])
    for k in ("hist_x", "hist_u"):
        assert SC.same(tr[k], sw[k]), k
    assert np.array_equal(tr["hist_status"], sw["hist_status"])
    assert SC.same(tr["hist_car_s"], sw["hist_obs_s"])
    bit = np.where(tr["hist_tl"] >= 0, (tr["hist_tl"] >> light_bit) & 1, -1)
    assert np.array_equal(bit, sw["hist_tl"])
    SC.assert_step_time_column(tr)


def anchor_scripts(mpcqp, fsms, padded):
    out = []
    for f in fsms:
        car, light = mpcqp.actors_from_fsm(f)
        none = mpcqp.MpcActor
        out.append([none(), car, none(), light, none()] if padded else [car, light])
    return out


def index_case(mpcqp, traj, B=257):
    """B egos spread over the stretch, A = 3, per-ego scripts cycling through five types."""
    car, light, none = mpcqp.car, mpcqp.light, mpcqp.MpcActor
    types = [
        [car(S0 + 10.0, S0 + 45.0, 4.0, FAR), none(), light(S0 + 50.0, 100.0, 0.4)],
        [light(S0 + 35.0, 100.0, 0.6), car(S0 + 5.0, S0 + 70.0, 3.0, FAR), car(S0 + 20.0, S0 + 90.0, 6.0, FAR)],
        [none(), none(), none()],
        [car(S0 - 1.0, S0 + 70.0, 2.0, FAR), car(S0 - 1.0, S0 + 80.0, 5.0, S0 + 95.0), none()],
        [light(FAR, 100.0, 1.0), car(FAR, S0, 1.0, FAR), none()],
    ]
    x_init = SC.starts(traj, B, spread=(SC.S_STOP - S0) / B)
    return x_init, [types[b % 5] for b in range(B)], types


def verdict_case(mpcqp, traj):
    """Two egos whose verdicts are fixed by construction: two lights, the second where the ego cannot stop for
    it (sweep_cases.verdict_case's placement); two cars, the second 0.5 m ahead at step 0."""
    s0, v0, dt = S0, 9.0, 0.2
    x_init = np.array([[s0, 0.0, 0.0, traj.get_state(s0)[3], v0]] * 2)
    scripts = [[mpcqp.light(FAR, 100.0, 1.0), mpcqp.light(s0 + 0.5 * v0 * dt, 100.0, 20.0)],
               [mpcqp.car(s0 - 1.0, s0 + 60.0, 9.0, FAR), mpcqp.car(s0 - 1.0, s0 + 0.5, 0.0, FAR)]]
    return x_init, scripts, s0 + 20.0


def check_verdict_case(mpcqp, slv, traj, tr):
    from sanity_checks import check_verdicts
    from shard import CL_FIELDS
    p = slv.params
    v, counts = slv.cl_verdicts(tr["quant"], traj.s_max)
    exp = [check_verdicts(dict(zip(CL_FIELDS, row[:11])), list(p.u_min), list(p.u_max), traj.s_max)
           for row in tr["quant"]]
    for b, e in enumerate(exp):
        for k, name in enumerate(mpcqp.CLV_NAMES):
            assert bool(v[b] & (1 << k)) == bool(e[name]), (b, name)
    assert counts.tolist() == [sum(bool(e[name]) for e in exp) for name in mpcqp.CLV_NAMES]
    assert (tr["n_steps"] >= 2).all()
    bit = {name: 1 << k for k, name in enumerate(mpcqp.CLV_NAMES)}
    assert tr["quant"][0, 10] == 1.0 and tr["extra"][0, mpcqp.TRX_N_RED_PASS] == 1.0
    assert not v[0] & bit["light_ok"] and v[0] & bit["obstacle_ok"]
    assert not v[1] & bit["obstacle_ok"] and tr["quant"][1, 9] <= 0.5
    assert tr["extra"][1, mpcqp.TRX_MIN_GAP_ACTOR] == 1.0 and v[1] & bit["light_ok"]


# ---------------------------------------------------------------------------------------------
# the test bodies shared by the host-backend and the device test files.  env: dict(mpcqp, shard, TT, traj,
# solver(max_obs=0) -> a Solver on trajectory2 with N = 20 on the backend under test)
# ---------------------------------------------------------------------------------------------
def check_anchor(env):
    """The seven sweep scenarios through actors_from_fsm, A = 2 and padded to A = 5, against the sweep."""
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"]()
    _, fsms = SC.scenarios(mpcqp, both_off=True)
    x_init = SC.starts(traj, 7)
    ms = 300
    sw = slv.closed_loop_sweep(x_init, fsms, ms, s_stop=SC.S_STOP, hist_egos=range(7))
    assert (sw["n_steps"] > 0).all() and np.isfinite(sw["hist_obs_s"]).any() and sw["hist_tl"].max() == 1
    for padded, light_bit in ((False, 1), (True, 3)):
        tr = slv.closed_loop_traffic(x_init, anchor_scripts(mpcqp, fsms, padded), ms, s_stop=SC.S_STOP,
                                     hist_egos=range(7))
        assert tr["hist_slab"].shape == (7, ms, 5 if padded else 2, 2)
        assert_anchor(mpcqp, sw, tr, light_bit)


def many_driver(env):
    """The many-actor case's restatement (computed once per test module), checked for what it is for."""
    mpcqp = env["mpcqp"]
    names, scripts = many_scripts(mpcqp)
    x_init = SC.starts(env["traj"], 6)
    d = driver(env["TT"], mpcqp, env["shard"], env["solver"](max_obs=A_MANY), x_init, scripts, MAX_STEPS_MANY,
               S_STOP_MANY)
    assert_case_shape(names, d, mpcqp)
    return dict(names=names, scripts=scripts, x_init=x_init, d=d)


def check_many(env, many):
    tr = env["solver"]().closed_loop_traffic(many["x_init"], many["scripts"], MAX_STEPS_MANY, s_stop=S_STOP_MANY,
                                             hist_egos=range(6))
    assert_equals_driver(tr, many["d"])
    assert np.array_equal(tr["quant"][:, 0], np.arange(6.0))
    SC.assert_step_time_column(tr)


def check_indexing(env):
    """B = 257, A = 3: the kept rows and sampled quant / extra rows equal one-ego traffic runs; a shared script
    equals the same script repeated per ego."""
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"]()
    B, ms = 257, 60
    x_init, scripts, types = index_case(mpcqp, traj, B)
    keep = (0, 63, 64, 255, 256)
    tr = slv.closed_loop_traffic(x_init, scripts, ms, s_stop=SC.S_STOP, hist_egos=keep)
    assert len(set(tr["n_steps"].tolist())) >= 5 and tr["n_steps"].min() < 5 and tr["n_steps"].max() > 30
    assert tr["extra"][:, 0].max() >= 2 and np.isfinite(tr["quant"][:, 9]).any()
    names = ("hist_x", "hist_u", "hist_car_s", "hist_slab", "hist_tl", "hist_status", "hist_nobs")
    for b in sorted(set(keep) | {1, 2, 3, 4, 62, 65, 127, 128, 129, 254}):
        r1 = slv.closed_loop_traffic(x_init[b], [scripts[b]], ms, s_stop=SC.S_STOP, hist_egos=[0])
        assert int(tr["n_steps"][b]) == int(r1["n_steps"][0]), b
        assert SC.same(tr["quant"][b, QCOLS], r1["quant"][0, QCOLS]), b
        assert SC.same(tr["extra"][b], r1["extra"][0]), b
        if b in keep:
            for name in names:
                assert SC.same(tr[name][keep.index(b)].astype(np.float64), r1[name][0].astype(np.float64)), (name, b)
    SC.assert_step_time_column(tr)
    x12 = SC.starts(traj, 12, spread=4.0)
    one = slv.closed_loop_traffic(x12, types[0], ms, s_stop=SC.S_STOP, hist_egos=range(12))
    rep = slv.closed_loop_traffic(x12, [types[0]] * 12, ms, s_stop=SC.S_STOP, hist_egos=range(12))
    for name in names + ("n_steps", "extra"):
        assert SC.same(one[name].astype(np.float64), rep[name].astype(np.float64)), name
    assert SC.same(one["quant"][:, QCOLS], rep["quant"][:, QCOLS]) and np.isfinite(one["hist_car_s"]).any()


def check_verdicts(env):
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"]()
    x_init, scripts, s_stop = verdict_case(mpcqp, traj)
    tr = slv.closed_loop_traffic(x_init, scripts, 200, s_stop=s_stop)
    check_verdict_case(mpcqp, slv, traj, tr)


def check_misuse(env):
    """Every misuse case of include/mpcqp.h is MPC_E_ARG with a message; B == 0 succeeds; the version."""
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"]()
    L = mpcqp.lib()
    assert L.mpc_version() == 5
    B, A = 3, 2
    x = np.ascontiguousarray(SC.starts(traj, B))
    arr = (mpcqp.MpcActor * (B * A))(*([mpcqp.car(S0 + 5.0, S0 + 40.0, 4.0, FAR), mpcqp.light(S0 + 30.0, 100.0, 1.0)] * B))
    bad = (mpcqp.MpcActor * (B * A))(*arr)
    bad[3].kind = 3
    neg = (mpcqp.MpcActor * (B * A))(*arr)
    neg[0].kind = -1
    quant = np.empty((B, 13))
    hx = np.empty((2, 11, 5)); hl = np.empty((2, 10, A, 2))

    def call(B=B, actors=arr, A=A, n_scripts=B, q=quant, n_hist=0, egos=None, hist_x=None, hist_slab=None):
        he = None if egos is None else np.asarray(egos, np.int32)
        rc = L.mpc_closed_loop_traffic(slv.h, B, mpcqp._p(x), actors, A, n_scripts, 10, SC.S_STOP, mpcqp._p(q), None,
                                       n_hist, mpcqp._pi(he), mpcqp._p(hist_x), None, None, None, None, None,
                                       mpcqp._p(hist_slab), None, None)
        return rc, mpcqp.last_error()

    assert call()[0] == 0                                        # the well-formed call these cases depart from
    for kw in (dict(A=-1), dict(A=17), dict(n_scripts=2), dict(n_scripts=0), dict(actors=None, n_scripts=1),
               dict(actors=None, n_scripts=B), dict(actors=None, n_scripts=0), dict(actors=bad), dict(actors=neg),
               dict(q=None), dict(n_hist=-1), dict(n_hist=0, hist_x=hx), dict(n_hist=0, hist_slab=hl),
               dict(actors=None, A=0, n_scripts=0, n_hist=2, egos=[0, 1], hist_slab=hl),
               dict(n_hist=2, egos=[1, B], hist_x=hx), dict(n_hist=2, egos=[-1, 2], hist_x=hx),
               dict(n_hist=2, egos=[1, 1], hist_x=hx)):
        rc, msg = call(**kw)
        assert rc == -1 and msg, kw
    assert call(actors=None, A=0, n_scripts=0)[0] == 0 and call(n_scripts=1)[0] == 0
    assert call(n_hist=2, egos=[2, 0], hist_x=hx, hist_slab=hl)[0] == 0
    assert call(B=0, n_scripts=0, actors=None, A=0)[0] == 0 and call(B=0, n_scripts=1)[0] == 0
    r0 = slv.closed_loop_traffic(np.empty((0, 5)), None, 10, s_stop=SC.S_STOP)
    assert r0["quant"].shape == (0, 13) and r0["extra"].shape == (0, 3)
    # no script at all: the obstacle-free run of the sweep without scenarios
    tr = slv.closed_loop_traffic(x, None, 40, s_stop=SC.S_STOP, hist_egos=[1], lo=100)
    sw = slv.closed_loop_sweep(x, None, 40, s_stop=SC.S_STOP, hist_egos=[1])
    assert SC.same(tr["quant"][:, QCOLS], sw["quant"][:, QCOLS]) and SC.same(tr["hist_x"], sw["hist_x"])
    assert tr["quant"][:, 0].tolist() == [100.0, 101.0, 102.0] and tr["hist_slab"].shape == (1, 40, 0, 2)
    assert (tr["extra"] == [0.0, 0.0, -1.0]).all()


def check_pack_sweep(env):
    """shard.pack_sweep takes a traffic result as it stands and round-trips through unpack_closed_loop."""
    mpcqp, shard, traj, slv = env["mpcqp"], env["shard"], env["traj"], env["solver"]()
    _, scripts = many_scripts(mpcqp)
    x_init = SC.starts(traj, 6)
    ms, rows, he = 40, 8, 2
    tr = slv.closed_loop_traffic(x_init, scripts, ms, s_stop=S_STOP_MANY, hist_egos=[4, 2], lo=10)
    q, hist = shard.unpack_closed_loop(shard.pack_sweep(tr, rows, he, ms), rows, he, ms)
    assert SC.same(q, tr["quant"][:, :11]) and q[:, 0].tolist() == [10.0 + b for b in range(6)]
    assert hist.shape == (he, ms, shard.HIST_COLS)
    assert SC.same(hist[:, :, :5], tr["hist_x"][:, 1:].astype(np.float32))
    assert SC.same(hist[:, :, 5:], tr["hist_u"].astype(np.float32))


def check_long_cap(env, B):
    """max_steps = 50 000 with a stop a few metres ahead and no history: allocates and returns; a few egos are
    checked against one-ego runs capped at 60 steps."""
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"]()
    _, scripts, _ = index_case(mpcqp, traj, B)
    s_stop = S0 + 8.0
    x_init = SC.starts(traj, B, spread=6.0 / B)
    x_init[:, 4] = np.linspace(5.0, 9.0, B)
    tr = slv.closed_loop_traffic(x_init, scripts, 50000, s_stop=s_stop)
    assert tr["hist_x"].shape[0] == 0 and tr["step_ms"].shape == (50000,)
    assert (tr["n_steps"] > 0).all() and (tr["n_steps"] < 60).all()
    assert np.isfinite(tr["step_ms"][:tr["n_steps"].max()]).all() and np.isnan(tr["step_ms"][64:]).all()
    for b in (0, 1, B // 2, B - 1):
        r1 = slv.closed_loop_traffic(x_init[b], [scripts[b]], 60, s_stop=s_stop)
        assert int(tr["n_steps"][b]) == int(r1["n_steps"][0])
        assert SC.same(tr["quant"][b, QCOLS], r1["quant"][0, QCOLS]) and SC.same(tr["extra"][b], r1["extra"][0])
    SC.assert_step_time_column(tr)
