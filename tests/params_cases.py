"""Shared pieces of the non-default-parameter tests (test_params_cpu.py on the oracle and the host backend,
test_gpu_params.py on the device): the parameter sets and the reference's records under them
(tests/golden/params_golden.npz, written by tests/golden/make_goldens.py --only params), and the checks both files
run through the library's C ABI.

A parameter set is a dict of the mpc_params fields that differ from mpc_default_params; the sets are read from the
fixture, so the tests and the reference's records cannot drift apart.  A and B move every field, in opposite
directions; W, U, G and T move one group each (weights, control bounds, geometry, dt), so a failure under one of
them names its group."""
import functools
import json

import numpy as np

from conftest import load_golden, traj_arrays

KNOBS = dict(brake_distance=25.0, brake_accel=-3.5)      # the warm start's knobs, which the reference hard-codes


@functools.lru_cache(maxsize=None)
def _golden():
    return load_golden("params_golden")


def sets():
    """name -> parameter set, in the fixture's order."""
    return json.loads(str(_golden()["sets_json"]))


SET_NAMES = ("A", "B", "W", "U", "G", "T")


def rho():
    return float(_golden()["rho"])


def frozen(pset):
    """A parameter set as a hashable tuple of (field, value) (test_gpu_horizons.oracle_solve caches on it)."""
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in pset.items()))


@functools.lru_cache(maxsize=None)
def cases(name, kind):
    """The records of set `name`; kind: 'qp', 'model' or 'warmstart' (the formats of qp_golden, model_golden and
    warmstart_golden)."""
    g = _golden()
    out = []
    for j in range(int(g[f"{name}_{kind}_n"])):
        pre = f"{name}_{kind}_c{j}_"
        out.append({k[len(pre):]: v for k, v in g.items() if k.startswith(pre)})
    return out


def slab(c):
    """(obs [1, M, 2] | None, n_obs [1] | None, M) of one record."""
    o = np.asarray(c["obs"], np.float64).reshape(-1, 2)
    if len(o) == 0:
        return None, None, 0
    return o[None], np.array([len(o)], np.int32), len(o)


class Library:
    """libmpcqp contexts on one device (-1: the host backend), one per trajectory, re-parameterised per call."""

    def __init__(self, mpcqp, device):
        self.mpcqp, self.device, self._ctx = mpcqp, device, {}

    def ctx(self, traj):
        if traj not in self._ctx:
            self._ctx[traj] = self.mpcqp.Solver(*traj_arrays(traj), self.mpcqp.default_params(), device=self.device)
        return self._ctx[traj]

    def run(self, c, pset, ubar=None, **kw):
        """One record's instance under `pset` and the solver knobs kw; ubar None: the library's warm start."""
        obs, n, mo = slab(c)
        slv = self.ctx(int(c["traj"]))
        slv.set_params(self.mpcqp.default_params(N=int(c["N"]), max_obs=mo, **pset, **kw))
        ub = None if ubar is None else np.asarray(ubar, np.float64).reshape(1, -1, 2)
        r = slv.solve_batch(np.asarray(c["x0"], np.float64)[None], obs, n, ubar=ub)
        return {k: v[0] for k, v in r.items()}

    def close(self):
        for s in self._ctx.values():
            s.close()
        self._ctx.clear()


# ---------------------------------------------------------------------------------------------
# the three golden checks of the library (device = -1 and device = 0)
# ---------------------------------------------------------------------------------------------
def check_warm_start(side, name):
    """sqp_iters = 0 returns the reference's u_init under the set, bit for bit (its s_curr += v dt stepping and the
    obstacle at the brake threshold depend on dt)."""
    pset = sets()[name]
    braking = 0
    for j, c in enumerate(cases(name, "warmstart")):
        r = side.run(c, pset, sqp_iters=0)
        assert np.array_equal(r["U"].ravel(), c["ubar"]), (name, j, c["x0"], c["obs"])
        assert r["status"] == 0 and r["iters"] == 0
        braking += int((c["ubar"][1::2] == -2.0).any())
    assert 0 < braking < len(cases(name, "warmstart"))


def check_predict(side, name):
    """Xpred at a given U with sqp_iters = 0 is the reference's predict() under the set, bit for bit."""
    pset = sets()[name]
    for j, c in enumerate(cases(name, "model")):
        r = side.run(dict(c, obs=np.zeros((0, 2))), pset, ubar=c["U"], sqp_iters=0)
        assert np.array_equal(r["Xpred"], c["X"]), (name, j)


def check_qp_solution(solve, oracles, name, tol, label):
    """solve(c, pset) -> (U flat, status) at the golden's ubar, against the KKT-certified optimum of the reference's
    QP under the set: within tol on every case; the statuses by the rule of
    test_oracle_golden.test_qp_solution_vs_certified_golden.  Returns the worst error."""
    from test_oracle_golden import golden_violation, params
    pset = sets()[name]
    worst, nfeas, nel = 0.0, 0, 0
    for j, c in enumerate(cases(name, "qp")):
        assert bool(c["ok_elastic"])
        U, status = solve(c, pset)
        err = float(np.abs(U - c["U_elastic"]).max())
        worst = max(worst, err)
        assert err <= tol, (label, name, j, int(c["N"]), err, status, json.loads(str(c["fdcheck"])))
        viol = golden_violation(oracles[int(c["traj"])], params(c["N"], c["obs"].shape[0], pset, elastic_rho=rho()), c)
        if bool(c["feasible"]):
            nfeas += 1
            assert status == 0, (label, name, j, status)
        elif viol > 1e-5:
            nel += 1
            assert status == 2, (label, name, j, status, viol)
        else:
            assert status in (0, 2), (label, name, j, status, viol)
    print(f"{label} set {name}: worst |U - U*_golden| = {worst:.3e} over {len(cases(name, 'qp'))} cases "
          f"({nfeas} feasible, {nel} elastic)")
    assert nfeas >= 3
    return worst


def library_qp(side):
    def solve(c, pset):
        r = side.run(c, pset, ubar=c["ubar"], elastic_rho=rho())
        return r["U"].ravel(), int(r["status"])
    return solve


def oracle_qp(oracles):
    from test_oracle_golden import params

    def solve(c, pset):
        r = oracles[int(c["traj"])].solve(params(c["N"], c["obs"].shape[0], pset, elastic_rho=rho()), c["x0"], c["obs"],
                                         ubar=c["ubar"])
        return r["U"], int(r["status"])
    return solve


# ---------------------------------------------------------------------------------------------
# the warm start's own knobs (the reference hard-codes 40 m and -2.0: checked against the oracle alone)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def knob_cases():
    """Records (traj, N, x0, obs) with one or two obstacles drawn either side of brake_distance = 25: at the
    threshold to within 1e-9 at the first stage, crossing it at stage 3 of the set's own dt stepping, well inside
    25 m, between 25 m and the default 40 m (brakes only under the default knob), and beyond 40 m plus the horizon's
    travel (never brakes)."""
    import workloads as W
    out = []
    for ti, N, seed in ((1, 10, 5), (2, 20, 6), (3, 40, 7)):
        wb = W.make_batch({1: "C2", 2: "C3", 3: "C5"}[ti], B=6, seed=seed)
        for b, x0 in enumerate(wb["x0"]):
            s, v = x0[0], x0[4]
            # the reach of the N-stage stepping at the largest dt of the sets: "far" never comes inside 40 m
            far = s + 40.0 + 0.3 * 41 * v + 5.0
            obs = [[(s + 25.0 - 1e-9, 1.0)], [(s + 25.0 + 1e-9, 1.0)], [(s + 25.0 + 2.5 * 0.2 * v, 0.0)],
                   [(s + 12.0, 3.0), (far, 2.0)], [(s + 33.0, 2.0)], [(far, 0.0)]][b]
            out.append(dict(traj=ti, N=N, x0=x0, obs=np.array(obs, np.float64).reshape(-1, 2)))
    return out


def check_knobs(side, oracles, name=None):
    """brake_distance = 25 and brake_accel = -3.5, under the defaults (name None) or a set: sqp_iters = 0 returns
    the oracle's warm start bit for bit; the cases brake at -3.5 on some stages and not on others, and those
    between 25 m and 40 m differ from the default knobs' warm start."""
    from test_oracle_golden import params
    pset = dict(sets()[name] if name else {}, **KNOBS)
    brake = free = moved = 0
    for j, c in enumerate(knob_cases()):
        orc = oracles[int(c["traj"])]
        want = orc.warm_start(params(c["N"], len(c["obs"]), pset), c["x0"], c["obs"])
        r = side.run(c, pset, sqp_iters=0)
        assert np.array_equal(r["U"].ravel(), want), (name, j, c["x0"], c["obs"])
        assert not (want[1::2] == -2.0).any()
        brake += int((want[1::2] == -3.5).sum())
        free += int((want[1::2] != -3.5).sum())
        default = orc.warm_start(params(c["N"], len(c["obs"]), sets()[name] if name else {}), c["x0"], c["obs"])
        moved += int(((default[1::2] == -2.0) != (want[1::2] == -3.5)).any())
    assert brake >= 50 and free >= 50 and moved >= 3, (brake, free, moved)


# ---------------------------------------------------------------------------------------------
# closed loop under set A
# ---------------------------------------------------------------------------------------------
LOOP_STEPS = 60


def closed_loop_A(TT, device):
    """(tracker, trajectory, FSM factory, x_init [3, 5]) of the set-A closed loop: the shim's TrajectoryTracker with
    set A's attributes (dt = 0.15 drives the Euler plant, the FSM's car and its light timer; the bounds clamp the
    actuation), N = 10 on trajectory 2 with the ObstaclesFSM.  Ego 0 stands 6 m before the red light, whose stop
    duration is cut to 3 s so that it turns GREEN after 20 steps of 0.15 s; ego 1 starts 3 m before the car's
    trigger, with the car spawned 35 m ahead; ego 2 drives towards the red light from 90 m."""
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    traj = TrajectoryLoader(builtin_trajectory(2))
    mpc = TT.TrajectoryTracker(traj, device=device)
    for k, v in sets()["A"].items():
        setattr(mpc, k, np.array(v, np.float64) if k in ("u_min", "u_max") else float(v))
    mpc.N = 10

    def mk():
        fsm = TT.ObstaclesFSM(dynamic_obstacle=True, traffic_light=True)
        fsm.tl_stop_duration = 3.0
        fsm.obs_start_s = fsm.obs_s = 745.0
        return fsm
    k = lambda s: traj.get_state(s)[3]
    x_init = np.array([[544.0, 0.0, 0.0, k(544.0), 0.05], [707.0, 0.02, 0.0, k(707.0), 8.0],
                       [460.0, -0.03, 0.0, k(460.0), 9.0]])
    return mpc, traj, mk, x_init


def assert_loop_switches(r, mpc):
    """Both state machines switch within the run, at set A's dt: ego 0's light turns GREEN at the step its timer
    reaches the stop duration, ego 1's car appears and then advances obs_v dt a step; the applied controls stay
    inside set A's bounds and touch neither default bound."""
    n = r["n_steps"]
    assert (n == LOOP_STEPS).all(), n
    tl = r["hist_tl"][0, :LOOP_STEPS]
    assert tl[0] == 0 and tl[-1] == 1
    first_green = int(np.argmax(tl == 1))
    timer, want = 0.0, 0                     # the timer adds dt a step from step 0 on (20 sums of 0.15 stay below 3.0)
    while timer + mpc.dt < 3.0:
        timer, want = timer + mpc.dt, want + 1
    assert first_green == want and 19 <= want <= 20, (first_green, want)
    car = r["hist_obs_s"][1, :LOOP_STEPS]
    assert np.isnan(car[0]) and np.isfinite(car[-1])
    seen = car[np.isfinite(car)]
    assert np.allclose(np.diff(seen), 4.0 * mpc.dt, rtol=0, atol=1e-9)
    u = r["hist_u"][:, :LOOP_STEPS]
    assert (u >= mpc.u_min - 1e-9).all() and (u <= mpc.u_max + 1e-9).all()


# ---------------------------------------------------------------------------------------------
# the 203-ego batches of test_gpu_horizons.sweep_batch under the sets
# ---------------------------------------------------------------------------------------------
BATCH_N = (15, 20, 25, 30, 40)


def assert_paths(name, wl, N, r):
    """The batch still runs the paths it is there for.  The oracle alone gives, over the five horizons and six sets:
    C2 65 (T, N = 40) to 163 (W, N = 15) crossover-certified, 40 (W, N = 15) to 138 (T, N = 40) deferred, 12 (B, W, T)
    to 90 (U, N = 40) elastic; C3 123 to 172 crossover-certified, 31 (B, N = 15) to 80 deferred, 9 (B, N = 15) to 22
    elastic."""
    xo, deferred = int((r["iters"] == 0).sum()), int((r["iters"] > 0).sum())
    elastic = int(((r["status"] & 15) == 2).sum())
    print(f"set {name} {wl} N={N}: crossover-certified {xo}, deferred {deferred}, elastic {elastic}")
    if wl in ("C2", "C3"):
        assert xo >= 20 and deferred >= 20, (name, wl, N, xo, deferred)
        assert elastic >= 5, (name, wl, N, elastic)
