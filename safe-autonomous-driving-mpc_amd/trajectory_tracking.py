"""Drop-in host surface of the reference tracking MPC, backed by the MI355X library.

Reference: medinammartin3/Safe-Autonomous-Driving-MPC trajectory_tracking.py
  TrajectoryTracker  (:8-263)   same attributes (dt, N, u_min, u_max, weights, safety params),
                                 same methods; solve(x0, obstacles) -> (u0, pred_X, solve_time)
                                 now runs one QP(ubar) instance on the GPU through libmpcqp
                                 (include/mpcqp.h); solve_batch() is the batched form.
  ObstaclesFSM       (:266-374)  same update(dt, s, v) -> (obstacles, 'RED'|'GREEN') contract;
                                 both presets of the reference (trajectory2 active, trajectory3
                                 commented out at :311-327) selectable by name.
  run_simulation     (:377-443)  same loop and returned histories, plus an optional step cap.

What differs by design: the reference's SLSQP on the nonlinear problem
(ftol 1e-3, maxiter 15, finite-difference gradients) is replaced by a Gauss-Newton SQP from the
same warm start: each QP is solved to 1e-9 by a primal-dual interior point on the GPU and re-linearised
about its solution until U moves by at most `sqp_tol` (at most `sqp_iters` QPs; it also stops on a 2-cycle
and after 5 elastic QPs in a row, include/mpcqp.h).  By default solve()
therefore returns the optimum of the reference's own nonlinear problem (pinned to it by
tests/golden/nlp_golden.npz), which its SLSQP only approximates; `sqp_iters = 1` gives the single
tracking QP at the warm start that bench.py times.  Nothing falls back silently: without libmpcqp.so, or
without a GPU for a device index, solve() raises; TrajectoryTracker(X_ref, device=-1) runs the library's host
backend (config 1's CPU path).
"""
import time

import numpy as np

import mpcqp
from sanity_checks import trajectory_tracking_check

# Gauss-Newton SQP cap of the drop-in default: sqp_tol stops it earlier, after 5-8 QPs on 50 of the 52
# certified nlp_golden cases; the slowest (a braking start far inside the obstacle margin) needs 28
SQP_ITERS = 30

# TrajectoryTracker attribute -> mpc_params field
_PARAM_ATTRS = ("dt", "N", "vehicle_radius", "w_d", "w_o", "w_v", "w_u1", "w_u2", "obstacle_safety_distance",
                "max_time_2_obs", "wheelbase", "lane_width", "safe_lane_margin")
_SOLVER_ATTRS = ("linearization", "sqp_iters", "max_iter", "polish", "tol", "tol_mu", "elastic_rho",
                 "brake_distance", "brake_accel", "sqp_tol")


class TrajectoryTracker:
    """Real-time tracking MPC (Frenet kinematic model, x = [s, d, o, k, v], u = [dk/dt, dv/dt])."""

    def __init__(self, X_ref=None, device=0):
        self.X_ref = X_ref
        self.device = device
        # model / horizon (:17-18)
        self.dt = 0.2
        self.N = 5
        # actuator limits (:31-33)
        self.u_min = np.array([-0.6, -5.0])
        self.u_max = np.array([0.6, 4.0])
        self.vehicle_radius = 1.0
        # objective weights (:36-40)
        self.w_d, self.w_o, self.w_v = 10.0, 10.0, 5.0
        self.w_u1, self.w_u2 = 0.5, 0.5
        # safety (:43-47)
        self.obstacle_safety_distance = 5.0
        self.max_time_2_obs = 1.5
        self.wheelbase = 2.8
        self.lane_width = 3.0
        self.safe_lane_margin = 0.1
        # GPU solver knobs.  The SQP defaults make solve() return the optimum of the reference's nonlinear
        # problem (nlp_golden); the other values are those of mpc_default_params
        self.linearization = 1
        self.sqp_iters = SQP_ITERS
        self.sqp_tol = 1e-10
        self.max_iter = 80
        self.polish = 2
        self.tol = 1e-9
        self.tol_mu = 1e-10
        self.elastic_rho = 1e5
        self.brake_distance = 40.0
        self.brake_accel = -2.0
        self.last_status = None
        self.last_iters = None
        self._solver = None
        self._solver_key = None

    # ---- model utilities (host-side numpy, same arithmetic as the reference) --------------
    def dynamics(self, x, u, k_ref):
        """x_dot = [v, v*o, v*(k - k_ref), u1, u2]  (:50-67)."""
        s, d, o, k, v = x
        return np.array([v, v * o, v * (k - k_ref), u[0], u[1]])

    def unpack(self, U_flat):
        return np.asarray(U_flat).reshape(self.N, 2)

    @staticmethod
    def pack(U):
        return np.asarray(U).ravel()

    def predict(self, x0, U_flat):
        """Explicit-Euler rollout over the horizon (:87-114)."""
        U = self.unpack(U_flat)
        X = np.zeros((self.N + 1, 5))
        X[0] = x0
        x = np.array(x0, dtype=np.float64)
        for j in range(self.N):
            x = x + self.dt * self.dynamics(x, U[j], self.X_ref.get_state(x[0])[3])
            X[j + 1] = x
        return X

    def cost(self, U_flat, x0):
        """Tracking + comfort objective (:116-152)."""
        U = self.unpack(U_flat)
        X = self.predict(x0, U_flat)
        c = 0.0
        for row in X[1:]:
            r = self.X_ref.get_state(row[0])
            c += self.w_d * (row[1] - r[1]) ** 2 + self.w_o * (row[2] - r[2]) ** 2 + self.w_v * (row[4] - r[4]) ** 2
        return c + float(np.sum(self.w_u1 * U[:, 0] ** 2 + self.w_u2 * U[:, 1] ** 2))

    def constraints(self, x0, obstacles):
        """{'type': 'ineq', 'fun': g(U) >= 0}, rows in the reference order (:155-211)."""
        sl = self.lane_width / 2.0 - self.vehicle_radius - self.safe_lane_margin

        def g(U_flat):
            X = self.predict(x0, U_flat)
            out = []
            for j in range(1, self.N + 1):
                s, d, o, _, v = X[j]
                for c in (0.0, self.wheelbase / 2.0, self.wheelbase):
                    e = d + c * o
                    out += [sl - e, e + sl]
                for ob in obstacles:
                    out.append(ob["s"] + ob["v"] * (j * self.dt) - s - max(self.obstacle_safety_distance,
                                                                             v * self.max_time_2_obs))
                out.append(v)
            return np.array(out)
        return {"type": "ineq", "fun": g}

    # ---- the GPU path ----------------------------------------------------------------------
    def params(self, max_obs=0):
        p = mpcqp.default_params()
        for a in _PARAM_ATTRS + _SOLVER_ATTRS:
            setattr(p, a, type(getattr(p, a))(getattr(self, a)))
        p.u_min[0], p.u_min[1] = float(self.u_min[0]), float(self.u_min[1])
        p.u_max[0], p.u_max[1] = float(self.u_max[0]), float(self.u_max[1])
        p.max_obs = int(max_obs)
        return p

    def solver(self, max_obs=0):
        """The libmpcqp context for X_ref (created on first use, parameters re-synced every call)."""
        if self.X_ref is None:
            raise ValueError("TrajectoryTracker needs X_ref (a TrajectoryLoader) to solve")
        key = id(self.X_ref)
        p = self.params(max_obs)
        if self._solver is None or self._solver_key != key:
            self._solver = mpcqp.Solver(self.X_ref.X_ref, self.X_ref.U_ref, p, device=self.device)
            self._solver_key = key
        else:
            self._solver.set_params(p)
        return self._solver

    def solve(self, x0, obstacles):
        """u0, pred_X, solve_time for one state (drop-in for :213-263).

        obstacles: list of {'s': position, 'v': speed, ...}; 'type' is ignored like the reference.
        solve_time covers the library call (host->device->host), as the reference timed minimize()."""
        obs = np.array([[float(o["s"]), float(o["v"])] for o in obstacles], dtype=np.float64).reshape(-1, 2)
        slv = self.solver(max_obs=len(obs))
        t0 = time.time()
        r = slv.solve_batch(np.asarray(x0, np.float64).reshape(1, 5),
                            obs.reshape(1, -1, 2) if len(obs) else None,
                            np.array([len(obs)], np.int32) if len(obs) else None)
        solve_time = time.time() - t0
        self.last_status = int(r["status"][0])
        self.last_iters = int(r["iters"][0])
        return r["U"][0][0].copy(), r["Xpred"][0].copy(), solve_time

    def solve_batch(self, x0, obstacles=None, ubar=None):
        """Batched solve: x0 [B,5]; obstacles: list (len B) of obstacle lists, or an array [B,M,2]."""
        x0 = np.asarray(x0, np.float64).reshape(-1, 5)
        B = x0.shape[0]
        obs = n = None
        if obstacles is not None:
            if isinstance(obstacles, np.ndarray):
                obs = obstacles.reshape(B, -1, 2)
                n = np.full(B, obs.shape[1], np.int32)
            else:
                mo = max((len(o) for o in obstacles), default=0)
                if mo:
                    obs = np.zeros((B, mo, 2))
                    n = np.zeros(B, np.int32)
                    for b, lst in enumerate(obstacles):
                        n[b] = len(lst)
                        for i, o in enumerate(lst):
                            obs[b, i] = (o["s"], o["v"])
        slv = self.solver(max_obs=0 if obs is None else obs.shape[1])
        return slv.solve_batch(x0, obs, n, ubar)

    def evaluate_batch(self, x0, U, obstacles=None):
        """cost(U, x0), the rows of constraints(x0, obstacles) and predict(x0, U) for a batch, on the library
        (mpc_evaluate_batch): x0 [B,5], U [B,N,2] any control sequences; obstacles as in solve_batch.  Returns
        mpcqp.Solver.evaluate_batch's dict with rows, plus 'n_obs' [B]; constraint_rows(r, b) is instance b's
        vector in the reference's order."""
        x0 = np.asarray(x0, np.float64).reshape(-1, 5)
        B = x0.shape[0]
        obs, n = _obstacle_slab(B, obstacles)
        slv = self.solver(max_obs=0 if obs is None else obs.shape[1])
        r = slv.evaluate_batch(x0, U, obs, n, rows=True)
        r["n_obs"] = np.zeros(B, np.int32) if n is None else n
        return r

    def certify_batch(self, x0, U, obstacles=None):
        """The first-order certificate of the control sequences U [B,N,2] at x0 [B,5], on the library
        (mpc_multipliers_batch, then mpc_gradient_batch with its multipliers); obstacles as in solve_batch.  Returns
        mpcqp.Solver.certify_batch's dict, plus 'n_obs' [B]."""
        x0 = np.asarray(x0, np.float64).reshape(-1, 5)
        B = x0.shape[0]
        obs, n = _obstacle_slab(B, obstacles)
        slv = self.solver(max_obs=0 if obs is None else obs.shape[1])
        r = slv.certify_batch(x0, U, obs, n)
        r["n_obs"] = np.zeros(B, np.int32) if n is None else n
        return r

    def hessian_batch(self, x0, U, lam=None, obstacles=None, mode="exact"):
        """The dense Hessian of cost - lam . g and the dense Jacobian of the rows at the control sequences U [B,N,2]
        from x0 [B,5], on the library (mpc_hessvec_batch with unit directions); obstacles as in solve_batch, lam as
        certify_batch returns it.  Returns mpcqp.Solver.hessian_batch's dict, plus 'n_obs' [B]."""
        x0 = np.asarray(x0, np.float64).reshape(-1, 5)
        B = x0.shape[0]
        obs, n = _obstacle_slab(B, obstacles)
        slv = self.solver(max_obs=0 if obs is None else obs.shape[1])
        r = slv.hessian_batch(x0, U, lam, obs, n, mode)
        r["n_obs"] = np.zeros(B, np.int32) if n is None else n
        return r


def _obstacle_slab(B, obstacles):
    """(obs [B,M,2], n_obs [B]) of solve_batch's obstacle forms: None, an array [B,M,2], or a list (len B) of
    obstacle lists; (None, None) when there is no obstacle at all."""
    if obstacles is None:
        return None, None
    if isinstance(obstacles, np.ndarray):
        obs = np.asarray(obstacles, np.float64).reshape(B, -1, 2)
        return (obs, np.full(B, obs.shape[1], np.int32)) if obs.shape[1] else (None, None)
    mo = max((len(o) for o in obstacles), default=0)
    if not mo:
        return None, None
    obs = np.zeros((B, mo, 2))
    n = np.zeros(B, np.int32)
    for b, lst in enumerate(obstacles):
        n[b] = len(lst)
        for i, o in enumerate(lst):
            obs[b, i] = (o["s"], o["v"])
    return obs, n


def constraint_rows(result_or_rows, b=0, n_obs=None):
    """The reference-order constraint vector of one instance (constraints(x0, obstacles)['fun'](U),
    trajectory_tracking.py:155-211: per stage the six lane rows, one row per obstacle, then v) from
    evaluate_batch's rows.  result_or_rows: the dict evaluate_batch returned (instance b, n_obs from its 'n_obs'
    unless given), or a rows array [B,N,7+M] / [N,7+M]; without n_obs the obstacle columns that are not NaN in
    the first stage are taken."""
    if isinstance(result_or_rows, dict):
        R = np.asarray(result_or_rows["rows"])[b]
        if n_obs is None and "n_obs" in result_or_rows:
            n_obs = int(np.asarray(result_or_rows["n_obs"])[b])
    else:
        R = np.asarray(result_or_rows, np.float64)
        R = R[b] if R.ndim == 3 else R
    if n_obs is None:
        n_obs = int(np.sum(~np.isnan(R[0, 7:])))
    return np.concatenate([R[:, :6], R[:, 7:7 + int(n_obs)], R[:, 6:7]], axis=1).ravel()


# ---------------------------------------------------------------------------------------------
# obstacle scenario state machine (trajectory_tracking.py:266-374)
# ---------------------------------------------------------------------------------------------
FSM_PRESETS = {
    # trajectory_tracking.py:292-308 (active in the reference)
    "trajectory2": dict(obs_trigger_s=710.0, obs_start_s=780.0, obs_v=4.0, obs_end_s=1050.0,
                        tl_pos=550.0, tl_trigger_s=100.0, tl_stop_duration=20.0),
    # trajectory_tracking.py:311-327 (commented out in the reference)
    "trajectory3": dict(obs_trigger_s=5.0, obs_start_s=150.0, obs_v=4.0, obs_end_s=850.0,
                        tl_pos=2000.0, tl_trigger_s=100.0, tl_stop_duration=20.0),
}


class ObstaclesFSM:
    """One dynamic car (WAITING -> ACTIVE -> COMPLETED) and one traffic light
    (RED_APPROACH -> RED_WAITING -> GREEN); update() returns the obstacles the MPC must respect."""

    def __init__(self, dynamic_obstacle=False, traffic_light=False, preset="trajectory2"):
        self.dynamic_obstacle = dynamic_obstacle
        self.traffic_light = traffic_light
        for k, v in FSM_PRESETS[preset].items():
            setattr(self, k, v)
        self.obs_active = False
        self.obs_has_triggered = False
        self.obs_s = self.obs_start_s
        self.tl_state = "RED"
        self.tl_timer = 0.0
        self.tl_waiting = False

    def update(self, dt, s, v):
        active = []
        if self.dynamic_obstacle:
            if s >= self.obs_trigger_s and not self.obs_has_triggered:
                self.obs_has_triggered = self.obs_active = True
            if self.obs_active:
                self.obs_s += self.obs_v * dt
                if self.obs_s > self.obs_end_s:
                    self.obs_active = False
                else:
                    active.append({"s": self.obs_s, "v": self.obs_v, "type": "car"})
        if self.traffic_light and self.tl_state == "RED":
            gap = self.tl_pos - s
            if 0 < gap < self.tl_trigger_s:
                active.append({"s": self.tl_pos, "v": 0.0, "type": "light"})
                if v < 0.1 and gap < 10.0:
                    self.tl_waiting = True
            if self.tl_waiting:
                self.tl_timer += dt
                if self.tl_timer >= self.tl_stop_duration:
                    self.tl_state = "GREEN"
                    self.tl_waiting = False
        return active, self.tl_state


def run_simulation(mpc, fsm, trajectory, max_steps=None, verbose=True):
    """Closed loop of trajectory_tracking.py:377-443 (same histories); max_steps caps the loop
    (the reference has no cap and spins forever if the ego stalls)."""
    x = np.array([0.0, 0.0, 0.0, 0.0, 0.5])
    hist_x, hist_u, hist_t, hist_preds, hist_obs_s, hist_tl_state = [x], [], [], [], [], []
    step = 0
    while x[0] <= trajectory.s_max - 1.0 and (max_steps is None or step < max_steps):
        obstacles, tl_state = fsm.update(mpc.dt, x[0], x[4])
        u, pred_X, cpu = mpc.solve(x, obstacles)
        k_ref = trajectory.get_state(x[0])[3]
        x = x + mpc.dt * mpc.dynamics(x, u, k_ref)       # plant == prediction model (:404-406)
        hist_x.append(x)
        hist_u.append(u)
        hist_t.append(cpu)
        hist_preds.append(pred_X)
        hist_tl_state.append(tl_state)
        car = [o["s"] for o in obstacles if o["type"] == "car"]
        hist_obs_s.append(car[0] if car else np.nan)
        if verbose and step % 50 == 0:
            print(progress_line(step, x, tl_state, hist_obs_s[-1], fsm, mpc.obstacle_safety_distance))
        step += 1
    trajectory_tracking_check(mpc, hist_x, hist_u, hist_t, hist_obs_s, hist_tl_state, fsm, trajectory.s_max)
    return (np.array(hist_x), np.array(hist_u), np.array(hist_t), hist_preds, hist_obs_s, hist_tl_state,
            trajectory)


def progress_line(step, x, tl_state, obstacle_s, fsm, safety_distance=5.0):
    """The reference's progress print of run_simulation (trajectory_tracking.py:423-435), verbatim format."""
    vehicle_info = f"s={x[0]:.1f}m, v={x[4] * 3.6:.1f}km/h"
    if fsm.traffic_light:
        dist_2_tl = fsm.tl_pos - x[0]
        tl_info = (f"color={tl_state}, distance={dist_2_tl:.1f}m" if dist_2_tl > safety_distance
                   else f"color={tl_state}, distance=NaN")
    else:
        tl_info = "NaN"
    obs_info = f"{obstacle_s - x[0]:.1f}m" if not np.isnan(obstacle_s) else "NaN"
    return f"Step {step} | {vehicle_info} | Traffic Light : {tl_info} | Distance to obstacle : {obs_info}"


def fsm_params(fsm):
    """mpc_fsm (include/mpcqp.h) of an ObstaclesFSM, or None when it has no scenario switched on."""
    if fsm is None or not (fsm.dynamic_obstacle or fsm.traffic_light):
        return None
    return mpcqp.default_fsm(dynamic_obstacle=int(bool(fsm.dynamic_obstacle)), traffic_light=int(bool(fsm.traffic_light)),
                             **{k: float(getattr(fsm, k)) for k in FSM_PRESETS["trajectory2"]})


def run_simulation_batch(mpc, fsm, trajectory, x_init=None, B=1, max_steps=2000, checks=False, verbose=False):
    """run_simulation (trajectory_tracking.py:377-443) for B independent egos, entirely on the device
    (mpc_closed_loop): each ego owns a fresh copy of `fsm`'s scenario, the loop runs while
    s <= s_max - 1.  x_init [B,5] defaults to the reference start [0,0,0,0,0.5] (:382).
    Returns the device histories (see mpcqp.Solver.closed_loop); with checks=True also runs the
    restated trajectory_tracking_check on every ego and adds 'checks_passed' [B]."""
    if x_init is None:
        x_init = np.tile(np.array([0.0, 0.0, 0.0, 0.0, 0.5]), (B, 1))
    x_init = np.asarray(x_init, np.float64).reshape(-1, 5)
    r = mpc.solver(max_obs=0).closed_loop(x_init, fsm_params(fsm), max_steps=max_steps, s_max=trajectory.s_max)
    if checks:
        r["checks_passed"] = closed_loop_checks(mpc, fsm, trajectory, r, verbose)
    return r


def scenario_grid(base_fsm, **axes):
    """The Cartesian product of ObstaclesFSM field values as a list of scenarios: copies of `base_fsm` with
    the named fields replaced, e.g. scenario_grid(fsm, obs_v=[2, 4, 6], tl_stop_duration=[5, 20]) -> 6 scenarios.
    Order: itertools.product over the axes in keyword order, so the last axis varies fastest
    ((2, 5), (2, 20), (4, 5), ...)."""
    import copy
    import itertools
    for k in axes:
        if not hasattr(base_fsm, k):
            raise ValueError(f"ObstaclesFSM has no field {k!r}")
    out = []
    for values in itertools.product(*axes.values()):
        f = copy.copy(base_fsm)
        for k, v in zip(axes, values):
            setattr(f, k, v)
        out.append(f)
    return out


def _fsm_record(fsm):
    """mpc_fsm of one ego of a sweep: the ObstaclesFSM's fields (fsm_params), both switches off for None."""
    if fsm is None:
        return mpcqp.default_fsm()
    return mpcqp.default_fsm(dynamic_obstacle=int(bool(fsm.dynamic_obstacle)), traffic_light=int(bool(fsm.traffic_light)),
                             **{k: float(getattr(fsm, k)) for k in FSM_PRESETS["trajectory2"]})


def run_scenario_sweep(mpc, scenarios, trajectory, x_init, max_steps=2000, hist_egos=(), s_stop=None):
    """One closed loop per (ego, scenario) pair in a single library call (mpc_closed_loop_sweep): ego b starts
    at x_init[b] and runs scenarios[b], an ObstaclesFSM or None (no scenario), while s <= s_stop (default
    s_max - 1).  The check quantities are accumulated while the loop runs; full histories come back only for
    the egos in `hist_egos`.  Returns mpcqp.Solver.closed_loop_sweep's dict plus 'verdicts' [B] (bitmask,
    mpcqp.CLV_NAMES), 'counts' {name: egos passing} and one boolean column [B] per verdict name
    (sanity_checks.check_verdicts with s_total = s_max)."""
    x_init = np.asarray(x_init, np.float64).reshape(-1, 5)
    scenarios = list(scenarios)
    if len(scenarios) != x_init.shape[0]:
        raise ValueError("one scenario (or None) per ego")
    recs = None if all(f is None for f in scenarios) else [_fsm_record(f) for f in scenarios]
    slv = mpc.solver(max_obs=0)
    r = slv.closed_loop_sweep(x_init, recs, max_steps, s_stop=s_stop, s_max=trajectory.s_max, hist_egos=hist_egos)
    v, counts = slv.cl_verdicts(r["quant"], trajectory.s_max)
    r["verdicts"] = v
    r["counts"] = {k: int(counts[i]) for i, k in enumerate(mpcqp.CLV_NAMES)}
    for i, k in enumerate(mpcqp.CLV_NAMES):
        r[k] = (v & (1 << i)) != 0
    return r


class TrafficScript:
    """A traffic script for one ego: a list of actors (mpcqp.car(...), mpcqp.light(...), or mpcqp.MpcActor() as a
    placeholder), each running ObstaclesFSM's per-obstacle state machine on its own state.  update() is the host
    restatement of one step of mpc_closed_loop_traffic for this ego, in the reference's update() shape, so the
    one-ego loop (run_simulation's) can drive it; run_traffic_sweep runs many of them on the device."""

    def __init__(self, actors=()):
        self.actors = list(actors)
        if len(self.actors) > mpcqp.MAX_ACTORS:
            raise ValueError(f"at most {mpcqp.MAX_ACTORS} actors per script")
        for a in self.actors:
            if a.kind not in (mpcqp.ACTOR_NONE, mpcqp.ACTOR_CAR, mpcqp.ACTOR_LIGHT):
                raise ValueError(f"actor kind {a.kind} outside ACTOR_NONE .. ACTOR_LIGHT")
        # per actor: car [position, active, triggered]; light [timer, green, waiting]
        self.state = [[a.pos_s if a.kind == mpcqp.ACTOR_CAR else 0.0, False, False] for a in self.actors]

    @classmethod
    def from_fsm(cls, fsm):
        """[car, light] restating an ObstaclesFSM (a placeholder for a switch that is off; mpc_actors_from_fsm)."""
        return cls(mpcqp.actors_from_fsm(_fsm_record(fsm)))

    def padded(self, A):
        """The actors padded with placeholders to A entries (every script of one call has the same length)."""
        if len(self.actors) > A:
            raise ValueError("script longer than the requested width")
        return self.actors + [mpcqp.MpcActor() for _ in range(A - len(self.actors))]

    def update(self, dt, s, v):
        """One step on the ego state before the step.  Returns (active_obstacles, states): the obstacles in
        actor order as ObstaclesFSM.update's dicts, and one state per actor ('WAITING' / 'ACTIVE' / 'COMPLETED'
        for a car, 'RED' / 'GREEN' for a light, None for a placeholder)."""
        active, states = [], []
        for a, st in zip(self.actors, self.state):
            if a.kind == mpcqp.ACTOR_CAR:
                if s >= a.trigger_s and not st[2]:
                    st[2] = st[1] = True
                if st[1]:
                    st[0] += a.v * dt
                    if st[0] > a.end_s:
                        st[1] = False
                    else:
                        active.append({"s": st[0], "v": a.v, "type": "car"})
                states.append("ACTIVE" if st[1] else ("COMPLETED" if st[2] else "WAITING"))
            elif a.kind == mpcqp.ACTOR_LIGHT:
                if not st[1]:
                    gap = a.pos_s - s
                    if 0 < gap < a.trigger_s:
                        active.append({"s": a.pos_s, "v": 0.0, "type": "light"})
                        if v < 0.1 and gap < 10.0:
                            st[2] = True
                    if st[2]:
                        st[0] += dt
                        if st[0] >= a.stop_duration:
                            st[1], st[2] = True, False
                states.append("GREEN" if st[1] else "RED")
            else:
                states.append(None)
        return active, states


def run_traffic_sweep(mpc, scripts, trajectory, x_init, max_steps=2000, hist_egos=(), s_stop=None):
    """run_scenario_sweep with a traffic script per ego (mpc_closed_loop_traffic): ego b starts at x_init[b] and
    runs scripts[b], a TrafficScript, a sequence of actors, or None (no actor); shorter scripts are padded with
    placeholders to the longest.  Returns mpcqp.Solver.closed_loop_traffic's dict plus 'verdicts' [B], 'counts'
    and one boolean column [B] per verdict name, like run_scenario_sweep."""
    x_init = np.asarray(x_init, np.float64).reshape(-1, 5)
    scripts = [s if isinstance(s, TrafficScript) else TrafficScript(s or ()) for s in scripts]
    if len(scripts) != x_init.shape[0]:
        raise ValueError("one script (or None) per ego")
    A = max((len(s.actors) for s in scripts), default=0)
    rows = [s.padded(A) for s in scripts] if A else None
    slv = mpc.solver(max_obs=0)
    r = slv.closed_loop_traffic(x_init, rows, max_steps, s_stop=s_stop, s_max=trajectory.s_max, hist_egos=hist_egos)
    v, counts = slv.cl_verdicts(r["quant"], trajectory.s_max)
    r["verdicts"] = v
    r["counts"] = {k: int(counts[i]) for i, k in enumerate(mpcqp.CLV_NAMES)}
    for i, k in enumerate(mpcqp.CLV_NAMES):
        r[k] = (v & (1 << i)) != 0
    return r


def convoy_starts(traj, n_worlds, W, headway_m, v, s0=0.0):
    """Start states [n_worlds * W, 5] of n_worlds identical convoys on the reference line of `traj` (a
    TrajectoryLoader): in every world ego 0 starts at s0 and ego i `headway_m` metres ahead of ego i - 1 (the
    last ego leads), on the line (d = o = 0) at speed v, with k taken from the table."""
    s = s0 + headway_m * np.arange(W)
    world = np.array([[si, 0.0, 0.0, traj.get_state(si)[3], v] for si in s])
    return np.tile(world, (n_worlds, 1))


def run_convoy_sweep(mpc, trajectory, x_init, W, K, lead_range=np.inf, scripts=None, max_steps=2000, hist_egos=(),
                     s_stop=None):
    """run_traffic_sweep with the egos [w*W, (w+1)*W) of a world seeing each other (mpc_closed_loop_convoy): per
    step an ego's obstacles are its script's, then its up to K nearest leaders within lead_range.  scripts: None,
    or one TrafficScript / sequence of actors / None per ego.  Returns mpcqp.Solver.closed_loop_convoy's dict plus
    'verdicts' [B], 'counts' and one boolean column [B] per verdict name, like run_scenario_sweep."""
    x_init = np.asarray(x_init, np.float64).reshape(-1, 5)
    rows = None
    if scripts is not None:
        scripts = [s if isinstance(s, TrafficScript) else TrafficScript(s or ()) for s in scripts]
        if len(scripts) != x_init.shape[0]:
            raise ValueError("one script (or None) per ego")
        A = max((len(s.actors) for s in scripts), default=0)
        rows = [s.padded(A) for s in scripts] if A else None
    slv = mpc.solver(max_obs=0)
    r = slv.closed_loop_convoy(x_init, W, K, lead_range=lead_range, scripts=rows, max_steps=max_steps, s_stop=s_stop,
                               s_max=trajectory.s_max, hist_egos=hist_egos)
    v, counts = slv.cl_verdicts(r["quant"], trajectory.s_max)
    r["verdicts"] = v
    r["counts"] = {k: int(counts[i]) for i, k in enumerate(mpcqp.CLV_NAMES)}
    for i, k in enumerate(mpcqp.CLV_NAMES):
        r[k] = (v & (1 << i)) != 0
    return r


_NZ_M0, _NZ_M1, _NZ_W0, _NZ_W1 = (np.uint64(c) for c in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85))
_NZ_MASK, _NZ_32 = np.uint64(0xFFFFFFFF), np.uint64(32)
NOISE_C = 1.7320508075688772 * 2.0 ** -32          # the double nearest sqrt(3), scaled exactly


def philox4x32(counter, key):
    """Philox4x32-10 in numpy uint64 arithmetic: counter (c0, c1, c2, c3) and key (k0, k1) of 32-bit words
    (arrays broadcast) -> the four output words [..., 4] (uint32)."""
    c = [np.asarray(x, np.uint64) & _NZ_MASK for x in counter]
    k = [np.asarray(x, np.uint64) & _NZ_MASK for x in key]
    for _ in range(10):
        p0, p1 = _NZ_M0 * c[0], _NZ_M1 * c[2]       # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> _NZ_32) ^ c[1] ^ k[0], p1 & _NZ_MASK, (p0 >> _NZ_32) ^ c[3] ^ k[1], p0 & _NZ_MASK]
        k = [(k[0] + _NZ_W0) & _NZ_MASK, (k[1] + _NZ_W1) & _NZ_MASK]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def noise_variates(seed, ego, step, channel):
    """The draws of mpc_closed_loop_noisy restated (include/mpcqp.h; what Solver.noise_draw returns, bit for bit):
    key (seed & 0xffffffff, seed >> 32), counter (ego & 0xffffffff, ego >> 32, step, channel), one Philox4x32-10
    block per draw, z = (w0 + w1 + w2 + w3 - 8589934590) * sqrt(3) * 2^-32.  ego, step, channel broadcast.
    Returns (words [..., 4] uint32, z [...])."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g = np.asarray(ego).astype(np.uint64)                    # int64 or uint64 (egos past 2^63 in the known answers)
    step = np.asarray(step, np.int64).astype(np.uint64) & _NZ_MASK
    ch = np.asarray(channel, np.int64).astype(np.uint64) & _NZ_MASK
    w = philox4x32((g & _NZ_MASK, g >> _NZ_32, step, ch), (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)))
    total = w.astype(np.uint64).sum(axis=-1)                 # < 2^34: exact as a double
    return w, (total.astype(np.float64) - 8589934590.0) * NOISE_C


def run_noisy_sweep(mpc, trajectory, x_init, noise, seeds, W=1, K=0, lead_range=np.inf, scripts=None,
                    max_steps=2000, hist_egos=(), s_stop=None, seed=0):
    """A Monte Carlo disturbance sweep (mpc_closed_loop_noisy): the scenario x_init [W,5] (one ego, or one world of
    W egos with run_convoy_sweep's scripts, one per ego of the world) replicated once per entry of `seeds` and run
    under `noise` (an mpcqp.MpcNoise shared by all).  A seed is a stream index under the key `seed`: replica s runs
    as the global egos s*W .. s*W + W - 1, so its rows equal Solver.closed_loop_noisy(x_init, ..., seed=seed,
    lo=s*W) whatever else shares the batch; runs of consecutive seeds go into one library call each.  hist_egos
    index the replicated batch (replica r, ego i of the world: r*W + i).  Returns closed_loop_noisy's dict over
    all replicas in `seeds` order plus 'seeds' [n], 'verdicts' [n*W], 'counts', one boolean column per verdict
    name and 'pass_rate' {name: fraction of the n*W egos passing}."""
    x_world = np.asarray(x_init, np.float64).reshape(-1, 5)
    W = int(W)
    if x_world.shape[0] != W:
        raise ValueError("x_init holds one world: W start states")
    seeds = [int(s) for s in seeds]
    if not seeds or min(seeds) < 0:
        raise ValueError("seeds: a non-empty sequence of integers >= 0")
    rows = None
    if scripts is not None:
        scripts = [s if isinstance(s, TrafficScript) else TrafficScript(s or ()) for s in scripts]
        if len(scripts) != W:
            raise ValueError("one script (or None) per ego of the world")
        A = max((len(s.actors) for s in scripts), default=0)
        rows = [s.padded(A) for s in scripts] if A else None
    slv = mpc.solver(max_obs=0)
    hist_egos = np.asarray(hist_egos, np.int64).ravel()
    parts, r0 = [], 0
    while r0 < len(seeds):                                   # runs of consecutive seeds: one call each
        r1 = r0 + 1
        while r1 < len(seeds) and seeds[r1] == seeds[r1 - 1] + 1:
            r1 += 1
        n = r1 - r0
        he = hist_egos[(hist_egos >= r0 * W) & (hist_egos < r1 * W)] - r0 * W
        parts.append(slv.closed_loop_noisy(np.tile(x_world, (n, 1)), W, K, lead_range=lead_range,
                                           scripts=None if rows is None else rows * n, max_steps=max_steps,
                                           s_stop=s_stop, s_max=trajectory.s_max, hist_egos=he, noise=noise,
                                           seed=seed, lo=seeds[r0] * W))
        p = parts[-1]
        p["hist_egos"] = p["hist_egos"] + r0 * W
        p["hist_lead"] = p["hist_lead"] + np.where(p["hist_lead"] >= 0, r0 * W, 0).astype(np.int32)
        r0 = r1
    r = {k: (np.fmax.reduce([p[k] for p in parts]) if k == "step_ms" else np.concatenate([p[k] for p in parts]))
         for k in parts[0]}
    r["seeds"] = np.asarray(seeds, np.int64)
    v, counts = slv.cl_verdicts(r["quant"], trajectory.s_max)
    r["verdicts"] = v
    r["counts"] = {k: int(counts[i]) for i, k in enumerate(mpcqp.CLV_NAMES)}
    r["pass_rate"] = {k: float(counts[i]) / v.size for i, k in enumerate(mpcqp.CLV_NAMES)}
    for i, k in enumerate(mpcqp.CLV_NAMES):
        r[k] = (v & (1 << i)) != 0
    return r


def run_simulation_traced(mpc, fsms, trajectory, hist_egos=None, max_steps=2000, x_init=None):
    """run_simulation (trajectory_tracking.py:377-443) for a list of ObstaclesFSM scenarios (None: no scenario) in
    one library call that keeps every step's prediction (mpc_closed_loop_traced): ego b runs fsms[b] restated as a
    two-actor script, from x_init[b] (default: the reference start [0,0,0,0,0.5], :382) while s <= s_max - 1.
    Returns, for each ego of hist_egos (default: every ego), the reference's tuple
        hist_x [n+1,5], hist_u [n,2], hist_t [n], hist_preds, hist_obs_s, hist_tl_state, trajectory
    cut at the ego's n steps: hist_preds a list of n (N+1, 5) arrays, hist_obs_s a list of car positions (NaN: no
    car), hist_tl_state a list of 'RED' / 'GREEN', hist_t the step times of the whole batch in seconds.  The tuple
    feeds driving_animation and plot_tracking_results as run_simulation's does.  Prints nothing and runs no
    sanity check."""
    return _run_simulation_batched(mpc, fsms, trajectory, hist_egos, max_steps, x_init, None)


def run_simulation_carried(mpc, fsms, trajectory, hist_egos=None, max_steps=2000, x_init=None, tail=None, reset=0):
    """run_simulation_traced with the carried loop (mpc_closed_loop_warm, WARM_CARRY): every step's QP is linearised
    about the ego's previous plan shifted by one stage instead of the reference warm start.  tail: mpcqp.WTAIL_*
    (default WTAIL_REFERENCE); reset: an OR of mpcqp.WRESET_* bits.  The same return values per named ego."""
    warm = mpcqp.default_warm(mode=mpcqp.WARM_CARRY, tail=mpcqp.WTAIL_REFERENCE if tail is None else tail, reset=reset)
    return _run_simulation_batched(mpc, fsms, trajectory, hist_egos, max_steps, x_init, warm)


def _run_simulation_batched(mpc, fsms, trajectory, hist_egos, max_steps, x_init, warm):
    """run_simulation_traced (warm None) or run_simulation_carried (warm: the MpcWarm of the loop)."""
    fsms = list(fsms)
    B = len(fsms)
    if x_init is None:
        x_init = np.tile(np.array([0.0, 0.0, 0.0, 0.0, 0.5]), (B, 1))
    x_init = np.asarray(x_init, np.float64).reshape(-1, 5)
    if x_init.shape[0] != B:
        raise ValueError("one start state per scenario")
    hist_egos = list(range(B)) if hist_egos is None else [int(e) for e in hist_egos]
    scripts = [TrafficScript.from_fsm(f).actors for f in fsms]
    kw = dict(scripts=scripts, max_steps=max_steps, s_max=trajectory.s_max, hist_egos=hist_egos, preds=True)
    slv = mpc.solver(max_obs=0)
    r = slv.closed_loop_traced(x_init, **kw) if warm is None else slv.closed_loop_warm(x_init, warm=warm, **kw)
    out = []
    for k, b in enumerate(hist_egos):
        n = int(r["n_steps"][b])
        green = (r["hist_tl"][k, :n] & 2) != 0            # actor 1 of the script is the light
        out.append((r["hist_x"][k, :n + 1].copy(), r["hist_u"][k, :n].copy(), r["step_ms"][:n] / 1000.0,
                    [r["hist_pred"][k, t].copy() for t in range(n)], [float(v) for v in r["hist_car_s"][k, :n]],
                    ["GREEN" if g else "RED" for g in green], trajectory))
    return out


def closed_loop_checks(mpc, fsm, trajectory, r, verbose=False):
    """The restated trajectory_tracking_check (sanity_checks.py:79-184) on every ego of a closed_loop()
    result (mpcqp.Solver.closed_loop layout); returns the per-ego verdicts [B] (bool)."""
    import contextlib
    import io
    B = np.asarray(r["n_steps"]).size
    ok = np.zeros(B, bool)
    for b in range(B):
        n = int(r["n_steps"][b])
        # the solve time this ego waited for at each of its steps: that batched step's device time
        # (the reference tests max(hist_t) per step, sanity_checks.py:134-135; shard.closed_loop_quantities)
        step_s = np.asarray(r["step_ms"][:n], np.float64) / 1e3
        f = ObstaclesFSM(fsm.dynamic_obstacle, fsm.traffic_light) if fsm is not None else ObstaclesFSM()
        if fsm is not None:
            for k in FSM_PRESETS["trajectory2"]:
                setattr(f, k, getattr(fsm, k))
        buf = io.StringIO()
        tl = ["GREEN" if t == 1 else "RED" for t in r["hist_tl"][b, :n]]
        with contextlib.redirect_stdout(buf):
            ok[b] = bool(trajectory_tracking_check(mpc, list(r["hist_x"][b, :n + 1]), list(r["hist_u"][b, :n]),
                                                   list(step_s), list(r["hist_obs_s"][b, :n]), tl, f,
                                                   trajectory.s_max))
        if verbose:
            print(buf.getvalue())
    return ok


if __name__ == "__main__":
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    traj = TrajectoryLoader(builtin_trajectory(2))
    run_simulation(TrajectoryTracker(traj), ObstaclesFSM(dynamic_obstacle=True, traffic_light=True), traj)
