"""Shared pieces of the planner's non-default-parameter tests (test_plan_params_cpu.py on the oracle, the host
backend and the emulated kernel; test_gpu_plan_params.py on the device): the named parameter sets, the plan_params
of each side built from a set, the batches, and the evaluator cases regenerated under a set.

A parameter set is a dict of the plan_params model fields that differ from plan_default_params (the 13 fields dt,
w_y, w_s, w_u, w_slack, u_min[2], u_max[2], k_min, k_max, a_max, v_min, defect_sign).  A and B move the weights,
the bounds and dt in opposite directions; W, U, G, T, V and S move one group each (weights, control bounds, curvature
and lateral-acceleration bounds, dt, v_min, defect_sign), so a failure under one of them names its group.

v_min > 0 (B, V): the reference's last state has no slack (trajectory_planning.py:253-256), so a final chunk, whose
v_N = 0 (:231-236), is infeasible there and the library leaves that row out.  Such sets are solved on intermediate
chunks only (batch() clears the final flags); the evaluator sees them on both kinds.
defect_sign = -1 (S) is the committed source's literal sign (:205): time runs backwards, progress needs v < 0 and
the speed rows are then met by the slack alone.  It converges less often than the forward rule, so it stays out of A
and B (which would fall below the condition the GPU comparisons need) and has the set S of its own.
GK is the launch-order test's set: k_min = -k_max = 0.01, so the order score |kappa| / max(|k_min|, |k_max|) of the
synth1 chunks (|kappa| up to 0.13) spreads over every bucket of the longest-first order, where under the default
bounds all of them share the last one."""
import functools

import numpy as np

SETS = {
    "A": dict(dt=0.24, w_y=6.0, w_s=14.0, w_u=0.25, w_slack=60.0, u_min=(-0.45, -4.0), u_max=(0.5, 3.0), k_min=-0.6,
              k_max=0.7, a_max=4.5),
    "B": dict(dt=0.36, w_y=15.0, w_s=5.0, w_u=0.05, w_slack=150.0, u_min=(-0.7, -6.0), u_max=(0.65, 5.0), k_min=-0.9,
              k_max=0.85, a_max=7.5, v_min=0.5),
    "W": dict(w_y=6.0, w_s=14.0, w_u=0.25, w_slack=60.0),
    "U": dict(u_min=(-0.45, -4.0), u_max=(0.5, 3.0)),
    "G": dict(k_min=-0.6, k_max=0.7, a_max=4.5),
    "T": dict(dt=0.24),
    "V": dict(v_min=0.5),
    "S": dict(defect_sign=-1.0),
}
GROUP_SETS = ("W", "U", "G", "T", "V", "S")
GK = dict(k_min=-0.01, k_max=0.01)
MODEL_FIELDS = ("dt", "w_y", "w_s", "w_u", "w_slack", "u_min", "u_max", "k_min", "k_max", "a_max", "v_min", "defect_sign")


def pset(name):
    return GK if name == "GK" else SETS[name]


def intermediate_only(ps):
    return ps.get("v_min", 0.0) > 0.0


def lib_params(mod, ps, **kw):
    """plan_params of mpcplan or plan_oracle (mod.default_params) under the set, plus solver fields kw (N, ...)."""
    return mod.default_params(**ps, **kw)


def ref_params(ps):
    """(plan_ref.Params, dt) under the set."""
    import plan_ref as PR
    return PR.Params(**{k: v for k, v in ps.items() if k != "dt"}), ps.get("dt", 0.3)


def fields(p):
    """The 13 model fields of a plan_params structure as a flat tuple."""
    out = []
    for f in MODEL_FIELDS:
        v = getattr(p, f)
        out += [v[0], v[1]] if f in ("u_min", "u_max") else [v]
    return tuple(out)


# ---------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------
# the GPU comparison's shapes: (N, route) -- a single lane group, N = 20, and just past a 32-stage boundary
GPU_SHAPES = ((5, "synth1"), (20, "traj2"), (33, "synth2"))
GPU_CASES = tuple((s, N, rt) for s in ("A", "B") for N, rt in GPU_SHAPES) + \
    tuple((s, 20, "traj2") for s in GROUP_SETS)


def batch(W, route, N, ps, B=64, final_frac=0.25):
    """workloads.plan_batch(route, N, B, seed = N, final_frac) -- all intermediate under a set with v_min > 0."""
    wb = W.plan_batch(route, N, B, seed=N, final_frac=final_frac)
    if intermediate_only(ps):
        wb = W.plan_batch(route, N, B, seed=N, final_frac=0.0)
    return wb


def mixed_batch(W, r, ps, n=48, seed=11):
    """test_plan_host._batch: intermediate and final chunks of the horizons 13, 16, 20, 26 along the route (the
    final ones intermediate under a set with v_min > 0)."""
    rng = np.random.default_rng(seed)
    x0 = np.zeros((n, 5))
    s0 = rng.uniform(0.0, r.s_total - 45.0, n)
    x0[:, 0] = s0
    x0[:, 1] = rng.uniform(-0.05, 0.05, n)
    x0[:, 3] = [r.k_ref_fun(s) for s in s0]
    x0[:, 4] = [rng.uniform(0.3, 0.9) * r.v_max_fun(s) for s in s0]
    fin = (np.arange(n) % 4 == 3).astype(np.int32)
    st = np.where(fin == 1, np.minimum(s0 + 35.0, r.s_total), s0 + 20.0)
    if intermediate_only(ps):
        fin[:] = 0
    N = np.array([(13, 16, 20, 26)[i % 4] for i in range(n)], np.int32)
    return x0, st, fin, N


def order_batch(W, r):
    """160 chunks of mixed N in {8, 16, 24} (at or above the 128 at which the longest-first order is used)."""
    parts = [W.plan_batch(r, n, 160, seed=50 + n, final_frac=0.2) for n in (8, 16, 24)]
    N = np.array([(8, 16, 24)[i % 3] for i in range(160)], np.int32)
    pick = lambda key: np.array([parts[i % 3][key][i] for i in range(160)])
    return pick("x0"), pick("s_target"), pick("is_final").astype(np.int32), N


def loop_starts(r):
    """three starts on a route: the reference's and two along it"""
    starts = np.zeros((3, 5))
    for b, s0 in ((1, 400.0), (2, 1100.0)):
        starts[b] = (s0, 0.02, 0.0, r.k_ref_fun(s0), 0.6 * r.v_max_fun(s0))
    return starts


def loop_optimizer(TP, ps, device):
    """A TrajectoryOptimizer with the set's attributes (the sets it is used with keep v_min and defect_sign)."""
    opt = TP.TrajectoryOptimizer(device=device)
    for k, v in ps.items():
        setattr(opt, k, np.array(v, float) if k in ("u_min", "u_max") else v)
    return opt


OUTPUTS = ("X", "U", "S", "status", "iters", "sqp")
ACTIVE = 1e-6       # a row counts as active at a solution when its margin is at most this (they sit at ~1e-12)


def active_rows(o, p):
    """Per chunk of a solve_batch result under the plan_params p: (a lateral-acceleration row is active, a curvature
    bound is active) at some stage k >= 1 (stage 0 is x0 and has neither row), judged by the margins a_max - |k| v^2,
    k - k_min and k_max - k."""
    k, v = o["X"][:, 1:, 3], o["X"][:, 1:, 4]
    lat = (p.a_max - np.abs(k) * v * v).min(axis=1) <= ACTIVE
    cur = np.minimum(k - p.k_min, p.k_max - k).min(axis=1) <= ACTIVE
    return lat, cur


def counts(status):
    return np.bincount(status, minlength=5).tolist()


# ---------------------------------------------------------------------------------------------
# the evaluator's cases under a set (plan_evaluate_cases' generator with dt and the set)
# ---------------------------------------------------------------------------------------------
EV_HORIZONS = (1, 2, 63, 64, 65)
EV_ROUTE = "traj2"
EV_SEED = 2025
EV_SETS = ("A", "B", "W", "U", "G", "T", "V", "S")

# The largest absolute error of the host backend against plan_ref over the 10 cases of each set, measured on the
# CPU (test_plan_params_cpu.py prints every figure and asserts 8 x these; sums relative to 1 + |ref|).  traj2 is the
# route on which plan_ref itself is least exact (plan_evaluate_cases: 1.8e-15 against synth1's 8.3e-17 in the defects).
MEASURED_DEFECTS = 4.4408920985006262e-16      # set A (G 2.2e-16, V 1.1e-16, the others <= 6.2e-17)
MEASURED_ROWS = 0.0                            # every set: the rows are single subtractions in plan_ref's order
MEASURED_SUMS = 8.5855184349053702e-16         # set B (A 7.8e-16, T 7.4e-16, G 7.3e-16, S 6.5e-16, U 6.4e-16, W 5.9e-16, V 4.6e-16)
MARGIN = 8.0
TOL_DEFECTS = MARGIN * MEASURED_DEFECTS
TOL_ROWS = MARGIN * MEASURED_ROWS
TOL_SUMS = MARGIN * MEASURED_SUMS


@functools.lru_cache(maxsize=None)
def ev_cases(name):
    """The 10 evaluator cases of a set (read-only): horizon-major, intermediate then final."""
    import plan_evaluate_cases as PC
    import workloads as W
    params, dt = ref_params(pset(name))
    route = W.plan_route(EV_ROUTE)
    rng = np.random.default_rng([EV_SEED, EV_SETS.index(name)])
    return tuple(PC._make(route, N, fin, rng, dt=dt, params=params) for N in EV_HORIZONS for fin in (0, 1))
