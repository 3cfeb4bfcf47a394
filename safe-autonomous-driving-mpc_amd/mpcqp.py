"""ctypes binding of libmpcqp.so (include/mpcqp.h) — the MI355X batched tracking-MPC solver.

This is the product's host boundary.  It loads the in-tree HIP library and fails loudly when
it is missing or when a GPU context is asked for without a GPU: nothing falls back silently.  device=-1
selects the library's host backend explicitly (csrc/cpu_backend.h; BASELINE config 1's CPU path).  The
CPU restatement in oracle/ is test infrastructure and is never used here.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmpcqp.so")

MPC_OK, MPC_MAX_ITER, MPC_INFEASIBLE, MPC_NUMERICAL = 0, 1, 2, 3
# flag OR-ed onto the last QP's status when the SQP (sqp_iters > 1, sqp_tol > 0) stopped unconverged
MPC_SQP_UNCONVERGED, MPC_STATUS_MASK = 16, 15
STATUS_NAMES = {0: "ok", 1: "max_iter", 2: "infeasible", 3: "numerical"}
MAX_N = 63
MAX_OBS = 64

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


class MpcParams(C.Structure):
    """`mpc_params` of include/mpcqp.h (mirrors TrajectoryTracker.__init__, trajectory_tracking.py:17-47)."""
    _fields_ = [
        ("N", C.c_int), ("max_obs", C.c_int), ("dt", C.c_double),
        ("u_min", C.c_double * 2), ("u_max", C.c_double * 2),
        ("vehicle_radius", C.c_double),
        ("w_d", C.c_double), ("w_o", C.c_double), ("w_v", C.c_double), ("w_u1", C.c_double), ("w_u2", C.c_double),
        ("obstacle_safety_distance", C.c_double), ("max_time_2_obs", C.c_double), ("wheelbase", C.c_double),
        ("lane_width", C.c_double), ("safe_lane_margin", C.c_double),
        ("brake_distance", C.c_double), ("brake_accel", C.c_double),
        ("linearization", C.c_int), ("sqp_iters", C.c_int), ("max_iter", C.c_int), ("polish", C.c_int),
        ("tol", C.c_double), ("tol_mu", C.c_double), ("elastic_rho", C.c_double), ("sqp_tol", C.c_double),
    ]


class MpcFsm(C.Structure):
    """`mpc_fsm` of include/mpcqp.h (ObstaclesFSM parameters, trajectory_tracking.py:286-304)."""
    _fields_ = [("dynamic_obstacle", C.c_int), ("traffic_light", C.c_int),
                ("obs_trigger_s", C.c_double), ("obs_start_s", C.c_double), ("obs_v", C.c_double),
                ("obs_end_s", C.c_double), ("tl_pos", C.c_double), ("tl_trigger_s", C.c_double),
                ("tl_stop_duration", C.c_double)]


class MpcActor(C.Structure):
    """`mpc_actor` of include/mpcqp.h: one car or light of a traffic script (mpc_closed_loop_traffic)."""
    _fields_ = [("kind", C.c_int), ("trigger_s", C.c_double), ("pos_s", C.c_double), ("v", C.c_double),
                ("end_s", C.c_double), ("stop_duration", C.c_double)]


class MpcNoise(C.Structure):
    """`mpc_noise` of include/mpcqp.h: the sigmas of mpc_closed_loop_noisy (all zero: no noise)."""
    _fields_ = [("meas_sigma", C.c_double * 5), ("act_sigma", C.c_double * 2), ("proc_sigma", C.c_double * 5),
                ("perc_sigma", C.c_double * 2)]


class MpcWarm(C.Structure):
    """`mpc_warm` of include/mpcqp.h: how mpc_closed_loop_warm picks each step's linearisation point."""
    _fields_ = [("mode", C.c_int), ("tail", C.c_int), ("reset", C.c_int)]


class MpcError(RuntimeError):
    pass


EXPORTS = ["mpc_default_params", "mpc_create", "mpc_solve_batch", "mpc_solve_batch_device", "mpc_lookup",
           "mpc_set_params", "mpc_get_params", "mpc_last_error", "mpc_version", "mpc_destroy", "mpc_default_fsm",
           "mpc_closed_loop", "mpc_closed_loop_sweep", "mpc_cl_verdicts", "mpc_actors_from_fsm",
           "mpc_closed_loop_traffic", "mpc_closed_loop_convoy", "mpc_default_noise", "mpc_closed_loop_noisy",
           "mpc_closed_loop_traced", "mpc_default_warm", "mpc_closed_loop_warm", "mpc_noise_draw", "mpc_evaluate_batch", "mpc_evaluate_batch_device", "mpc_gradient_batch", "mpc_gradient_batch_device", "mpc_multipliers_batch", "mpc_multipliers_batch_device", "mpc_hessvec_batch", "mpc_hessvec_batch_device", "mpc_global_pose", "mpc_read_trajectory_json", "mpc_create_from_json",
           "mpc_comm_unique_id", "mpc_comm_create", "mpc_comm_info", "mpc_gather", "mpc_gather_host",
           "mpc_comm_allreduce_max", "mpc_comm_barrier", "mpc_comm_destroy"]
COMM_UID_BYTES = 128
# columns of mpc_closed_loop_sweep's per-ego summary (MPC_CLQ_*): shard.CL_FIELDS, then two status counters
CL_NQ = 13
CLQ_FIELDS = ("ego", "n_steps", "s_final", "max_dev", "u1_min", "u1_max", "u2_min", "u2_max", "max_step_ms",
              "min_obs_dist", "red_pass", "n_infeasible", "n_not_ok")
# verdict bits of mpc_cl_verdicts (MPC_CLV_*), sanity_checks.check_verdicts' order
CLV_NAMES = ("destination", "on_road", "steer_ok", "accel_ok", "realtime", "obstacle_ok", "light_ok", "passed")
# mpc_closed_loop_traffic: actor kinds (MPC_ACTOR_*), the script width limit, the columns of `extra` (MPC_TRX_*)
ACTOR_NONE, ACTOR_CAR, ACTOR_LIGHT = 0, 1, 2
MAX_ACTORS = 16
TRX_MAX_NOBS, TRX_N_RED_PASS, TRX_MIN_GAP_ACTOR = 0, 1, 2
TR_NX = 3
TRX_FIELDS = ("max_nobs", "n_red_pass", "min_gap_actor")
# mpc_closed_loop_convoy: the world size limit and the columns its `extra` adds to the traffic ones (MPC_CVX_*)
MAX_WORLD = 256
CVX_MIN_LEAD_GAP, CVX_MIN_LEAD_EGO, CVX_MAX_LEADERS = 3, 4, 5
CV_NX = 6
CVX_FIELDS = TRX_FIELDS + ("min_lead_gap", "min_lead_ego", "max_leaders")
# mpc_closed_loop_noisy: the noise channels (MPC_NZ_CH_*) and the columns its `extra` adds (MPC_NZX_*)
NZ_CH_MEAS, NZ_CH_ACT, NZ_CH_PROC, NZ_CH_PERC, NZ_CHANNELS = 0, 5, 7, 16, 48
NZX_U1A_MIN, NZX_U1A_MAX, NZX_U2A_MIN, NZX_U2A_MAX, NZX_N_CLAMPED = 6, 7, 8, 9, 10
NZ_NX = 11
NZX_FIELDS = CVX_FIELDS + ("u1a_min", "u1a_max", "u2a_min", "u2a_max", "n_clamped")
# mpc_closed_loop_traced: the lookahead limit and the columns of a gapq row (MPC_TG_*)
MAX_LOOK = 4
TG_N_CMP, TG_MAX_DS, TG_MAX_DD, TG_MAX_DV, TG_STEP_DD = 0, 1, 2, 3, 4
TG_NQ = 5
TG_FIELDS = ("n_cmp", "max_ds", "max_dd", "max_dv", "step_dd")
# mpc_closed_loop_warm: the modes, tails and reset bits of MpcWarm (MPC_WARM_*, MPC_WTAIL_*, MPC_WRESET_*) and the
# columns of a warmq row (MPC_WQ_*)
WARM_REFERENCE, WARM_CARRY = 0, 1
WTAIL_REFERENCE, WTAIL_HOLD = 0, 1
WRESET_NOBS, WRESET_INFEASIBLE, WRESET_MAX_ITER = 1, 2, 4
WQ_N_RESET, WQ_MAX_MOVE, WQ_STEP_MAX_MOVE, WQ_SUM_MOVE = 0, 1, 2, 3
WQ_NQ = 4
WQ_FIELDS = ("n_reset", "max_move", "step_max_move", "sum_move")
# mpc_evaluate_batch: the columns of its per-instance summary (MPC_EVQ_*)
EVQ_COST, EVQ_MIN_ROW, EVQ_ARGMIN_STAGE, EVQ_ARGMIN_KIND, EVQ_L1, EVQ_N_NEG = 0, 1, 2, 3, 4, 5
EVQ_MIN_LANE, EVQ_MIN_OBS, EVQ_MIN_V, EVQ_BOX = 6, 7, 8, 9
EV_NQ = 10
EVQ_FIELDS = ("cost", "min_row", "argmin_stage", "argmin_kind", "l1", "n_neg", "min_lane", "min_obs", "min_v", "box")
# mpc_gradient_batch: the columns of its per-instance summary (MPC_GRQ_*)
GRQ_COST, GRQ_GRAD_INF, GRQ_LAG_INF, GRQ_PG_INF, GRQ_COMPL, GRQ_MIN_LAM = 0, 1, 2, 3, 4, 5
GR_NQ = 6
GRQ_FIELDS = ("cost", "grad_inf", "lag_inf", "pg_inf", "compl", "min_lam")
# mpc_multipliers_batch: the list limit, the statuses (MPC_MU_*) and the columns of its summary (MPC_MUQ_*)
MAX_ACTIVE = 64
MU_OK, MU_OVERFLOW, MU_NO_FREE, MU_NONFINITE = 0, 1, 2, 3
MU_NAMES = ("ok", "overflow", "no_free", "nonfinite")
MUQ_STATUS, MUQ_N_ACTIVE, MUQ_N_FREE, MUQ_N_USED, MUQ_RESID, MUQ_MIN_PIVOT = 0, 1, 2, 3, 4, 5
MU_NQ = 6
MUQ_FIELDS = ("status", "n_active", "n_free", "n_used", "resid", "min_pivot")
# mpc_hessvec_batch: the direction limit, the modes (MPC_HV_*) and the columns of its summary (MPC_HVQ_*)
HV_MAX_DIRS = 128
HV_EXACT, HV_GAUSS_NEWTON = 0, 1
HV_MODES = {"exact": HV_EXACT, "gauss_newton": HV_GAUSS_NEWTON}
HVQ_COST, HVQ_MIN_RAYLEIGH, HVQ_MAX_RAYLEIGH, HVQ_ARGMIN_DIR, HVQ_N_NEG = 0, 1, 2, 3, 4
HV_NQ = 5
HVQ_FIELDS = ("cost", "min_rayleigh", "max_rayleigh", "argmin_dir", "n_neg")

_lib = None


def lib():
    """Load libmpcqp.so (raises if it has not been built: run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MpcError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    L.mpc_default_params.argtypes = [C.POINTER(MpcParams)]
    L.mpc_create.restype = C.c_int
    L.mpc_create.argtypes = [_dp, C.c_int, _dp, C.c_int, C.POINTER(MpcParams), C.c_int, C.POINTER(C.c_void_p)]
    L.mpc_solve_batch.restype = C.c_int
    L.mpc_solve_batch.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _ip, _dp, _dp, _dp, _dp, _ip, _ip]
    L.mpc_solve_batch_device.restype = C.c_int
    L.mpc_solve_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mpc_evaluate_batch.restype = C.c_int
    L.mpc_evaluate_batch.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _ip, _dp, _dp, _dp, _dp, _dp]
    L.mpc_evaluate_batch_device.restype = C.c_int
    L.mpc_evaluate_batch_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 9
    L.mpc_gradient_batch.restype = C.c_int
    L.mpc_gradient_batch.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
    L.mpc_gradient_batch_device.restype = C.c_int
    L.mpc_gradient_batch_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 11
    L.mpc_multipliers_batch.restype = C.c_int
    L.mpc_multipliers_batch.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _ip, _dp, C.c_double, C.c_double, C.c_double,
                                        _dp, _ip, _dp]
    L.mpc_hessvec_batch.restype = C.c_int
    L.mpc_hessvec_batch.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _ip, _dp, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp]
    L.mpc_hessvec_batch_device.restype = C.c_int
    L.mpc_hessvec_batch_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int] + \
        [C.c_void_p] * 5
    L.mpc_multipliers_batch_device.restype = C.c_int
    L.mpc_multipliers_batch_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_double] * 3 + \
        [C.c_void_p] * 4
    L.mpc_lookup.restype = C.c_int
    L.mpc_lookup.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
    L.mpc_set_params.restype = C.c_int
    L.mpc_set_params.argtypes = [C.c_void_p, C.POINTER(MpcParams)]
    L.mpc_get_params.restype = C.c_int
    L.mpc_get_params.argtypes = [C.c_void_p, C.POINTER(MpcParams)]
    L.mpc_last_error.restype = C.c_char_p
    L.mpc_version.restype = C.c_int
    L.mpc_destroy.argtypes = [C.c_void_p]
    L.mpc_default_fsm.argtypes = [C.POINTER(MpcFsm)]
    L.mpc_global_pose.restype = C.c_int
    L.mpc_global_pose.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
    L.mpc_read_trajectory_json.restype = C.c_int
    L.mpc_read_trajectory_json.argtypes = [C.c_char_p, _dp, C.c_int, _dp, C.c_int, _ip, _ip]
    L.mpc_create_from_json.restype = C.c_int
    L.mpc_create_from_json.argtypes = [C.c_char_p, C.POINTER(MpcParams), C.c_int, C.POINTER(C.c_void_p)]
    L.mpc_closed_loop.restype = C.c_int
    L.mpc_closed_loop.argtypes = [C.c_void_p, C.c_int, _dp, C.POINTER(MpcFsm), C.c_int, C.c_double, _dp, _dp, _dp,
                                  _ip, _ip, _ip, _dp]
    L.mpc_closed_loop_sweep.restype = C.c_int
    L.mpc_closed_loop_sweep.argtypes = [C.c_void_p, C.c_int, _dp, C.POINTER(MpcFsm), C.c_int, C.c_int, C.c_double, _dp,
                                        C.c_int, _ip, _dp, _dp, _dp, _ip, _ip, _ip, _dp]
    L.mpc_cl_verdicts.restype = C.c_int
    L.mpc_cl_verdicts.argtypes = [C.c_void_p, C.c_int, _dp, C.c_double, _ip, _ip]
    L.mpc_actors_from_fsm.restype = None
    L.mpc_actors_from_fsm.argtypes = [C.POINTER(MpcFsm), C.POINTER(MpcActor)]
    L.mpc_closed_loop_traffic.restype = C.c_int
    L.mpc_closed_loop_traffic.argtypes = [C.c_void_p, C.c_int, _dp, C.POINTER(MpcActor), C.c_int, C.c_int, C.c_int,
                                          C.c_double, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp, _ip, _ip, _ip, _dp,
                                          _ip, _dp]
    L.mpc_closed_loop_convoy.restype = C.c_int
    L.mpc_closed_loop_convoy.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, _dp, C.POINTER(MpcActor),
                                         C.c_int, C.c_int, C.c_int, C.c_double, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp,
                                         _ip, _ip, _ip, _dp, _ip, _ip, _dp]
    L.mpc_default_noise.restype = None
    L.mpc_default_noise.argtypes = [C.POINTER(MpcNoise)]
    L.mpc_closed_loop_noisy.restype = C.c_int
    L.mpc_closed_loop_noisy.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, _dp, C.POINTER(MpcActor),
                                        C.c_int, C.c_int, C.POINTER(MpcNoise), C.c_int, C.c_ulonglong, C.c_longlong,
                                        C.c_int, C.c_double, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, _ip,
                                        _ip, _ip, _dp, _ip, _ip, _dp]
    L.mpc_closed_loop_traced.restype = C.c_int
    L.mpc_closed_loop_traced.argtypes = L.mpc_closed_loop_noisy.argtypes + [_ip, C.c_int, _dp, _dp, _dp]
    if hasattr(L, "mpc_closed_loop_warm"):          # no version step: the entry is detected by its symbol
        L.mpc_default_warm.restype = None
        L.mpc_default_warm.argtypes = [C.POINTER(MpcWarm)]
        L.mpc_closed_loop_warm.restype = C.c_int
        L.mpc_closed_loop_warm.argtypes = L.mpc_closed_loop_traced.argtypes + [C.POINTER(MpcWarm), _dp, _dp]
    L.mpc_noise_draw.restype = C.c_int
    L.mpc_noise_draw.argtypes = [C.c_void_p, C.c_ulonglong, C.c_int, C.POINTER(C.c_longlong), _ip, _ip,
                                 C.POINTER(C.c_uint), _dp]
    L.mpc_comm_unique_id.restype = C.c_int
    L.mpc_comm_unique_id.argtypes = [C.c_char_p]
    L.mpc_comm_create.restype = C.c_int
    L.mpc_comm_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.mpc_comm_info.restype = C.c_int
    L.mpc_comm_info.argtypes = [C.c_void_p, _ip, _ip, _ip]
    L.mpc_gather.restype = C.c_int
    L.mpc_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
    L.mpc_gather_host.restype = C.c_int
    L.mpc_gather_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    L.mpc_comm_allreduce_max.restype = C.c_int
    L.mpc_comm_allreduce_max.argtypes = [C.c_void_p, _dp]
    L.mpc_comm_barrier.restype = C.c_int
    L.mpc_comm_barrier.argtypes = [C.c_void_p]
    L.mpc_comm_destroy.argtypes = [C.c_void_p]
    _lib = L
    return L


def last_error():
    return lib().mpc_last_error().decode()


def default_params(**kw):
    p = MpcParams()
    lib().mpc_default_params(C.byref(p))
    for k, v in kw.items():
        if k in ("u_min", "u_max"):
            arr = getattr(p, k)
            arr[0], arr[1] = float(v[0]), float(v[1])
        else:
            setattr(p, k, v)
    return p


def default_fsm(**kw):
    f = MpcFsm()
    lib().mpc_default_fsm(C.byref(f))
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def default_noise(**kw):
    """mpc_default_noise (every sigma 0) with the given fields set: meas_sigma [5], act_sigma [2], proc_sigma [5],
    perc_sigma [2]; a scalar sets every component of its field."""
    n = MpcNoise()
    lib().mpc_default_noise(C.byref(n))
    for k, v in kw.items():
        arr = getattr(n, k)
        vals = np.broadcast_to(np.asarray(v, np.float64), (len(arr),))
        for i, x in enumerate(vals):
            arr[i] = float(x)
    return n


def default_warm(**kw):
    """mpc_default_warm (WARM_REFERENCE, WTAIL_REFERENCE, no optional reset) with the given fields set: mode, tail,
    reset (an OR of WRESET_* bits)."""
    w = MpcWarm()
    lib().mpc_default_warm(C.byref(w))
    for k, v in kw.items():
        setattr(w, k, int(v))
    return w


def car(trigger_s, start_s, v, end_s):
    """A car of a traffic script: spawned at start_s once the ego reaches trigger_s, driving at v until end_s."""
    return MpcActor(kind=ACTOR_CAR, trigger_s=float(trigger_s), pos_s=float(start_s), v=float(v),
                    end_s=float(end_s))


def light(pos_s, trigger_s, stop_duration):
    """A light of a traffic script at pos_s: an obstacle while RED and closer than trigger_s; GREEN after the
    ego has stood in front of it for stop_duration seconds."""
    return MpcActor(kind=ACTOR_LIGHT, trigger_s=float(trigger_s), pos_s=float(pos_s),
                    stop_duration=float(stop_duration))


def actors_from_fsm(fsm):
    """mpc_actors_from_fsm: [car, light] restating an MpcFsm (ACTOR_NONE in place of a switch that is off)."""
    out = (MpcActor * 2)()
    lib().mpc_actors_from_fsm(C.byref(fsm), out)
    return [MpcActor.from_buffer_copy(a) for a in out]


def read_trajectory_json(path):
    """Native reader of the reference trajectory JSON (mpc_read_trajectory_json): returns (X [T,5], U [Tu,2])."""
    T, Tu = C.c_int(), C.c_int()
    b = os.fsencode(path)
    _check(lib().mpc_read_trajectory_json(b, None, 0, None, 0, C.byref(T), C.byref(Tu)), "mpc_read_trajectory_json")
    X = np.empty((T.value, 5))
    U = np.empty((Tu.value, 2))
    _check(lib().mpc_read_trajectory_json(b, X.ctypes.data_as(_dp), T.value, U.ctypes.data_as(_dp), Tu.value,
                                          C.byref(T), C.byref(Tu)), "mpc_read_trajectory_json")
    return X, U


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _pi(a):
    return None if a is None else a.ctypes.data_as(_ip)


def _check(rc, what):
    if rc != 0:
        raise MpcError(f"{what} failed (rc={rc}): {last_error()}")


def _s_stop(s_stop, s_max):
    """Where the closed loops end: s_stop, by default s_max - 1 (trajectory_tracking.py:395)."""
    if s_stop is None:
        if s_max is None:
            raise ValueError("give s_stop or s_max")
        s_stop = s_max - 1.0
    return s_stop


def _script_array(scripts):
    """(mpc_actor pointer, A, n_scripts) of closed_loop_traffic's `scripts` argument: None, one sequence of
    MpcActor (shared), or a sequence of such sequences of one length."""
    if scripts is None:
        return None, 0, 0
    scripts = list(scripts)
    rows = [scripts] if all(isinstance(a, MpcActor) for a in scripts) else [list(r) for r in scripts]
    n_scripts = len(rows)
    A = len(rows[0]) if rows else 0
    if any(len(r) != A for r in rows):
        raise ValueError("every script must have the same number of actors (pad with ACTOR_NONE)")
    buf = (MpcActor * max(n_scripts * A, 1))()
    for i, r in enumerate(rows):
        for a, act in enumerate(r):
            C.memmove(C.byref(buf, (i * A + a) * C.sizeof(MpcActor)), C.byref(act), C.sizeof(MpcActor))
    return C.cast(buf, C.POINTER(MpcActor)), A, n_scripts


class Solver:
    """One libmpcqp context: device-resident reference table + parameters (one HIP device)."""

    def __init__(self, X, U, params=None, device=0):
        self.X = np.ascontiguousarray(X, np.float64)
        self.U = np.ascontiguousarray(U, np.float64)
        if self.X.ndim != 2 or self.X.shape[1] != 5 or self.U.ndim != 2 or self.U.shape[1] != 2:
            raise ValueError("X must be [T,5] and U [Tu,2]")
        self.params = params if params is not None else default_params()
        h = C.c_void_p()
        _check(lib().mpc_create(_p(self.X), self.X.shape[0], _p(self.U), self.U.shape[0], C.byref(self.params),
                                int(device), C.byref(h)), "mpc_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            lib().mpc_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, params):
        _check(lib().mpc_set_params(self.h, C.byref(params)), "mpc_set_params")
        self.params = params

    def solve_batch(self, x0, obs=None, n_obs=None, ubar=None):
        """x0 [B,5]; obs [B,max_obs,2] (s, v); n_obs [B]; ubar [B,N,2] or None (reference warm start).
        Returns dict(u0 [B,2], U [B,N,2], Xpred [B,N+1,5], status [B], iters [B])."""
        p = self.params
        N, mo = p.N, p.max_obs
        x0 = np.ascontiguousarray(x0, np.float64).reshape(-1, 5)
        B = x0.shape[0]
        if obs is not None and np.asarray(obs).size > 0 and mo == 0:
            # the library refuses this too (MPC_E_ARG): an obstacle slab must never be dropped silently
            raise ValueError("obstacles given but params.max_obs == 0: set max_obs to the slab width")
        if obs is not None and mo > 0:
            obs = np.ascontiguousarray(obs, np.float64).reshape(B, mo, 2)
            n_obs = (np.full(B, mo, np.int32) if n_obs is None
                     else np.ascontiguousarray(n_obs, np.int32).reshape(B))
        else:
            obs, n_obs = None, None
        ub = None if ubar is None else np.ascontiguousarray(ubar, np.float64).reshape(B, N, 2)
        u0 = np.empty((B, 2)); U = np.empty((B, N, 2)); X = np.empty((B, N + 1, 5))
        st = np.empty(B, np.int32); it = np.empty(B, np.int32)
        _check(lib().mpc_solve_batch(self.h, B, _p(x0), _p(obs), _pi(n_obs), _p(ub), _p(u0), _p(U), _p(X), _pi(st),
                                     _pi(it)), "mpc_solve_batch")
        return dict(u0=u0, U=U, Xpred=X, status=st, iters=it)

    def solve_batch_device(self, B, x0_ptr, obs_ptr, nobs_ptr, ubar_ptr, u0_ptr, U_ptr, X_ptr, st_ptr, it_ptr,
                           stream=0):
        """Device-pointer variant (ints are raw device addresses, e.g. torch tensor.data_ptr())."""
        _check(lib().mpc_solve_batch_device(self.h, int(B), x0_ptr, obs_ptr, nobs_ptr, ubar_ptr, u0_ptr, U_ptr,
                                            X_ptr, st_ptr, it_ptr, C.c_void_p(stream)), "mpc_solve_batch_device")

    def _batch_inputs(self, x0, U, obs, n_obs, lam, what):
        """The inputs the evaluators share, as the library takes them: (B, N, max_obs, x0 [B,5], U [B,N,2],
        obs [B,max_obs,2] or None, n_obs [B] int32 or None (the library reads None as all max_obs rows; n_obs travels
        only with obs), lam [B,N,7+max_obs] or None).  `what` ends the refusal of a missing U."""
        p = self.params
        N, mo = p.N, p.max_obs
        x0 = np.ascontiguousarray(x0, np.float64).reshape(-1, 5)
        B = x0.shape[0]
        if U is None:
            raise ValueError(f"U is required: the control sequences to {what}")
        U = np.ascontiguousarray(U, np.float64).reshape(B, N, 2)
        if obs is not None and np.asarray(obs).size > 0 and mo == 0:
            raise ValueError("obstacles given but params.max_obs == 0: set max_obs to the slab width")
        if obs is not None and mo > 0:
            obs = np.ascontiguousarray(obs, np.float64).reshape(B, mo, 2)
            n_obs = None if n_obs is None else np.ascontiguousarray(n_obs, np.int32).reshape(B)
        else:
            obs, n_obs = None, None
        if lam is not None:
            lam = np.ascontiguousarray(lam, np.float64).reshape(B, N, 7 + mo)
        return B, N, mo, x0, U, obs, n_obs, lam

    def evaluate_batch(self, x0, U, obs=None, n_obs=None, rows=False):
        """mpc_evaluate_batch: the reference's measures of ANY control sequences U [B,N,2] from x0 [B,5] (obs, n_obs
        as in solve_batch).  Returns dict(Xpred [B,N+1,5] = predict(x0, U), summary [B,10] (columns EVQ_FIELDS:
        cost, min / argmin of the constraint rows, L1 violation, negative rows, minima per row family, box
        excess), terms [B,5] (cost shares d, o, v, u1, u2)) and, with rows=True, rows [B,N,7+max_obs] (columns:
        six lane rows, v, the obstacles, NaN past n_obs; constraint_rows() gives the reference's vector)."""
        B, N, mo, x0, U, obs, n_obs, _ = self._batch_inputs(x0, U, obs, n_obs, None, "evaluate")
        X = np.empty((B, N + 1, 5)); summary = np.empty((B, EV_NQ)); terms = np.empty((B, 5))
        R = np.empty((B, N, 7 + mo)) if rows else None
        _check(lib().mpc_evaluate_batch(self.h, B, _p(x0), _p(obs), _pi(n_obs), _p(U), _p(X), _p(summary), _p(terms),
                                        _p(R)), "mpc_evaluate_batch")
        out = dict(Xpred=X, summary=summary, terms=terms)
        if rows:
            out["rows"] = R
        return out

    def evaluate_batch_device(self, B, x0_ptr, obs_ptr, nobs_ptr, U_ptr, X_ptr, summary_ptr, terms_ptr, rows_ptr,
                              stream=0):
        """Device-pointer variant (ints are raw device addresses, e.g. torch tensor.data_ptr(); 0 / None = NULL)."""
        _check(lib().mpc_evaluate_batch_device(self.h, int(B), x0_ptr, obs_ptr, nobs_ptr, U_ptr, X_ptr, summary_ptr,
                                               terms_ptr, rows_ptr, C.c_void_p(stream)), "mpc_evaluate_batch_device")

    def gradient_batch(self, x0, U, obs=None, n_obs=None, lam=None, costate=False):
        """mpc_gradient_batch: the gradients of what evaluate_batch computes at ANY control sequences U [B,N,2] from
        x0 [B,5] (obs, n_obs as in evaluate_batch).  lam [B,N,7+max_obs] or None: row weights in the layout of
        evaluate_batch's rows (columns past n_obs are not read).  Returns dict(grad [B,N,2] = d cost / d U,
        gx0 [B,5] = d cost / d x0, summary [B,6] (columns GRQ_FIELDS: cost, max |grad|, max |grad - jtl|, the
        projected-gradient measure, max |lam g|, min lam)) and, with lam, jtl [B,N,2] = J' lam of the constraint
        rows; with costate=True, costate [B,N,5] = p_1..p_N of the cost."""
        B, N, mo, x0, U, obs, n_obs, lam = self._batch_inputs(x0, U, obs, n_obs, lam, "differentiate at")
        grad = np.empty((B, N, 2)); gx0 = np.empty((B, 5)); summary = np.empty((B, GR_NQ))
        jtl = np.empty((B, N, 2)) if lam is not None else None
        P = np.empty((B, N, 5)) if costate else None
        _check(lib().mpc_gradient_batch(self.h, B, _p(x0), _p(obs), _pi(n_obs), _p(U), _p(lam), _p(grad), _p(jtl),
                                        _p(gx0), _p(P), _p(summary)), "mpc_gradient_batch")
        out = dict(grad=grad, gx0=gx0, summary=summary)
        if lam is not None:
            out["jtl"] = jtl
        if costate:
            out["costate"] = P
        return out

    def gradient_batch_device(self, B, x0_ptr, obs_ptr, nobs_ptr, U_ptr, lam_ptr, grad_ptr, jtl_ptr, gx0_ptr,
                              costate_ptr, summary_ptr, stream=0):
        """Device-pointer variant (ints are raw device addresses, e.g. torch tensor.data_ptr(); 0 / None = NULL)."""
        _check(lib().mpc_gradient_batch_device(self.h, int(B), x0_ptr, obs_ptr, nobs_ptr, U_ptr, lam_ptr, grad_ptr,
                                               jtl_ptr, gx0_ptr, costate_ptr, summary_ptr, C.c_void_p(stream)),
               "mpc_gradient_batch_device")

    def multipliers_batch(self, x0, U, obs=None, n_obs=None, active_tol=1e-6, bound_tol=1e-9, rank_tol=1e-10,
                          outputs=("lam", "active", "summary")):
        """mpc_multipliers_batch: least-squares multiplier estimates of the constraint rows at ANY control sequences
        U [B,N,2] from x0 [B,5] (obs, n_obs as in evaluate_batch): grad = J' lam over the rows with g <= active_tol
        and the control components more than bound_tol inside their bounds, rows dropped greedily by rank_tol.
        Returns dict(lam [B,N,7+max_obs] in the layout of evaluate_batch's rows (0 where nothing is estimated; hand
        it to gradient_batch as it is), active [B,64] int32 (the active rows in the reference's order as
        (stage - 1) * (7 + max_obs) + column, -1 past the count), summary [B,6] (columns MUQ_FIELDS: status MU_*,
        active rows, free components, rows kept, least-squares residual, least pivot ratio)); `outputs` names the
        ones to compute."""
        B, N, mo, x0, U, obs, n_obs, _ = self._batch_inputs(x0, U, obs, n_obs, None, "estimate the multipliers at")
        out = {}
        if "lam" in outputs:
            out["lam"] = np.empty((B, N, 7 + mo))
        if "active" in outputs:
            out["active"] = np.empty((B, MAX_ACTIVE), np.int32)
        if "summary" in outputs:
            out["summary"] = np.empty((B, MU_NQ))
        _check(lib().mpc_multipliers_batch(self.h, B, _p(x0), _p(obs), _pi(n_obs), _p(U), float(active_tol),
                                           float(bound_tol), float(rank_tol), _p(out.get("lam")),
                                           _pi(out.get("active")), _p(out.get("summary"))), "mpc_multipliers_batch")
        return out

    def multipliers_batch_device(self, B, x0_ptr, obs_ptr, nobs_ptr, U_ptr, lam_ptr, active_ptr, summary_ptr,
                                 active_tol=1e-6, bound_tol=1e-9, rank_tol=1e-10, stream=0):
        """Device-pointer variant (ints are raw device addresses, e.g. torch tensor.data_ptr(); 0 / None = NULL)."""
        _check(lib().mpc_multipliers_batch_device(self.h, int(B), x0_ptr, obs_ptr, nobs_ptr, U_ptr, float(active_tol),
                                                  float(bound_tol), float(rank_tol), lam_ptr, active_ptr, summary_ptr,
                                                  C.c_void_p(stream)), "mpc_multipliers_batch_device")

    def hessvec_batch(self, x0, U, V=None, M=None, lam=None, obs=None, n_obs=None, mode="exact",
                      outputs=("HV", "JV", "curv", "summary")):
        """mpc_hessvec_batch: Hessian-vector products and row tangents at ANY control sequences U [B,N,2] from x0 [B,5]
        (obs, n_obs, lam as in gradient_batch).  V [B,M,N,2]: the directions; V None: the unit vectors e_0..e_M-1 of
        the flattened U (M defaults to 2N, the dense Hessian).  mode "exact" (the Hessian of cost - lam . g) or
        "gauss_newton" (the cost's with the dynamics linearised), or the HV_* integers.  Returns dict(HV [B,M,N,2] =
        H v, JV [B,M,N,7+max_obs] = J v in the layout of evaluate_batch's rows, curv [B,M,2] = (v'Hv, v'v),
        summary [B,5] (columns HVQ_FIELDS: cost, min and max Rayleigh quotient, its first minimising direction, the
        directions of negative curvature)); `outputs` names the ones to compute."""
        B, N, mo, x0, U, obs, n_obs, lam = self._batch_inputs(x0, U, obs, n_obs, lam, "differentiate at")
        if V is not None:
            V = np.ascontiguousarray(V, np.float64)
            M = V.size // max(B * N * 2, 1) if M is None else int(M)
            V = V.reshape(B, M, N, 2)
        elif M is None:
            M = 2 * N
        M = int(M)
        Mo = max(M, 0)
        shapes = dict(HV=(B, Mo, N, 2), JV=(B, Mo, N, 7 + mo), curv=(B, Mo, 2), summary=(B, HV_NQ))
        out = {k: np.empty(shapes[k]) for k in shapes if k in outputs}
        _check(lib().mpc_hessvec_batch(self.h, B, _p(x0), _p(obs), _pi(n_obs), _p(U), _p(lam), M, _p(V),
                                       int(HV_MODES.get(mode, mode)), _p(out.get("HV")), _p(out.get("JV")),
                                       _p(out.get("curv")), _p(out.get("summary"))), "mpc_hessvec_batch")
        return out

    def hessvec_batch_device(self, B, x0_ptr, obs_ptr, nobs_ptr, U_ptr, lam_ptr, M, V_ptr, mode, HV_ptr, JV_ptr,
                             curv_ptr, summary_ptr, stream=0):
        """Device-pointer variant (ints are raw device addresses, e.g. torch tensor.data_ptr(); 0 / None = NULL)."""
        _check(lib().mpc_hessvec_batch_device(self.h, int(B), x0_ptr, obs_ptr, nobs_ptr, U_ptr, lam_ptr, int(M), V_ptr,
                                              int(HV_MODES.get(mode, mode)), HV_ptr, JV_ptr, curv_ptr, summary_ptr,
                                              C.c_void_p(stream)), "mpc_hessvec_batch_device")

    def hessian_batch(self, x0, U, lam=None, obs=None, n_obs=None, mode="exact"):
        """The dense second-order data of U in one call (V NULL, M = 2N): dict(H [B,2N,2N] = the Hessian of
        cost - lam . g in the flattened U (index 2k + c), J [B,N*(7+max_obs),2N] = the Jacobian of the rows in the
        flattened layout of evaluate_batch's rows (NaN rows past n_obs), curv, summary as hessvec_batch)."""
        N = self.params.N
        r = self.hessvec_batch(x0, U, None, 2 * N, lam, obs, n_obs, mode)
        B = r["HV"].shape[0]
        return dict(H=r["HV"].reshape(B, 2 * N, 2 * N), J=r["JV"].reshape(B, 2 * N, -1).transpose(0, 2, 1).copy(),
                    curv=r["curv"], summary=r["summary"])

    def certify_batch(self, x0, U, obs=None, n_obs=None, active_tol=1e-6, bound_tol=1e-9, rank_tol=1e-10):
        """The first-order certificate of U: multipliers_batch, then gradient_batch with its lam.  Returns
        dict(lam, active, multipliers [B,6] (MUQ_FIELDS), summary [B,6] (GRQ_FIELDS: with lam, so pg_inf is the
        projected gradient of the Lagrangian, compl the complementarity and min_lam the least multiplier), grad,
        jtl)."""
        m = self.multipliers_batch(x0, U, obs, n_obs, active_tol, bound_tol, rank_tol)
        g = self.gradient_batch(x0, U, obs, n_obs, lam=m["lam"])
        return dict(lam=m["lam"], active=m["active"], multipliers=m["summary"], summary=g["summary"], grad=g["grad"],
                    jtl=g["jtl"])

    def closed_loop(self, x_init, fsm=None, max_steps=1000, s_stop=None, s_max=None):
        """Batched run_simulation (trajectory_tracking.py:377-443) on the device.
        x_init [B,5]; fsm: MpcFsm or None; the loop runs while s <= s_stop (default s_max - 1, :395).
        Returns dict(hist_x [B,max_steps+1,5], hist_u [B,max_steps,2], hist_obs_s [B,max_steps],
        hist_tl [B,max_steps], hist_status [B,max_steps], n_steps [B], step_ms [max_steps])."""
        x_init = np.ascontiguousarray(x_init, np.float64).reshape(-1, 5)
        B = x_init.shape[0]
        s_stop = _s_stop(s_stop, s_max)
        hx = np.empty((B, max_steps + 1, 5)); hu = np.empty((B, max_steps, 2)); ho = np.empty((B, max_steps))
        ht = np.empty((B, max_steps), np.int32); hs = np.empty((B, max_steps), np.int32)
        ns = np.empty(B, np.int32); sm = np.empty(max_steps)
        _check(lib().mpc_closed_loop(self.h, B, _p(x_init), None if fsm is None else C.byref(fsm), int(max_steps),
                                     float(s_stop), _p(hx), _p(hu), _p(ho), _pi(ht), _pi(hs), _pi(ns), _p(sm)),
               "mpc_closed_loop")
        return dict(hist_x=hx, hist_u=hu, hist_obs_s=ho, hist_tl=ht, hist_status=hs, n_steps=ns, step_ms=sm)

    def closed_loop_sweep(self, x_init, scenarios, max_steps, s_stop=None, s_max=None, hist_egos=(), lo=0):
        """mpc_closed_loop_sweep: the batched closed loop with a scenario per ego, the check quantities
        accumulated while it runs, and histories only for the egos in `hist_egos`.
        x_init [B,5]; scenarios: None (no scenario), one MpcFsm (shared), or a sequence / ctypes array of B
        MpcFsm (ego b runs scenarios[b]); the loop runs while s <= s_stop (default s_max - 1).
        Returns dict(quant [B,13] (columns CLQ_FIELDS; `lo`, the shard offset, is added to column 0), n_steps [B],
        step_ms [max_steps], hist_egos [n_hist], hist_x [n_hist,max_steps+1,5], hist_u [n_hist,max_steps,2],
        hist_obs_s, hist_tl, hist_status [n_hist,max_steps]: row k belongs to ego hist_egos[k])."""
        x_init = np.ascontiguousarray(x_init, np.float64).reshape(-1, 5)
        B = x_init.shape[0]
        s_stop = _s_stop(s_stop, s_max)
        if scenarios is None:
            fsm, n_fsm = None, 0
        elif isinstance(scenarios, MpcFsm):
            fsm, n_fsm = C.pointer(scenarios), 1
        else:
            n_fsm = len(scenarios)
            if isinstance(scenarios, C.Array):
                arr = scenarios
            else:
                arr = (MpcFsm * max(n_fsm, 1))()
                for i, f in enumerate(scenarios):
                    C.memmove(C.byref(arr, i * C.sizeof(MpcFsm)), C.byref(f), C.sizeof(MpcFsm))
            fsm = C.cast(arr, C.POINTER(MpcFsm))
        he = np.ascontiguousarray(hist_egos, np.int32).ravel()
        nh = he.size
        quant = np.empty((B, CL_NQ))
        ns = np.empty(B, np.int32); sm = np.empty(max_steps)
        hx = hu = ho = ht = hs = None
        if nh:
            hx = np.empty((nh, max_steps + 1, 5)); hu = np.empty((nh, max_steps, 2)); ho = np.empty((nh, max_steps))
            ht = np.empty((nh, max_steps), np.int32); hs = np.empty((nh, max_steps), np.int32)
        _check(lib().mpc_closed_loop_sweep(self.h, B, _p(x_init), fsm, int(n_fsm), int(max_steps), float(s_stop),
                                           _p(quant), nh, _pi(he) if nh else None, _p(hx), _p(hu), _p(ho), _pi(ht),
                                           _pi(hs), _pi(ns), _p(sm)), "mpc_closed_loop_sweep")
        quant[:, 0] += lo
        if not nh:
            hx = np.empty((0, max_steps + 1, 5)); hu = np.empty((0, max_steps, 2)); ho = np.empty((0, max_steps))
            ht = np.empty((0, max_steps), np.int32); hs = np.empty((0, max_steps), np.int32)
        return dict(quant=quant, n_steps=ns, step_ms=sm, hist_egos=he, hist_x=hx, hist_u=hu, hist_obs_s=ho,
                    hist_tl=ht, hist_status=hs)

    def closed_loop_traffic(self, x_init, scripts, max_steps, s_stop=None, s_max=None, hist_egos=(), lo=0):
        """mpc_closed_loop_traffic: closed_loop_sweep with a traffic script of up to MAX_ACTORS actors per ego.
        x_init [B,5]; scripts: None (no script), one sequence of MpcActor (shared by all egos), or a sequence of
        B such sequences of one length A (ego b runs scripts[b]).
        Returns closed_loop_sweep's dict with hist_car_s in place of hist_obs_s and hist_tl a bitmask (bit a:
        actor a is a GREEN light), plus extra [B,3] (columns TRX_FIELDS), hist_nobs [n_hist,max_steps] and
        hist_slab [n_hist,max_steps,A,2] (NaN past n_obs)."""
        return self._closed_loop_scripted("mpc_closed_loop_traffic", TR_NX, x_init, scripts, max_steps, s_stop, s_max,
                                          hist_egos, lo)

    def closed_loop_convoy(self, x_init, W, K, lead_range=np.inf, scripts=None, max_steps=2000, s_stop=None,
                           s_max=None, hist_egos=(), lo=0):
        """mpc_closed_loop_convoy: closed_loop_traffic in which the egos [w*W, (w+1)*W) of a world see each other.
        Per step an ego's slab holds its script's entries, then (s, v) of its up to K nearest leaders: the egos of
        its world that are ahead (larger s, on equal s the lower index) and still in the loop, cut at the first
        gap >= lead_range.  x_init [B,5], B a multiple of W; scripts as in closed_loop_traffic.
        Returns closed_loop_traffic's dict with extra [B,6] (columns CVX_FIELDS; min_lead_ego is a batch index,
        the shard offset `lo` is added to it), hist_slab [n_hist,max_steps,A+K,2] and hist_lead
        [n_hist,max_steps,K] (the leaders' batch indices of this call in slab order, -1 past them)."""
        return self._closed_loop_scripted("mpc_closed_loop_convoy", CV_NX, x_init, scripts, max_steps, s_stop, s_max,
                                          hist_egos, lo, world=(W, K, lead_range))

    def closed_loop_noisy(self, x_init, W=1, K=0, lead_range=np.inf, scripts=None, max_steps=2000, s_stop=None,
                          s_max=None, hist_egos=(), noise=None, seed=0, lo=0):
        """mpc_closed_loop_noisy: closed_loop_convoy with seeded noise between the world and the solver.  noise:
        None (no noise), one MpcNoise (shared), or a sequence of B MpcNoise.  Ego b draws as global ego lo + b
        (`lo` is passed as ego_offset and added to the index columns like closed_loop_convoy's), so a row depends
        on (seed, lo + b) and its world only.
        Returns closed_loop_convoy's dict with extra [B,11] (columns NZX_FIELDS), hist_ua [n_hist,max_steps,2] (the
        applied controls; hist_u stays the commanded ones) and hist_xm [n_hist,max_steps,5] (the state the solver
        was given)."""
        return self._closed_loop_noisy(x_init, W, K, lead_range, scripts, max_steps, s_stop, s_max, hist_egos, noise,
                                       seed, lo, None)

    def closed_loop_traced(self, x_init, W=1, K=0, lead_range=np.inf, scripts=None, max_steps=2000, s_stop=None,
                           s_max=None, hist_egos=(), noise=None, seed=0, lo=0, lookahead=(), preds=False, plans=False):
        """mpc_closed_loop_traced: closed_loop_noisy that keeps the plan behind each applied control.  lookahead: up
        to MAX_LOOK distinct stages j in 1 .. N; preds / plans: keep the solver's Xpred / U of every step for the
        egos of hist_egos.
        Returns closed_loop_noisy's dict, plus gapq [B,len(lookahead),5] (columns TG_FIELDS: the plan-vs-outcome gaps
        of every ego, stage j of the prediction made at step t against the true state j steps later) when lookahead
        is not empty, hist_pred [n_hist,max_steps,N+1,5] with preds and hist_plan [n_hist,max_steps,N,2] with plans
        (NaN past n_steps)."""
        return self._closed_loop_noisy(x_init, W, K, lead_range, scripts, max_steps, s_stop, s_max, hist_egos, noise,
                                       seed, lo, (lookahead, preds, plans))

    def closed_loop_warm(self, x_init, W=1, K=0, lead_range=np.inf, scripts=None, max_steps=2000, s_stop=None,
                         s_max=None, hist_egos=(), noise=None, seed=0, lo=0, lookahead=(), preds=False, plans=False,
                         warm=None, warmq=False, ubars=False):
        """mpc_closed_loop_warm: closed_loop_traced whose steps may linearise about the ego's previous plan shifted by
        one stage (the real-time iteration).  warm: an MpcWarm (default_warm(mode=WARM_CARRY, ...)), None for the
        defaults (the reference warm start every step: closed_loop_traced).
        Returns closed_loop_traced's dict, plus warmq [B,4] (columns WQ_FIELDS) with warmq=True and hist_ubar
        [n_hist,max_steps,N,2] (the linearisation point the solver was handed; NaN past n_steps) with ubars=True."""
        return self._closed_loop_noisy(x_init, W, K, lead_range, scripts, max_steps, s_stop, s_max, hist_egos, noise,
                                       seed, lo, (lookahead, preds, plans), (warm, warmq, ubars))

    def _closed_loop_noisy(self, x_init, W, K, lead_range, scripts, max_steps, s_stop, s_max, hist_egos, noise, seed,
                           lo, trace, warm=None):
        """closed_loop_noisy (trace None), closed_loop_traced (trace = (lookahead, preds, plans)) or closed_loop_warm
        (warm = (MpcWarm or None, warmq, ubars) as well)."""
        entry = "mpc_closed_loop_" + ("noisy" if trace is None else "traced" if warm is None else "warm")
        return self._closed_loop_scripted(entry, NZ_NX, x_init, scripts, max_steps, s_stop, s_max, hist_egos, lo,
                                          world=(W, K, lead_range), noise=(noise, seed), trace=trace, warm=warm)

    def _closed_loop_scripted(self, entry, nx, x_init, scripts, max_steps, s_stop, s_max, hist_egos, lo, world=None,
                              noise=None, trace=None, warm=None):
        """The body of closed_loop_traffic (world None), closed_loop_convoy (world = (W, K, lead_range)) and
        _closed_loop_noisy (noise = (noise, seed) as well; trace and warm as there): allocates the outputs (extra is
        [B,nx]), calls the library's `entry` and adds `lo` to the index columns."""
        x_init = np.ascontiguousarray(x_init, np.float64).reshape(-1, 5)
        B = x_init.shape[0]
        s_stop = _s_stop(s_stop, s_max)
        arr, A, n_scripts = _script_array(scripts)
        W, K, lead_range = world or (1, 0, np.inf)
        K = int(K)
        noisy = noise is not None
        if noisy:
            noise, seed = noise
            if noise is None:
                nz, n_noise = None, 0
            elif isinstance(noise, MpcNoise):
                nz, n_noise = C.pointer(noise), 1
            else:
                n_noise = len(noise)
                if isinstance(noise, C.Array):
                    buf = noise
                else:
                    buf = (MpcNoise * max(n_noise, 1))()
                    for i, z in enumerate(noise):
                        C.memmove(C.byref(buf, i * C.sizeof(MpcNoise)), C.byref(z), C.sizeof(MpcNoise))
                nz = C.cast(buf, C.POINTER(MpcNoise))
        he = np.ascontiguousarray(hist_egos, np.int32).ravel()
        nh = he.size
        quant = np.empty((B, CL_NQ)); extra = np.empty((B, nx))
        ns = np.empty(B, np.int32); sm = np.empty(max_steps)
        hx = np.empty((nh, max_steps + 1, 5)); hu = np.empty((nh, max_steps, 2)); hc = np.empty((nh, max_steps))
        ht = np.empty((nh, max_steps), np.int32); hs = np.empty((nh, max_steps), np.int32)
        hn = np.empty((nh, max_steps), np.int32); hl = np.empty((nh, max_steps, max(A + K, 0), 2))
        g = (lambda a: _p(a) if nh else None)          # no history pointer without a history ego
        gi = (lambda a: _pi(a) if nh else None)
        out = dict(quant=quant, extra=extra, n_steps=ns, step_ms=sm, hist_egos=he, hist_x=hx, hist_u=hu)
        args = (self.h, B) + ((int(W), K, float(lead_range)) if world else ())     # the entry's order from here on
        args += (_p(x_init), arr, int(A), int(n_scripts))
        if noisy:
            args += (nz, int(n_noise), int(seed), int(lo))
            out.update(hist_ua=np.empty((nh, max_steps, 2)), hist_xm=np.empty((nh, max_steps, 5)))
        args += (int(max_steps), float(s_stop), _p(quant), _p(extra), nh, gi(he), g(hx), g(hu))
        if noisy:
            args += (g(out["hist_ua"]), g(out["hist_xm"]))
        args += (g(hc), gi(ht), gi(hs), gi(hn), g(hl) if A + K > 0 else None)
        out.update(hist_car_s=hc, hist_tl=ht, hist_status=hs, hist_nobs=hn, hist_slab=hl)
        if world:
            out["hist_lead"] = np.empty((nh, max_steps, max(K, 0)), np.int32)
            args += (gi(out["hist_lead"]) if K > 0 else None,)
        args += (_pi(ns), _p(sm))
        if trace is not None:
            lookahead, preds, plans = trace
            N = self.params.N
            look = np.ascontiguousarray(lookahead, np.int32).ravel()
            if look.size:
                out["gapq"] = np.empty((B, look.size, TG_NQ))
            if preds:
                out["hist_pred"] = np.empty((nh, max_steps, N + 1, 5))
            if plans:
                out["hist_plan"] = np.empty((nh, max_steps, N, 2))
            args += (_pi(look) if look.size else None, int(look.size), _p(out.get("gapq")), g(out.get("hist_pred")),
                     g(out.get("hist_plan")))
        if warm is not None:
            how, want_q, want_ubar = warm
            if want_q:
                out["warmq"] = np.empty((B, WQ_NQ))
            if want_ubar:
                out["hist_ubar"] = np.empty((nh, max_steps, N, 2))
            args += (None if how is None else C.byref(how), _p(out.get("warmq")), g(out.get("hist_ubar")))
        _check(getattr(lib(), entry)(*args), entry)
        quant[:, 0] += lo
        if world:
            extra[:, CVX_MIN_LEAD_EGO] += np.where(extra[:, CVX_MIN_LEAD_EGO] >= 0, lo, 0)
        return out

    def noise_draw(self, seed, ego, step, channel):
        """mpc_noise_draw on this context's backend: the Philox words [n,4] (uint32) and the variates z [n] of
        (seed, ego[i], step[i], channel[i]); the index arrays broadcast against each other."""
        ego, step, channel = np.broadcast_arrays(np.asarray(ego, np.int64), np.asarray(step, np.int32),
                                                 np.asarray(channel, np.int32))
        ego = np.ascontiguousarray(ego.ravel(), np.int64)
        step = np.ascontiguousarray(step.ravel(), np.int32)
        channel = np.ascontiguousarray(channel.ravel(), np.int32)
        n = ego.size
        words = np.empty((n, 4), np.uint32); z = np.empty(n)
        _check(lib().mpc_noise_draw(self.h, int(seed), n, ego.ctypes.data_as(C.POINTER(C.c_longlong)), _pi(step),
                                    _pi(channel), words.ctypes.data_as(C.POINTER(C.c_uint)), _p(z)),
               "mpc_noise_draw")
        return words, z

    def cl_verdicts(self, quant, s_total):
        """mpc_cl_verdicts: the restated acceptance verdicts (sanity_checks.check_verdicts, with this context's
        control bounds) of a sweep's quantities.  Returns (verdicts [B] int32 bitmask, bit k = CLV_NAMES[k];
        counts [8] egos with each bit set)."""
        quant = np.ascontiguousarray(quant, np.float64).reshape(-1, CL_NQ)
        v = np.empty(quant.shape[0], np.int32)
        counts = np.zeros(8, np.int32)
        _check(lib().mpc_cl_verdicts(self.h, quant.shape[0], _p(quant), float(s_total), _pi(v), _pi(counts)),
               "mpc_cl_verdicts")
        return v, counts

    def global_pose(self, s, d):
        """TrajectoryLoader.get_global_pose on the device table, batched: s, d [n] -> [n, 3] (x, y, psi)."""
        s = np.ascontiguousarray(s, np.float64).ravel()
        d = np.ascontiguousarray(d, np.float64).ravel()
        if s.shape != d.shape:
            raise ValueError("s and d must have the same length")
        out = np.empty((s.size, 3))
        _check(lib().mpc_global_pose(self.h, s.size, _p(s), _p(d), _p(out)), "mpc_global_pose")
        return out

    def lookup(self, s):
        s = np.ascontiguousarray(s, np.float64).ravel()
        st = np.empty((s.size, 5)); ct = np.empty((s.size, 2))
        _check(lib().mpc_lookup(self.h, s.size, _p(s), _p(st), _p(ct)), "mpc_lookup")
        return st, ct


def comm_unique_id():
    """mpc_comm_unique_id: the RCCL unique id (COMM_UID_BYTES bytes) that rank 0 hands to every rank."""
    buf = C.create_string_buffer(COMM_UID_BYTES)
    _check(lib().mpc_comm_unique_id(buf), "mpc_comm_unique_id")
    return buf.raw


class Comm:
    """One libmpcqp ego-shard communicator (mpc_comm_*: RCCL over xGMI behind the C ABI, include/mpcqp.h).
    Collective construction: every rank of `nranks` calls it with rank 0's unique id."""

    def __init__(self, uid, nranks, rank, device):
        if len(uid) != COMM_UID_BYTES:
            raise ValueError(f"uid must be {COMM_UID_BYTES} bytes")
        h = C.c_void_p()
        _check(lib().mpc_comm_create(uid, int(nranks), int(rank), int(device), C.byref(h)), "mpc_comm_create")
        self.h, self.nranks, self.rank, self.device = h, int(nranks), int(rank), int(device)

    def gather(self, payload, root=0):
        """mpc_gather_host of a uint8 payload (the same size on every rank): the list of every rank's payload on
        the root, None elsewhere."""
        buf = np.ascontiguousarray(payload, np.uint8).ravel()
        out = np.empty(buf.size * self.nranks, np.uint8) if self.rank == root else None
        _check(lib().mpc_gather_host(self.h, buf.ctypes.data, buf.size, None if out is None else out.ctypes.data,
                                     int(root)), "mpc_gather_host")
        return None if out is None else [out[i * buf.size:(i + 1) * buf.size] for i in range(self.nranks)]

    def gather_device(self, send_ptr, nbytes, recv_ptr, root=0, stream=0):
        """mpc_gather on device buffers (raw addresses), asynchronous on `stream`."""
        _check(lib().mpc_gather(self.h, send_ptr, int(nbytes), recv_ptr, int(root), C.c_void_p(stream)),
               "mpc_gather")

    def allreduce_max(self, x):
        v = C.c_double(float(x))
        _check(lib().mpc_comm_allreduce_max(self.h, C.byref(v)), "mpc_comm_allreduce_max")
        return v.value

    def barrier(self):
        _check(lib().mpc_comm_barrier(self.h), "mpc_comm_barrier")

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            lib().mpc_comm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
