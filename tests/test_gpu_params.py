"""GPU tests of the tracker library away from mpc_default_params (params_cases.py; tests/test_params_cpu.py runs the
same checks on the oracle and the host backend).

KParams (csrc/device_common.h) carries 20 doubles that the host fills from mpc_params, the lane half-width is folded
from three fields, and the specialised (NT = 20, 30, 40) and crossover kernels were tuned on the default problem;
every other GPU test runs the default weights, dt, bounds and geometry.  Under each of the six parameter sets of
tests/golden/params_golden.npz (A, B: every field; W, U, G, T: weights, bounds, geometry, dt alone):
  - the warm start and the rollout equal the reference's bit for bit, the QP solution is within TOL_CERT of the
    KKT-certified optimum of the reference's QP (the golden checks of test_params_cpu.py on device 0);
  - mpc_evaluate_batch on the device equals the host backend bit for bit;
  - 203-ego batches (C2, C3, C5 at N = 15, 20, 25, 30, 40: every lane group, the specialised and the runtime
    horizons, a partial last wavefront) agree with the oracle at tol_u(N), and after three SQP iterations at the
    tolerances of test_gpu_horizons.test_sqp_horizons_vs_oracle; the batches keep crossover-certified, deferred and
    elastic instances;
  - the split launch pair equals the one-kernel launch bit for bit;
  - the device closed loop equals the shim's loop at set A's dt and bounds;
  - brake_distance and brake_accel, which the reference hard-codes, against the oracle's warm start.
No tolerance is new: TOL_CERT, tol_u and the SQP pair are test_gpu_parity.py's and test_gpu_horizons.py's.

Measured maxima of |dU| per set (MI355X; the bounds are tol_u(N) = 1e-9 / 5e-9, 1e-8 after SQP, TOL_CERT = 5e-8):
  set   GPU vs oracle, single QP   GPU vs oracle, 3 SQP   GPU vs golden   oracle vs golden
  A     3.1e-11                    2.2e-09                7.8e-10         7.8e-10
  B     3.2e-12                    1.4e-10                7.6e-10         7.6e-10
  W     2.2e-11                    1.5e-11                4.8e-12         4.8e-12
  U     5.5e-12                    1.6e-10                1.7e-10         1.7e-10
  G     7.2e-12                    6.5e-11                4.1e-10         4.1e-10
  T     5.7e-11                    8.4e-10                4.1e-10         4.1e-10
By horizon the single-QP worst is 1.2e-12 (N = 15), 3.1e-11 (20), 6.9e-12 (25), 4.2e-12 (30), 5.7e-11 (40).  Set U's
C2 batches hold one or two infeasible / numerical status flips each at N = 25, 30, 40, which check_vs_oracle judges
by the elastic objective as at the defaults.  cond(H) at N = 40 reaches 9e9 under B and 1.8e9 under the defaults.
"""
import numpy as np
import pytest

import evaluate_cases as EC
import params_cases as PC
from test_gpu_device_entry import assert_identical
from test_gpu_horizons import ctxs, last_linearisation_point, oracle_solve, solve, sweep_batch  # noqa: F401 (ctxs: fixture)
from test_gpu_parity import TOL_CERT, check_vs_oracle, tol_u

pytestmark = pytest.mark.gpu

SETS = PC.SET_NAMES
BATCH_N = PC.BATCH_N


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import mpcqp
    return mpcqp


@pytest.fixture(scope="module")
def gpu(lib):
    side = PC.Library(lib, 0)
    yield side
    side.close()


@pytest.fixture(scope="module")
def env(lib):
    import trajectory_tracking as TT
    yield dict(mpcqp=lib, TT=TT, device=0)
    EC.close_solvers()


# ---------------------------------------------------------------------------------------------
# 1. golden parity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_warm_start_bit_exact(gpu, name):
    PC.check_warm_start(gpu, name)


@pytest.mark.parametrize("name", SETS)
def test_predict_bit_exact(gpu, name):
    PC.check_predict(gpu, name)


@pytest.mark.parametrize("name", SETS)
def test_qp_solution_vs_certified_golden(gpu, oracles, name):
    PC.check_qp_solution(PC.library_qp(gpu), oracles, name, TOL_CERT, "GPU")


# ---------------------------------------------------------------------------------------------
# 2. evaluator
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_evaluator_equals_host_and_reference(env, name):
    """mpc_evaluate_batch under the set: the device equals the host backend bit for bit on the model records (every
    output), and with it the reference's cost and rows (evaluate_cases.check_reference_pin)."""
    cases, pset = PC.cases(name, "model"), PC.sets()[name]
    host = dict(env, device=-1)
    for (key, _, rg), (_, _, rh) in zip(EC.evaluate_golden(env, cases, name, **pset),
                                        EC.evaluate_golden(host, cases, name, **pset)):
        for k in EC.KEYS:
            assert EC.same(rg[k], rh[k]), (name, key, k)
    EC.check_reference_pin(env, cases, name, **pset)


# ---------------------------------------------------------------------------------------------
# 3. batches against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", BATCH_N)
@pytest.mark.parametrize("wl", ["C2", "C3", "C5"])
@pytest.mark.parametrize("name", SETS)
def test_batch_vs_oracle(lib, ctxs, name, wl, N):
    """The default single-QP launch (the split pair for N <= 31, one kernel at N = 40) on the 203 egos of
    test_gpu_horizons.sweep_batch under the set: GPU == oracle to tol_u(N)."""
    pset = PC.sets()[name]
    wb = sweep_batch(wl, N)
    r = solve(lib, ctxs(wb["traj"]), wb, **pset)
    ro, ctx = oracle_solve(wl, N, pset=PC.frozen(pset))
    check_vs_oracle(r, ro, ctx=ctx, label=f"set {name} {wl} N={N}", tol=tol_u(N))
    assert np.array_equal(r["u0"], r["U"][:, 0, :])
    assert np.isfinite(r["Xpred"]).all()
    PC.assert_paths(name, wl, N, r)


@pytest.mark.parametrize("N", [15, 20, 40])
@pytest.mark.parametrize("name", SETS)
def test_sqp_vs_oracle(lib, ctxs, name, N):
    """sqp_iters = 3 (MODE_FULL), one leg per lane group, on the C3 egos: the bar of
    test_gpu_horizons.test_sqp_horizons_vs_oracle."""
    pset = PC.sets()[name]
    fz = PC.frozen(pset)
    wb = sweep_batch("C3", N)
    r = solve(lib, ctxs(wb["traj"]), wb, sqp_iters=3, **pset)
    ro, ctx = oracle_solve("C3", N, 3, True, fz)
    ctx = ctx + (last_linearisation_point("C3", N, 3, True, fz),)
    s = check_vs_oracle(r, ro, ctx=ctx, label=f"set {name} SQP C3 N={N}", tol=1e-8, xtol=1e-7)
    assert s["elastic_alt_optima"] == 0
    assert (r["iters"] >= 0).all()


# ---------------------------------------------------------------------------------------------
# 4. launch paths give the same bits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [20, 25])
@pytest.mark.parametrize("wl", ["C2", "C3"])
@pytest.mark.parametrize("name", SETS)
def test_split_pair_equals_one_launch(lib, ctxs, name, wl, N):
    """MODE_XO + MODE_IPM == MODE_ONE (MPC_TWO_PHASE=0) under the set, at the specialised horizon 20 and the
    runtime horizon 25."""
    pset = PC.sets()[name]
    wb = sweep_batch(wl, N)
    r2 = solve(lib, ctxs(wb["traj"]), wb, **pset)
    r1 = solve(lib, ctxs(wb["traj"], MPC_TWO_PHASE=0), wb, **pset)
    assert_identical(r2, r1, f"set {name} {wl} N={N}")
    assert (r2["iters"] == 0).any() and (r2["iters"] > 0).any()


# ---------------------------------------------------------------------------------------------
# 5. closed loop
# ---------------------------------------------------------------------------------------------
def test_closed_loop_set_A(env):
    """run_simulation_batch on the device equals the shim's host loop bit for bit under set A (dt = 0.15 in the
    Euler plant and the FSM, the actuation clamp at set A's bounds): N = 10, trajectory 2 with the ObstaclesFSM,
    3 egos, 60 steps, within which the light turns GREEN and the car appears (test_params_cpu.py checks that on the
    host backend)."""
    from test_gpu_closed_loop import compare, host_loop
    TT = env["TT"]
    mpc, traj, mk, x_init = PC.closed_loop_A(TT, device=0)
    r = TT.run_simulation_batch(mpc, mk(), traj, x_init=x_init, max_steps=PC.LOOP_STEPS)
    for b in range(len(x_init)):
        compare(r, b, host_loop(TT, mpc, mk(), traj, x_init[b], PC.LOOP_STEPS))
    PC.assert_loop_switches(r, mpc)


# ---------------------------------------------------------------------------------------------
# 6. the warm start's own knobs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [None, "A"])
def test_warm_start_knobs(gpu, oracles, name):
    """brake_distance = 25, brake_accel = -3.5: the oracle's warm start bit for bit (the reference hard-codes both)."""
    PC.check_knobs(gpu, oracles, name)
