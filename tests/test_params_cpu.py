"""The tracker library away from mpc_default_params, without a GPU: the CPU oracle (oracle/oracle.py) and the
library's host backend (device = -1; csrc/cpu_backend.h, loop_steps.h, evaluate_kernel.h's host instantiation)
against the reference's own records under six parameter sets (tests/golden/params_golden.npz; params_cases.py).

Every other test of the tracker runs at the default weights, dt, control bounds, geometry and brake knobs, where a
literal left in the code, two swapped weights or a u_min / u_max mix-up cannot show.  Here the warm start and the
rollout are bit-equal to the reference under each set, the QP solution is within TOL_CERT of the KKT-certified
optimum of the reference's QP, the evaluator reproduces the reference's cost and rows, and the closed loop of the
host backend runs set A's dt and bounds.  A failure here and none in tests/test_gpu_params.py (or the reverse) tells
which restatement is wrong.

Measured (worst |U - U*_golden| per set, the same figures on the oracle and on the host backend):
  A 7.8e-10, B 7.6e-10, W 4.8e-12, U 1.7e-10, G 4.1e-10, T 4.1e-10   (TOL_CERT = 5e-8)
"""
import numpy as np
import pytest

import evaluate_cases as EC
import params_cases as PC
from test_gpu_parity import TOL_CERT

SETS = PC.SET_NAMES


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import mpcqp
    import trajectory_tracking as TT
    e = dict(mpcqp=mpcqp, TT=TT, device=-1, ptr=lambda a: (a.ctypes.data, a))
    yield e
    EC.close_solvers()


@pytest.fixture(scope="module")
def host(env):
    side = PC.Library(env["mpcqp"], -1)
    yield side
    side.close()


def test_fixture_holds_the_sets():
    """At least three sets; each keeps a positive lane half-width and bounds that bracket 0; every qp record is
    KKT-certified with finite-difference errors of the size the default goldens record (qp_golden: errG 8.9e-7,
    errg 1.5e-7, errc 6.2e-16, errcon 0); the horizons and obstacle kinds of each lane group are there."""
    import json
    import oracle as O
    sets = PC.sets()
    assert tuple(sets) == SETS
    d = O.default_params()
    for name, ps in sets.items():
        p = O.default_params(**ps)
        assert p.lane_width / 2.0 - p.vehicle_radius - p.safe_lane_margin > 0.0
        assert p.u_min[0] < 0 < p.u_max[0] and p.u_min[1] < 0 < p.u_max[1]
        assert any(getattr(p, k) != getattr(d, k) for k in ps if k not in ("u_min", "u_max")) or "u_min" in ps
        qp = PC.cases(name, "qp")
        assert {int(c["N"]) for c in qp} == {10, 15, 20, 25, 30, 40}
        assert {0, 8} <= {int(c["obs"].shape[0]) for c in qp}
        for c in qp:
            assert bool(c["ok_elastic"])
            chk = json.loads(str(c["fdcheck"]))
            # twice the default goldens' worst for the finite-difference Jacobians; the values to rounding
            assert chk["errG"] <= 2e-6 and chk["errg"] <= 3e-7 and chk["errc"] <= 1e-14 and chk["errcon"] == 0.0, chk
        assert len(PC.cases(name, "model")) >= 10 and len(PC.cases(name, "warmstart")) >= 12
    assert sum(len(PC.cases(n, "qp")) for n in SETS) >= 60
    # A and B change every field the reference's tracker has
    for name in ("A", "B"):
        assert len(sets[name]) == 14


# ---------------------------------------------------------------------------------------------
# the oracle against the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_oracle_model_and_warm_start(oracles, name):
    """predict and the warm start bit-equal; cost and constraints at the bar of
    test_oracle_golden.test_model_predict_cost_constraints."""
    from test_oracle_golden import params
    pset = PC.sets()[name]
    for c in PC.cases(name, "model"):
        orc, p = oracles[int(c["traj"])], params(c["N"], 0, pset)
        assert np.array_equal(orc.predict(p, c["x0"], c["U"]), c["X"])
        cost = orc.cost(p, c["x0"], c["U"])
        assert abs(cost - float(c["cost"])) <= 1e-12 * (1 + abs(float(c["cost"])))
        g = orc.constraints(p, c["x0"], c["obs"], c["U"])
        assert g.shape == c["cons"].shape and np.abs(g - c["cons"]).max() <= 1e-12
    for c in PC.cases(name, "warmstart"):
        ub = oracles[int(c["traj"])].warm_start(params(c["N"], 0, pset), c["x0"], c["obs"])
        assert np.array_equal(ub, c["ubar"]), (c["x0"], c["obs"])


@pytest.mark.parametrize("name", SETS)
def test_oracle_qp_solution_vs_certified_golden(oracles, name):
    PC.check_qp_solution(PC.oracle_qp(oracles), oracles, name, TOL_CERT, "oracle")


# ---------------------------------------------------------------------------------------------
# the host backend against the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_host_warm_start_bit_exact(host, name):
    PC.check_warm_start(host, name)


@pytest.mark.parametrize("name", SETS)
def test_host_predict_bit_exact(host, name):
    PC.check_predict(host, name)


@pytest.mark.parametrize("name", SETS)
def test_host_qp_solution_vs_certified_golden(host, oracles, name):
    PC.check_qp_solution(PC.library_qp(host), oracles, name, TOL_CERT, "host backend")


@pytest.mark.parametrize("name", SETS)
def test_host_evaluator_reference_pin(env, name):
    """mpc_evaluate_batch on the host backend: the reference's cost and constraint rows under the set, by the rule of
    evaluate_cases.check_reference_pin (bit-equal)."""
    EC.check_reference_pin(env, PC.cases(name, "model"), name, **PC.sets()[name])


@pytest.mark.parametrize("name", [None, "A"])
def test_host_warm_start_knobs(host, oracles, name):
    """brake_distance = 25, brake_accel = -3.5 (the reference hard-codes 40 and -2.0): the oracle's warm start bit for
    bit, under the defaults and under set A's dt."""
    PC.check_knobs(host, oracles, name)


@pytest.mark.parametrize("N", PC.BATCH_N)
@pytest.mark.parametrize("wl", ["C2", "C3", "C5"])
@pytest.mark.parametrize("name", SETS)
def test_host_batch_equals_oracle(env, name, wl, N):
    """The batches of tests/test_gpu_params.py on the host backend, at the bar of
    test_cpu_backend.test_backend_equals_oracle; it also checks, without a GPU, that under every set the batches hold
    the crossover-certified, deferred and elastic instances the GPU test asks for."""
    import test_gpu_horizons as H
    from test_cpu_backend import _assert_equals_oracle
    mpcqp, pset = env["mpcqp"], PC.sets()[name]
    wb = H.sweep_batch(wl, N)
    slv = EC.solver(env, wb["traj"], N, wb["max_obs"], **pset)
    r = slv.solve_batch(wb["x0"], wb["obs"], wb["n_obs"])
    ro, _ = H.oracle_solve(wl, N, pset=PC.frozen(pset))
    _assert_equals_oracle(r, ro, f"set {name} {wl} N={N}")
    PC.assert_paths(name, wl, N, r)


# ---------------------------------------------------------------------------------------------
# closed loop under set A
# ---------------------------------------------------------------------------------------------
def test_host_closed_loop_set_A(env):
    """The closed loop of tests/test_gpu_params.py on the host backend: mpc_closed_loop (loop_steps.h: FSM, Euler
    plant, actuation) equals the shim's loop over the same backend bit for bit at set A's dt and bounds, and both
    state machines switch within the 60 steps the GPU test relies on."""
    from test_gpu_closed_loop import compare, host_loop
    TT = env["TT"]
    mpc, traj, mk, x_init = PC.closed_loop_A(TT, device=-1)
    r = TT.run_simulation_batch(mpc, mk(), traj, x_init=x_init, max_steps=PC.LOOP_STEPS)
    for b in range(len(x_init)):
        compare(r, b, host_loop(TT, mpc, mk(), traj, x_init[b], PC.LOOP_STEPS))
    PC.assert_loop_switches(r, mpc)
