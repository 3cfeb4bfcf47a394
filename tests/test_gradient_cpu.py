"""mpc_gradient_batch on the host backend (device = -1): the gradient of the reference's cost in U and x0 and J' lam of
its constraint rows, pinned to an independent forward-mode restatement run in np.longdouble, to central differences
through mpc_evaluate_batch, its summary to numpy on the returned arrays; independence of the batch; the argument
contract.  The test bodies are shared with tests/test_gpu_gradient.py (gradient_cases.py)."""
import numpy as np
import pytest

import gradient_cases as GC
import gradient_params_cases as GP


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import mpcqp
    yield dict(mpcqp=mpcqp, device=-1, ptr=lambda a: (a.ctypes.data, a))
    GC.close_solvers()


def test_symbols_and_fields(env):
    mpcqp = env["mpcqp"]
    L = mpcqp.lib()
    assert L.mpc_version() == 5
    assert hasattr(L, "mpc_gradient_batch") and hasattr(L, "mpc_gradient_batch_device")
    assert len(mpcqp.GRQ_FIELDS) == mpcqp.GR_NQ == 6


def test_restatement_error_budget():
    """The float64 run of the restatement against its longdouble run stays within the worst that the bound was
    derived from (gradient_cases.py's header); the restatement's cost and rows are the reference's recorded ones."""
    assert np.finfo(np.longdouble).eps < 1e-18
    worst = GC.measure_restatement_error()
    print(f"restatement float64 vs longdouble: worst {worst:.3e}")
    assert worst <= GC.RESTATE_F64_WORST
    import evaluate_cases as EC
    for key, cs in EC.golden_groups().items():
        for b, c in enumerate(cs):
            ref = GC.yardstick()[(key, b)]
            assert abs(float(ref["cost"]) - float(c["cost"])) <= 1e-12 * (1 + abs(float(c["cost"])))
            got = EC.reference_vector(ref["rows"].astype(np.float64), key[2])
            assert np.abs(got - c["cons"]).max() <= 1e-12 * (1 + np.abs(c["cons"]).max())


def test_restatement_pin(env):
    GC.check_restatement_pin(env)


def test_finite_differences_through_the_evaluator(env):
    GC.check_finite_differences(env)


def test_cost_bits(env):
    GC.check_cost_bits(env)


def test_golden_summary_against_numpy(env):
    GC.check_golden_summary(env)


def test_summary_cases(env):
    GC.check_summary_cases(env)


def test_independence(env):
    GC.check_independence(env)


def test_contract(env):
    GC.check_contract(env)


@pytest.mark.parametrize("mo", GC.SHAPE_MO)
@pytest.mark.parametrize("N", GC.SHAPE_N)
def test_shapes_summary(env, N, mo):
    """The shapes of the GPU == host test on the host alone: the summary against numpy."""
    slv = GC.solver(env, 1, N, mo)
    for what, w in GC.shape_runs(N, mo):
        GC.check_summary(slv, w, GC.gradient(slv, w), (N, mo, what))


# ---------------------------------------------------------------------------------------------
# away from the goldens (gradient_params_cases.py)
# ---------------------------------------------------------------------------------------------
def test_params_restatement_is_the_reference():
    """Before the restatement judges the library under a parameter set, its longdouble run under model_of(mpc_params)
    reproduces the reference's recorded cost and rows on the 72 records; its float64 run stays within the error the
    bound was derived from."""
    import oracle as O
    assert GP.model_of(O.default_params()) == GC.default_model()
    worst = {name: GP.check_yardstick_is_the_reference(name) for name in GP.PC.SET_NAMES}
    print("restatement float64 vs longdouble per set:", {k: f"{v:.3e}" for k, v in worst.items()})
    assert max(worst.values()) <= GP.PARAMS_F64_WORST


@pytest.mark.parametrize("name", GP.PC.SET_NAMES)
def test_params_restatement_pin(env, name):
    GP.check_set_pin(env, name)


@pytest.mark.parametrize("name", GP.SUMMARY_SETS)
def test_params_summary_against_numpy(env, name):
    GP.check_set_summary(env, name)


@pytest.mark.parametrize("name", GP.FD_SETS)
def test_params_finite_differences(env, name):
    GP.check_set_finite_differences(env, name)


def test_shape_yardstick_budget():
    """Every generated batch holds what it is there for, and the float64 restatement stays within the recorded error
    per horizon."""
    for case in GP.shape_cases():
        GP.check_shape_inputs(case)
    assert {c[1] for c in GP.shape_cases()} == set(GP.SHAPE_N) == set(GP.SHAPE_F64_WORST)
    for N in GP.SHAPE_N:
        worst = GP.measure_shape_error(N)
        print(f"restatement float64 vs longdouble, N = {N}: worst {worst:.3e}")
        assert worst <= GP.SHAPE_F64_WORST[N], N


@pytest.mark.parametrize("case", GP.shape_cases(), ids=GP.case_id)
def test_shape_pin(env, case):
    GP.check_shape_inputs(case)
    GP.check_shape(env, case)


def test_stationarity_oracle_figures(env):
    """The oracle's SQP through the measure: the figures the stationarity bounds were taken from, re-measured."""
    worst = {}
    for case in GP.STATIONARITY_CASES:
        t = GP.measure_stationarity(env, case, GP.oracle_answer(case))
        GP.check_stationarity_population(case, t)
        f = GP.worst_figures(t)
        print(f"oracle {GP.stationarity_id(case)}: " + ", ".join(f"{n} {g:.3e}" for n, g in zip(GP.FIGURES, f)))
        worst[case[2]] = tuple(max(a, b) for a, b in zip(worst.get(case[2], f), f))
    for name, f in worst.items():
        assert all(a <= b for a, b in zip(f, GP.STATIONARITY_ORACLE[name])), (name, f)
        assert all(b <= 1.01 * a for a, b in zip(f, GP.STATIONARITY_ORACLE[name])), (name, f)


@pytest.mark.parametrize("case", GP.STATIONARITY_CASES, ids=GP.stationarity_id)
def test_stationarity(env, case):
    GP.check_stationarity(env, case)


def test_single_qp_is_not_stationary_printed(env):
    GP.print_single_qp(env, GP.STATIONARITY_CASES[4])
