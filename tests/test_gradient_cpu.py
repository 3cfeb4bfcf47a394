"""mpc_gradient_batch on the host backend (device = -1): the gradient of the reference's cost in U and x0 and J' lam of
its constraint rows, pinned to an independent forward-mode restatement run in np.longdouble, to central differences
through mpc_evaluate_batch, its summary to numpy on the returned arrays; independence of the batch; the argument
contract.  The test bodies are shared with tests/test_gpu_gradient.py (gradient_cases.py)."""
import numpy as np
import pytest

import gradient_cases as GC


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
