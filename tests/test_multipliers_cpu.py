"""mpc_multipliers_batch on the host backend (device = -1): the least-squares multiplier estimates of the reference's
constraint rows, pinned to a longdouble restatement of the header's definition with steered active lists, to the
tool's numpy estimator on the oracle's SQP answers, end to end through certify_batch; independence of the batch; the
consistency with the evaluator and the gradient entry; the argument contract.  The test bodies are shared with
tests/test_gpu_multipliers.py (multiplier_cases.py).

Measured on the host backend (the figures DESIGN.md section 5f quotes): see the printed lines of test_yardstick_pin."""
import numpy as np
import pytest

import gradient_cases as GC
import gradient_params_cases as GP
import multiplier_cases as MC


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
    assert hasattr(L, "mpc_multipliers_batch") and hasattr(L, "mpc_multipliers_batch_device")
    assert len(mpcqp.MUQ_FIELDS) == mpcqp.MU_NQ == 6 and mpcqp.MAX_ACTIVE == 64
    assert (mpcqp.MU_OK, mpcqp.MU_OVERFLOW, mpcqp.MU_NO_FREE, mpcqp.MU_NONFINITE) == (0, 1, 2, 3)


def test_yardstick_restates_the_gradient_yardstick(env):
    """restate_jac() against gradient_cases.restate() in longdouble on the golden cases: the same grad and rows, and
    its Jacobian applied to the seeded lam is restate()'s jtl.  A self-check of the reference: it runs no library code
    beyond asking for the symbol the yardstick is there for."""
    assert hasattr(env["mpcqp"].lib(), "mpc_multipliers_batch")
    n = 0
    for key, cs in sorted(MC.EC.golden_groups().items()):
        w = GC.group_inputs(key, cs)
        for b in range(0, len(cs), 2):
            obs = np.zeros((0, 2)) if w["obs"] is None else w["obs"][b]
            ref = GC.yardstick()[(key, b)]
            R = MC.restate_jac(key[0], w["x0"][b], w["U"][b], obs, np.longdouble)
            assert np.array_equal(R["grad"], ref["grad"].reshape(-1)) and np.array_equal(R["rows"], ref["rows"])
            jtl = np.einsum("kc,kci->i", w["lam"][b].astype(np.longdouble), R["jac"])
            assert GC.rel_err(jtl, ref["jtl"].reshape(-1)) <= 1e-17
            n += 1
    assert n >= 30


@pytest.mark.parametrize("group", MC.pin_groups(), ids=lambda g: g[0])
def test_yardstick_pin(env, group):
    """The entry against the longdouble yardstick with the active list steered to m = 0, 1, 5, 2N - 1, 2N, 64, 65.
    Measured (host backend; the device gives the same bits): 633 of 666 runs compared in 25 batches, the yardstick's
    float64 error at worst 1.50e-6 in a batch, the library's 3.25e-6 (bound of that batch 1.51e-5); every compared run
    agrees in status, counts, list and kept set.  33 runs lie in the threshold band and are checked in what the drop
    decision does not touch; per batch at most one run in ten does, but for golden (3, 20, 2) with 6 of 42 and golden
    (3, 30, 1) with 7 of 42, the named exceptions of multiplier_cases.BAND_EXCEPTIONS."""
    MC.check_pin(env, [group])


@pytest.mark.parametrize("case", [GP.STATIONARITY_CASES[0], GP.STATIONARITY_CASES[4]], ids=GP.stationarity_id)
def test_against_the_tools_estimator(env, case):
    MC.check_against_estimator(env, case)


@pytest.mark.parametrize("case", [GP.STATIONARITY_CASES[0], GP.STATIONARITY_CASES[4]], ids=GP.stationarity_id)
def test_certify_end_to_end(env, case):
    MC.check_certify(env, case)


def test_tracker_certify_batch(env):
    MC.check_tracker_certify(env)


def test_shape_batches_cover_every_kind_of_list(env):
    """The batches and tolerances of the GPU == host test (tests/test_gpu_multipliers.py) reach empty lists, lists kept
    whole, lists with dropped rows and overflowing lists; every horizon but N = 1 reaches all four."""
    seen = set()
    for N in MC.SHAPE_N:
        for mo in MC.SHAPE_MO:
            host, w, k = MC.solver(env, 1, N, mo), MC.shape_batch(N, mo), set()
            for tol in MC.shape_tols(host, w):
                k |= MC.shape_kinds(MC.multipliers(host, w, active_tol=tol)["summary"])
            assert k >= ({"empty", "dropped"} if N == 1 else {"empty", "full", "dropped", "overflow"}), (N, mo, k)
            seen |= k
    assert seen == {"empty", "full", "dropped", "overflow"}, seen


def test_independence(env):
    MC.check_independence(env)


def test_consistency_with_the_siblings(env):
    MC.check_siblings(env)


def test_contract(env):
    MC.check_contract(env)
