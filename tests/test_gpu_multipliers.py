"""GPU tests of mpc_multipliers_batch / mpc_multipliers_batch_device (csrc/multiplier_kernel.h): the yardstick pin,
the tool's estimator, certify_batch, the independence, the sibling consistency and the contract of
tests/test_multipliers_cpu.py on the device (multiplier_cases.py); GPU == host bit for bit at every lane-group
boundary horizon with short, long and overflowing lists; the device entry captured into a HIP graph, and beside a
solve on another stream of the same context."""
import numpy as np
import pytest

import gradient_cases as GC
import gradient_params_cases as GP
import multiplier_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    torch = pytest.importorskip("torch")
    import mpcqp
    dev = torch.device("cuda", 0)

    def ptr(a):
        t = torch.as_tensor(np.ascontiguousarray(a), device=dev)
        torch.cuda.synchronize()
        return t.data_ptr(), t

    yield dict(mpcqp=mpcqp, device=0, ptr=ptr, torch=torch, sync=torch.cuda.synchronize)
    torch.cuda.synchronize()
    GC.close_solvers()


@pytest.mark.parametrize("group", MC.pin_groups(), ids=lambda g: g[0])
def test_yardstick_pin(env, group):
    """The device gives the host backend's figures (tests/test_multipliers_cpu.py::test_yardstick_pin states them)."""
    MC.check_pin(env, [group])


@pytest.mark.parametrize("mo", MC.SHAPE_MO)
@pytest.mark.parametrize("N", MC.SHAPE_N)
def test_gpu_equals_host_bit_for_bit(env, N, mo):
    """N = 1 is the first stage alone; 15 | 16 and 31 | 32 are the two sides of the LDS classes, 63 the limit; n_obs
    mixed over {0, 1, 3}; instance 3 rolls past s_max; the lists run from empty over rank-deficient to overflowing."""
    gpu, host = MC.solver(env, 1, N, mo), MC.solver(env, 1, N, mo, device=-1)
    w = MC.shape_batch(N, mo)
    seen = set()
    for tol in MC.shape_tols(host, w):
        rg, rh = MC.multipliers(gpu, w, active_tol=tol), MC.multipliers(host, w, active_tol=tol)
        for k in MC.OUT_KEYS:
            assert MC.same(rg[k], rh[k]), (N, mo, tol, k)
        seen |= MC.shape_kinds(rh["summary"])
    # what every horizon must have compared; N = 1 has at most ten rows, so it cannot overflow
    assert seen >= ({"empty", "dropped"} if N == 1 else {"empty", "full", "dropped", "overflow"}), (N, mo, seen)


def test_bit_identity_covered_every_kind_of_list(env):
    """Over the parametrisation above, on the host backend (the same tolerances): empty lists, lists kept whole, lists
    with dropped rows and overflowing lists were each compared."""
    seen = set()
    for N in MC.SHAPE_N:
        for mo in MC.SHAPE_MO:
            host, w = MC.solver(env, 1, N, mo, device=-1), MC.shape_batch(N, mo)
            for tol in MC.shape_tols(host, w):
                seen |= MC.shape_kinds(MC.multipliers(host, w, active_tol=tol)["summary"])
    assert seen == {"empty", "full", "dropped", "overflow"}, seen


@pytest.mark.parametrize("case", [GP.STATIONARITY_CASES[0], GP.STATIONARITY_CASES[4]], ids=GP.stationarity_id)
def test_against_the_tools_estimator(env, case):
    MC.check_against_estimator(env, case)


@pytest.mark.parametrize("case", [GP.STATIONARITY_CASES[0], GP.STATIONARITY_CASES[4]], ids=GP.stationarity_id)
def test_certify_end_to_end(env, case):
    MC.check_certify(env, case)


def test_tracker_certify_batch(env):
    MC.check_tracker_certify(env)


def test_independence(env):
    MC.check_independence(env)


def test_consistency_with_the_siblings(env):
    MC.check_siblings(env)


def test_contract(env):
    MC.check_contract(env)
    env["sync"]()


def _batch(N, mo, B, seed):
    w = MC.EC.random_batch(2, N, B, mo, seed=seed)
    w["U"][::2] = np.clip(w["U"][::2], np.array(MC.U_MIN) * 0.9, np.array(MC.U_MAX) * 0.9)
    return w


def _buffers(env, slv, w):
    torch = env["torch"]
    dev = torch.device("cuda", 0)
    B, N, mo = w["x0"].shape[0], slv.params.N, slv.params.max_obs
    t = lambda a: None if a is None else torch.as_tensor(a, device=dev).contiguous()
    return dict(x0=t(w["x0"]), U=t(w["U"]), obs=t(w["obs"]), n_obs=t(w["n_obs"]),
                lam=torch.full((B, N, 7 + mo), -7.0, dtype=torch.float64, device=dev),
                active=torch.full((B, 64), -7, dtype=torch.int32, device=dev),
                summary=torch.full((B, 6), -7.0, dtype=torch.float64, device=dev))


def _device_call(slv, bufs, stream, tol):
    p = lambda t: None if t is None else t.data_ptr()
    slv.multipliers_batch_device(bufs["x0"].shape[0], p(bufs["x0"]), p(bufs["obs"]), p(bufs["n_obs"]), p(bufs["U"]),
                                 *(p(bufs[k]) for k in MC.OUT_KEYS), active_tol=tol, stream=stream)


def test_device_entry_in_a_graph(env):
    """mpc_multipliers_batch_device captured once into a HIP graph and replayed twice with changed inputs equals the
    eager call and the host-buffer entry."""
    torch = env["torch"]
    N, mo, B = 20, 3, 67
    slv = MC.solver(env, 2, N, mo)
    wa, wb, wc = (_batch(N, mo, B, s) for s in (191, 192, 193))
    tol = MC.shape_tols(slv, wa)[1]
    want = [MC.multipliers(slv, w, active_tol=tol) for w in (wa, wb, wc)]
    assert all((r["lam"] != 0).any() for r in want)
    bufs = _buffers(env, slv, wa)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    _device_call(slv, bufs, side.cuda_stream, tol)
    side.synchronize()
    for k in MC.OUT_KEYS:
        assert MC.same(bufs[k].cpu().numpy(), want[0][k]), k
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        _device_call(slv, bufs, torch.cuda.current_stream().cuda_stream, tol)
    for w, ref in ((wb, want[1]), (wc, want[2])):
        for k in ("x0", "U", "obs", "n_obs"):
            bufs[k].copy_(torch.as_tensor(w[k]))
        for k in MC.OUT_KEYS:
            bufs[k].fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for k in MC.OUT_KEYS:
            assert MC.same(bufs[k].cpu().numpy(), ref[k]), k


def test_multipliers_beside_a_solve_on_another_stream(env):
    """A multiplier call on one stream while a solve of the same context runs on another: both equal their serial
    values (the estimate shares no state with the solver)."""
    torch = env["torch"]
    dev = torch.device("cuda", 0)
    N, mo, B = 20, 3, 256
    slv = MC.solver(env, 2, N, mo)
    w = _batch(N, mo, B, 195)
    w["obs"][:, :, 0] = w["x0"][:, :1] + np.array([25.0, 60.0, 90.0])
    tol = MC.shape_tols(slv, w)[1]
    serial_solve = slv.solve_batch(w["x0"], w["obs"], w["n_obs"])
    serial = MC.multipliers(slv, w, active_tol=tol)
    bufs = _buffers(env, slv, w)
    out = dict(u0=torch.empty((B, 2), dtype=torch.float64, device=dev),
               U=torch.empty((B, N, 2), dtype=torch.float64, device=dev),
               Xpred=torch.empty((B, N + 1, 5), dtype=torch.float64, device=dev),
               status=torch.empty(B, dtype=torch.int32, device=dev), iters=torch.empty(B, dtype=torch.int32, device=dev))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    sa.wait_stream(torch.cuda.current_stream())
    sb.wait_stream(torch.cuda.current_stream())
    slv.solve_batch_device(B, bufs["x0"].data_ptr(), bufs["obs"].data_ptr(), bufs["n_obs"].data_ptr(), 0,
                           out["u0"].data_ptr(), out["U"].data_ptr(), out["Xpred"].data_ptr(),
                           out["status"].data_ptr(), out["iters"].data_ptr(), stream=sa.cuda_stream)
    _device_call(slv, bufs, sb.cuda_stream, tol)
    torch.cuda.synchronize()
    for k in MC.OUT_KEYS:
        assert MC.same(bufs[k].cpu().numpy(), serial[k]), k
    for k in ("u0", "U", "Xpred", "status", "iters"):
        assert np.array_equal(out[k].cpu().numpy(), serial_solve[k]), k
