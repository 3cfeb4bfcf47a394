"""GPU tests of mpc_gradient_batch / mpc_gradient_batch_device (csrc/gradient_kernel.h): the restatement pin and the
cost bits of tests/test_gradient_cpu.py on the device (gradient_cases.py); GPU == host bit for bit on the golden
cases and at every lane-group boundary horizon with spare lane groups in the wavefront; the summary cases, the
independence and the contract; the device entry captured into a HIP graph, and beside a solve on another stream of
the same context."""
import numpy as np
import pytest

import gradient_cases as GC
import gradient_params_cases as GP

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


def test_restatement_pin(env):
    GC.check_restatement_pin(env)


def test_cost_bits(env):
    GC.check_cost_bits(env)


def test_golden_gpu_equals_host(env):
    host = dict(env, device=-1)
    for (key, _, _, rg, _), (_, _, _, rh, _) in zip(GC.gradient_golden(env), GC.gradient_golden(host)):
        for k in GC.OUT_KEYS:
            assert GC.same(rg[k], rh[k]), (key, k)


@pytest.mark.parametrize("mo", GC.SHAPE_MO)
@pytest.mark.parametrize("N", GC.SHAPE_N)
def test_gpu_equals_host_bit_for_bit(env, N, mo):
    """N = 1 is the first stage alone; 15 | 16 and 31 | 32 are the two sides of the GL = 16 / 32 / 64 switches, 63
    the limit; B = 5 leaves spare lane groups in the last wavefront for every GL; n_obs mixed over {0, 1, 3} and
    NULL; with and without lam; instance 3 rolls past s_max."""
    gpu, host = GC.solver(env, 1, N, mo), GC.solver(env, 1, N, mo, device=-1)
    for what, w in GC.shape_runs(N, mo):
        rg, rh = GC.gradient(gpu, w), GC.gradient(host, w)
        assert sorted(rg) == sorted(rh)
        for k in rg:
            assert GC.same(rg[k], rh[k]), (N, mo, what, k)


def test_summary_cases(env):
    GC.check_summary_cases(env)


def test_independence(env):
    GC.check_independence(env)


def test_contract(env):
    GC.check_contract(env)
    env["sync"]()


def _buffers(env, slv, w):
    torch = env["torch"]
    dev = torch.device("cuda", 0)
    B, N = w["x0"].shape[0], slv.params.N
    t = lambda a: None if a is None else torch.as_tensor(a, device=dev).contiguous()
    e = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=dev)
    return dict(x0=t(w["x0"]), U=t(w["U"]), obs=t(w["obs"]), n_obs=t(w["n_obs"]), lam=t(w["lam"]), grad=e(B, N, 2),
                jtl=e(B, N, 2), gx0=e(B, 5), costate=e(B, N, 5), summary=e(B, 6))


def _device_call(slv, bufs, stream):
    p = lambda t: None if t is None else t.data_ptr()
    slv.gradient_batch_device(bufs["x0"].shape[0], p(bufs["x0"]), p(bufs["obs"]), p(bufs["n_obs"]), p(bufs["U"]),
                              p(bufs["lam"]), *(p(bufs[k]) for k in GC.OUT_KEYS), stream=stream)


def test_device_entry_in_a_graph(env):
    """mpc_gradient_batch_device captured once into a HIP graph and replayed twice with changed inputs equals the
    eager call and the host-buffer entry."""
    torch = env["torch"]
    N, mo, B = 20, 3, 67
    slv = GC.solver(env, 2, N, mo)
    wa, wb, wc = (GC.lam_batch(GC.EC.random_batch(2, N, B, mo, seed=s), mo, s + 100) for s in (91, 92, 93))
    want = [GC.gradient(slv, w) for w in (wa, wb, wc)]
    bufs = _buffers(env, slv, wa)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    _device_call(slv, bufs, side.cuda_stream)
    side.synchronize()
    for k in GC.OUT_KEYS:
        assert GC.same(bufs[k].cpu().numpy(), want[0][k]), k
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        _device_call(slv, bufs, torch.cuda.current_stream().cuda_stream)
    for w, ref in ((wb, want[1]), (wc, want[2])):
        for k in ("x0", "U", "obs", "n_obs", "lam"):
            bufs[k].copy_(torch.as_tensor(w[k]))
        for k in GC.OUT_KEYS:
            bufs[k].fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        for k in GC.OUT_KEYS:
            assert GC.same(bufs[k].cpu().numpy(), ref[k]), k


def test_gradient_beside_a_solve_on_another_stream(env):
    """A gradient call on one stream while a solve of the same context runs on another: both equal their serial
    values (the gradient shares no state with the solver)."""
    torch = env["torch"]
    dev = torch.device("cuda", 0)
    N, mo, B = 20, 3, 256
    slv = GC.solver(env, 2, N, mo)
    w = GC.lam_batch(GC.EC.random_batch(2, N, B, mo, seed=95), mo, 96)
    w["obs"][:, :, 0] = w["x0"][:, :1] + np.array([25.0, 60.0, 90.0])
    serial_solve = slv.solve_batch(w["x0"], w["obs"], w["n_obs"])
    serial_grad = GC.gradient(slv, w)
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
    _device_call(slv, bufs, sb.cuda_stream)
    torch.cuda.synchronize()
    for k in GC.OUT_KEYS:
        assert GC.same(bufs[k].cpu().numpy(), serial_grad[k]), k
    for k in ("u0", "U", "Xpred", "status", "iters"):
        assert np.array_equal(out[k].cpu().numpy(), serial_solve[k]), k


# ---------------------------------------------------------------------------------------------
# away from the goldens (gradient_params_cases.py)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GP.PC.SET_NAMES)
def test_params_restatement_pin(env, name):
    GP.check_set_pin(env, name)


@pytest.mark.parametrize("name", GP.SUMMARY_SETS)
def test_params_summary_against_numpy(env, name):
    GP.check_set_summary(env, name)


@pytest.mark.parametrize("name", GP.FD_SETS)
def test_params_finite_differences(env, name):
    GP.check_set_finite_differences(env, name)


@pytest.mark.parametrize("case", GP.shape_cases(), ids=GP.case_id)
def test_shape_pin(env, case):
    """Each lane group with two full wavefronts and one more instance, mixed n_obs, the 64-row slab and both OBS
    instantiations against the longdouble yardstick; the host backend agrees with the device bit for bit."""
    GP.check_shape_inputs(case)
    GP.check_shape(env, case)


@pytest.mark.parametrize("case", GP.STATIONARITY_CASES, ids=GP.stationarity_id)
def test_stationarity(env, case):
    GP.check_stationarity(env, case)


def test_single_qp_is_not_stationary_printed(env):
    GP.print_single_qp(env, GP.STATIONARITY_CASES[4])
