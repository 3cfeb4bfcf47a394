"""GPU tests of mpc_hessvec_batch / mpc_hessvec_batch_device (csrc/hessvec_kernel.h): the restatement pin, the finite
differences, the structure, the summary cases, the independence and the contract of tests/test_hessvec_cpu.py on the
device (hessvec_cases.py); GPU == host bit for bit on the golden cases and at every horizon of the shape list with
M = 1, the dense call, an M that straddles a pass boundary and M = 128; the device entry captured into a HIP graph, and
beside a solve on another stream of the same context."""
import numpy as np
import pytest

import hessvec_cases as HC

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
    HC.close_solvers()


def test_restatement_pin(env):
    HC.check_restatement_pin(env)


def test_finite_differences_of_the_gradient(env):
    HC.check_finite_differences(env)


def test_structure(env):
    HC.check_structure(env)


def test_golden_gpu_equals_host(env):
    host = dict(env, device=-1)
    for (key, _, _, dg, rg), (_, _, _, dh, rh) in zip(HC.hessvec_golden(env), HC.hessvec_golden(host)):
        for mode in HC.MODES:
            for k in HC.OUT_KEYS:
                assert HC.same(dg[mode][k], dh[mode][k]) and HC.same(rg[mode][k], rh[mode][k]), (key, mode, k)


@pytest.mark.parametrize("mo", HC.SHAPE_MO)
@pytest.mark.parametrize("N", HC.SHAPE_N)
def test_gpu_equals_host_bit_for_bit(env, N, mo):
    """N = 1 is the first stage alone; 15 | 16 and 31 | 32 are the gradient phase's lane-group boundaries, 63 the limit
    and the 32-direction pass; B = 5 is a partial grid; M = 1, the dense call, one M across a pass boundary (65 or 33)
    and 128; n_obs mixed over {0, 1, 3} and NULL; both modes, with and without lam; instance 3 rolls past s_max."""
    gpu, host = HC.solver(env, 1, N, mo), HC.solver(env, 1, N, mo, device=-1)
    for what, w, V, M, mode in HC.shape_runs(N, mo):
        rg, rh = HC.hessvec(gpu, w, V, M, mode), HC.hessvec(host, w, V, M, mode)
        assert sorted(rg) == sorted(rh)
        for k in rg:
            assert HC.same(rg[k], rh[k]), (N, mo, what, k)


@pytest.mark.parametrize("N", (56, 57))
def test_pass_width_boundary(env, N):
    """N = 56 is the longest horizon of the 64-direction pass (the kernel's largest LDS, 161,168 B), 57 the first of
    the 32-direction pass: GPU == host bit for bit on the same runs."""
    gpu, host = HC.solver(env, 1, N, 3), HC.solver(env, 1, N, 3, device=-1)
    for what, w, V, M, mode in HC.shape_runs(N, 3):
        rg, rh = HC.hessvec(gpu, w, V, M, mode), HC.hessvec(host, w, V, M, mode)
        for k in rg:
            assert HC.same(rg[k], rh[k]), (N, what, k)


def test_summary_cases(env):
    HC.check_summary_cases(env)


@pytest.mark.parametrize("N", (20, 63))
def test_independence(env, N):
    HC.check_independence(env, N)


def test_contract(env):
    HC.check_contract(env)
    env["sync"]()


def _buffers(env, slv, w, V):
    torch = env["torch"]
    dev = torch.device("cuda", 0)
    B, N, M, rw = w["x0"].shape[0], slv.params.N, V.shape[1], 7 + slv.params.max_obs
    t = lambda a: None if a is None else torch.as_tensor(a, device=dev).contiguous()
    e = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=dev)
    return dict(x0=t(w["x0"]), U=t(w["U"]), obs=t(w["obs"]), n_obs=t(w["n_obs"]), lam=t(w["lam"]), V=t(V),
                HV=e(B, M, N, 2), JV=e(B, M, N, rw), curv=e(B, M, 2), summary=e(B, 5))


def _device_call(slv, bufs, stream, mode="exact"):
    p = lambda t: None if t is None else t.data_ptr()
    slv.hessvec_batch_device(bufs["x0"].shape[0], p(bufs["x0"]), p(bufs["obs"]), p(bufs["n_obs"]), p(bufs["U"]),
                             p(bufs["lam"]), bufs["V"].shape[1], p(bufs["V"]), mode,
                             *(p(bufs[k]) for k in HC.OUT_KEYS), stream=stream)


def _batch(N, B, mo, M, seed):
    w = HC.GC.lam_batch(HC.EC.random_batch(2, N, B, mo, seed=seed), mo, seed + 100)
    return w, np.random.default_rng(seed + 200).normal(size=(B, M, N, 2))


def test_device_entry_in_a_graph(env):
    """mpc_hessvec_batch_device captured once into a HIP graph and replayed twice with changed inputs equals the eager
    call and the host-buffer entry."""
    torch = env["torch"]
    N, mo, B, M = 20, 3, 37, 65
    slv = HC.solver(env, 2, N, mo)
    (wa, Va), (wb, Vb), (wc, Vc) = (_batch(N, B, mo, M, s) for s in (191, 192, 193))
    want = [HC.hessvec(slv, w, V) for w, V in ((wa, Va), (wb, Vb), (wc, Vc))]
    bufs = _buffers(env, slv, wa, Va)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    _device_call(slv, bufs, side.cuda_stream)
    side.synchronize()
    for k in HC.OUT_KEYS:
        assert HC.same(bufs[k].cpu().numpy(), want[0][k]), k
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        _device_call(slv, bufs, torch.cuda.current_stream().cuda_stream)
    for (w, V), ref in (((wb, Vb), want[1]), ((wc, Vc), want[2])):
        for k in ("x0", "U", "obs", "n_obs", "lam"):
            bufs[k].copy_(torch.as_tensor(w[k]))
        bufs["V"].copy_(torch.as_tensor(V))
        for k in HC.OUT_KEYS:
            bufs[k].fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        for k in HC.OUT_KEYS:
            assert HC.same(bufs[k].cpu().numpy(), ref[k]), k


def test_hessvec_beside_a_solve_on_another_stream(env):
    """A hessvec call on one stream while a solve of the same context runs on another: both equal their serial values
    (the call shares no state with the solver)."""
    torch = env["torch"]
    dev = torch.device("cuda", 0)
    N, mo, B, M = 20, 3, 256, 40
    slv = HC.solver(env, 2, N, mo)
    w, V = _batch(N, B, mo, M, 195)
    w["obs"][:, :, 0] = w["x0"][:, :1] + np.array([25.0, 60.0, 90.0])
    serial_solve = slv.solve_batch(w["x0"], w["obs"], w["n_obs"])
    serial = HC.hessvec(slv, w, V)
    bufs = _buffers(env, slv, w, V)
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
    for k in HC.OUT_KEYS:
        assert HC.same(bufs[k].cpu().numpy(), serial[k]), k
    for k in ("u0", "U", "Xpred", "status", "iters"):
        assert np.array_equal(out[k].cpu().numpy(), serial_solve[k]), k
