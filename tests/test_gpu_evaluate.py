"""GPU tests of mpc_evaluate_batch / mpc_evaluate_batch_device (csrc/evaluate_kernel.h): the reference pin, the
summary against numpy and the solver consistency of tests/test_evaluate_cpu.py on the device (evaluate_cases.py);
GPU == host bit for bit at every lane-group boundary horizon, with partial tail groups, every slab width and NaN
instances among healthy wave partners; the output selection and misuse contract; the device entry on a side stream
and captured into a HIP graph."""
import numpy as np
import pytest

import evaluate_cases as EC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    torch = pytest.importorskip("torch")
    import mpcqp
    import trajectory_tracking as TT
    dev = torch.device("cuda", 0)

    def ptr(a):
        t = torch.as_tensor(np.ascontiguousarray(a), device=dev)
        torch.cuda.synchronize()
        return t.data_ptr(), t

    yield dict(mpcqp=mpcqp, TT=TT, device=0, ptr=ptr, torch=torch, sync=torch.cuda.synchronize)
    torch.cuda.synchronize()
    EC.close_solvers()


def test_reference_pin(env):
    EC.check_reference_pin(env)


def test_summary_against_numpy(env):
    EC.check_golden_summary(env)


def test_golden_gpu_equals_host(env):
    host = dict(env, device=-1)
    for (key, _, rg), (_, _, rh) in zip(EC.evaluate_golden(env), EC.evaluate_golden(host)):
        for k in EC.KEYS:
            assert EC.same(rg[k], rh[k]), (key, k)


def test_consistency_with_the_solver(env):
    EC.check_solver_consistency(env)


@pytest.mark.parametrize("mo", EC.SHAPE_MO)
@pytest.mark.parametrize("N", EC.SHAPE_N)
def test_gpu_equals_host_bit_for_bit(env, N, mo):
    """N covers both lane-group boundaries (15 | 16, 31 | 32) and the limits (1, 63); B = 1, 5, 67 leave a partial
    tail group for every GL; n_obs NULL, all zero and mixed; every fifth instance rolls past s_max; NaN instances
    (x0 of instance 1, a control of the last) sit among healthy wave partners."""
    gpu, host = EC.solver(env, 2, N, mo), EC.solver(env, 2, N, mo, device=-1)
    for B, mode, w in EC.shape_runs(N, mo):
        rg = gpu.evaluate_batch(w["x0"], w["U"], w["obs"], w["n_obs"], rows=True)
        rh = host.evaluate_batch(w["x0"], w["U"], w["obs"], w["n_obs"], rows=True)
        for k in EC.KEYS:
            assert EC.same(rg[k], rh[k]), (N, mo, B, mode, k)
        if B >= 5:
            v, ng = EC.check_nan_isolation(gpu, w, B, rg)
            nh = host.evaluate_batch(v["x0"], v["U"], v["obs"], v["n_obs"], rows=True)
            for k in EC.KEYS:
                assert EC.same(ng[k], nh[k]), (N, mo, B, mode, k, "nan")


def test_output_selection(env):
    EC.check_output_selection(env)


def test_misuse(env):
    EC.check_misuse(env)
    env["sync"]()


def _device_call(env, slv, bufs, stream):
    p = lambda t: None if t is None else t.data_ptr()
    slv.evaluate_batch_device(bufs["x0"].shape[0], p(bufs["x0"]), p(bufs["obs"]), p(bufs["n_obs"]), p(bufs["U"]),
                              p(bufs["Xpred"]), p(bufs["summary"]), p(bufs["terms"]), p(bufs["rows"]), stream=stream)


def _buffers(env, slv, w):
    torch = env["torch"]
    dev = torch.device("cuda", 0)
    B, N, mo = w["x0"].shape[0], slv.params.N, slv.params.max_obs
    t = lambda a: None if a is None else torch.as_tensor(a, device=dev).contiguous()
    e = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=dev)
    return dict(x0=t(w["x0"]), U=t(w["U"]), obs=t(w["obs"]), n_obs=t(w["n_obs"]), Xpred=e(B, N + 1, 5),
                summary=e(B, 10), terms=e(B, 5), rows=e(B, N, 7 + mo))


def test_device_entry_on_a_stream_and_in_a_graph(env):
    """mpc_evaluate_batch_device on torch buffers: on a non-null stream it equals the host-buffer entry; captured
    once into a HIP graph and replayed twice with changed inputs it equals eager calls."""
    torch = env["torch"]
    slv = EC.solver(env, 2, 20, 3)
    wa, wb, wc = (EC.random_batch(2, 20, 67, 3, seed=s) for s in (91, 92, 93))
    want = [slv.evaluate_batch(w["x0"], w["U"], w["obs"], w["n_obs"], rows=True) for w in (wa, wb, wc)]
    bufs = _buffers(env, slv, wa)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    _device_call(env, slv, bufs, side.cuda_stream)
    side.synchronize()
    for k in EC.KEYS:
        assert EC.same(bufs[k].cpu().numpy(), want[0][k]), k
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        _device_call(env, slv, bufs, torch.cuda.current_stream().cuda_stream)
    for w, ref in ((wb, want[1]), (wc, want[2])):
        for k in ("x0", "U", "obs", "n_obs"):
            bufs[k].copy_(torch.as_tensor(w[k]))
        for k in EC.KEYS:
            bufs[k].fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        for k in EC.KEYS:
            assert EC.same(bufs[k].cpu().numpy(), ref[k]), k
