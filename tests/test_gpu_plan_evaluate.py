"""The planner's evaluator on the GPU (plan_evaluate_kernel, csrc/plan_evaluate_kernel.h) against the host backend
(device = -1), whose agreement with the numpy restatement of the reference NLP tests/test_plan_evaluate_cpu.py pins.
Cases and tolerances: tests/plan_evaluate_cases.py.  Per route one call of B = 12 chunks at the horizons
{1, 2, 63, 64, 65, 130}, final and intermediate mixed: the comparisons (min / max / abs columns, the NaN pattern, the
integer columns, the rows, which hold no sin / cos) are equal bit for bit; the defects, COST, MAX_DEFECT and L1_EQ
agree within the measured bounds (TOL_DEFECTS absolute, TOL_SUMS relative to 1 + |host|)."""
import numpy as np
import pytest

import plan_evaluate_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import mpcplan
    import workloads as W
    return mpcplan, W


@pytest.fixture(scope="module")
def both(env):
    """{route: (packed inputs, device result, host result, device planner)}, computed once."""
    mpcplan, W = env
    out = {}
    for rn in PC.ROUTES:
        a = PC.pack(PC.cases(rn))
        dev = mpcplan.Planner(W.plan_route(rn), mpcplan.default_params(N=20), device=0)
        host = mpcplan.Planner(W.plan_route(rn), mpcplan.default_params(N=20), device=-1)
        d, h = PC.evaluate(dev, a), PC.evaluate(host, a)
        host.close()
        for r in (d, h):
            for v in r.values():
                v.setflags(write=False)
        out[rn] = (a, d, h, dev)
    yield out
    for rn in out:
        out[rn][3].close()


@pytest.mark.parametrize("rn", PC.ROUTES)
def test_device_against_host_backend(env, both, rn):
    mpcplan, W = env
    Q = mpcplan.EVQ
    a, d, h, _ = both[rn]
    assert a["X"].shape[0] == 12
    assert PC.same(np.isnan(d["defects"]), np.isnan(h["defects"]))
    assert PC.same(d["rows"], h["rows"])
    for col in PC.EXACT_COLUMNS:
        assert PC.same(d["summary"][:, Q[col]], h["summary"][:, Q[col]]), col
    ed = float(np.nanmax(np.abs(d["defects"] - h["defects"])))
    es = max(float((np.abs(d["summary"][:, Q[c]] - h["summary"][:, Q[c]]) / (1.0 + np.abs(h["summary"][:, Q[c]]))).max())
             for c in PC.ARITH_COLUMNS)
    print(f"{rn}: device against host: defects {ed:.3e} (bound {PC.TOL_DEFECTS:.3e}), "
          f"COST / MAX_DEFECT / L1_EQ {es:.3e} (bound {PC.TOL_SUMS:.3e})")
    assert ed <= PC.TOL_DEFECTS
    assert es <= PC.TOL_SUMS
    # and the device against plan_ref directly, the exact parts (N_NEG, ARGMIN_*, the NaN patterns) included
    PC.errors_against_ref(PC.cases(rn), d)
    v_d, v_h = both[rn][3].check_verdicts(d["summary"]), both[rn][3].check_verdicts(h["summary"])
    assert PC.same(v_d["verdicts"], v_h["verdicts"]) and PC.same(v_d["counts"], v_h["counts"])


def test_device_pointer_entry_and_graph_replay(env, both):
    """plan_evaluate_chunks_device with device pointers equals the host-pointer entry bit for bit; one call captured
    into a HIP graph after an eager warm-up and replayed once gives the same bits again."""
    import torch
    mpcplan, W = env
    rn = "synth1"
    a, d, _, pl = both[rn]
    dev = torch.device("cuda:0")
    t = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=dev)
    ins = [t(a["N"], torch.int32), t(a["x0"]), t(a["s_target"]), t(a["is_final"], torch.int32), t(a["X"]), t(a["U"]), t(a["S"])]
    B, Nm = 12, a["Nmax"]

    def outputs():
        return [torch.full(s, -1.0, dtype=torch.float64, device=dev)
                for s in ((B, mpcplan.PLAN_EV_NQ), (B, Nm, 5), (B, Nm + 1, 12))]

    def call(outs, stream):
        pl.evaluate_chunks_device(B, Nm, *[x.data_ptr() for x in ins], *[o.data_ptr() for o in outs], stream=stream)

    def check(outs, what):
        for o, k in zip(outs, ("summary", "defects", "rows")):
            assert PC.same(o.cpu().numpy(), d[k]), (what, k)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    eager = outputs()
    with torch.cuda.stream(side):
        call(eager, side.cuda_stream)
    torch.cuda.synchronize(dev)
    check(eager, "eager")
    cap = outputs()
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        call(cap, torch.cuda.current_stream(dev).cuda_stream)
    for o in cap:
        o.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize(dev)
    check(cap, "replay")


def test_solve_then_evaluate(env):
    """End to end: solve_chunks on W.plan_batch(traj1, N = 20, B = 64), then evaluate_chunks on the result: the
    converged chunks start exactly at x0 and their largest defect is within 10 x the CPU oracle's own
    (plan_evaluate_cases.E2E_MAX_DEFECT)."""
    mpcplan, W = env
    Q = mpcplan.EVQ
    r = W.plan_route("traj1")
    wb = W.plan_batch(r, 20, 64, seed=20, final_frac=0.25)
    pl = mpcplan.Planner(r, mpcplan.default_params(N=20), device=0)
    s = pl.solve_chunks(wb["x0"], wb["s_target"], wb["is_final"])
    q = pl.evaluate_chunks(wb["x0"], wb["s_target"], wb["is_final"], s["X"], s["U"], s["S"], want=("summary",))["summary"]
    pl.close()
    ok = s["status"] == mpcplan.PLAN_OK
    print(f"statuses {np.bincount(s['status'], minlength=5).tolist()}, PLAN_OK: max X0_RES {q[ok, Q['x0_res']].max():.3e}, "
          f"max MAX_DEFECT {q[ok, Q['max_defect']].max():.3e} (bound {PC.E2E_MAX_DEFECT:.3e})")
    assert ok.sum() >= 32
    assert (q[ok, Q["x0_res"]] == 0.0).all()
    assert q[ok, Q["max_defect"]].max() <= PC.E2E_MAX_DEFECT
