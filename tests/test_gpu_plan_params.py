"""The planner on the GPU away from plan_default_params (csrc/plan_kernel.h, plan_evaluate_kernel.h, plan.hip's copy
of the parameters to the device), under the parameter sets of tests/plan_params_cases.py.  The bounds are those of
tests/test_gpu_plan.py (compare(): 1e-8 on chunks both sides converge, status agreement >= 0.99, both converged on
>= 95% of the chunks the oracle does not report PLAN_QP_FAILED) and, for the evaluator, 8 x the host backend's measured
error against plan_ref (plan_params_cases.TOL_*).  tests/test_plan_params_cpu.py asserts that the oracle converges on
at least half of every batch used here, pins the oracle to scipy SLSQP under the sets, and runs the kernel's source on
the CPU under set A."""
import numpy as np
import pytest

import plan_evaluate_cases as PC
import plan_params_cases as PP
from test_gpu_plan import compare
from test_plan_params_cpu import check_optimize_loop, check_set_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import mpcplan
    import plan_oracle as PO
    import workloads as W
    return mpcplan, PO, W


@pytest.mark.parametrize("name,N,route", PP.GPU_CASES + (("A", 10, "traj1"),))
def test_chunks_vs_oracle(env, name, N, route):
    """64 chunks per set and shape: N = 5 (a single lane group), 20, 33 (just past a 32-stage boundary) under A and B,
    N = 20 under each single-group set; and the traj1 N = 10 batch whose chunk 62 freezes its limits under set A."""
    mpcplan, PO, W = env
    r = W.plan_route(route)
    ps = PP.pset(name)
    wb = PP.batch(W, r, N, ps)
    pl = mpcplan.Planner(r, PP.lib_params(mpcplan, ps, N=N))
    g = pl.solve_chunks(wb["x0"], wb["s_target"], wb["is_final"])
    pl.close()
    o = PO.PlanOracle(r).solve_batch(PP.lib_params(PO, ps, N=N), wb["x0"], wb["s_target"], wb["is_final"], num_threads=16)
    both = compare(f"set {name} N={N} {route}", g, o)
    assert np.isin(o["status"], (0, 4)).sum() >= 32
    # a bound decides a plan only where its row is active: the batches that move a_max, k_min or k_max hold chunks,
    # converged on both sides, with a lateral-acceleration row active at the optimum, and G one at a curvature bound
    lat, cur = PP.active_rows(o, PP.lib_params(PO, ps, N=N))
    print(f"set {name} N={N} {route}: active lateral row in chunks {np.flatnonzero(lat & both).tolist()}, "
          f"curvature bound in {np.flatnonzero(cur & both).tolist()}")
    if "a_max" in ps and N >= 20:
        assert (lat & both).any(), (name, N)
    if name == "G":
        assert (cur & both).any()


@pytest.mark.parametrize("name", ["A", "GK"])
def test_launch_order_changes_nothing(env, name):
    """160 chunks of mixed N in {8, 16, 24} in one call (longest-first order, whose score divides by
    max(|k_min|, |k_max|) and by a_max) equal the same chunks solved in two calls of 80 (index order), every output
    bit for bit: under set A, and under k_min = -k_max = 0.01, which spreads the scores over every bucket."""
    mpcplan, PO, W = env
    r = W.plan_route("synth1")
    x0, st, fin, N = PP.order_batch(W, r)
    pl = mpcplan.Planner(r, PP.lib_params(mpcplan, PP.pset(name), N=24))
    one = pl.solve_chunks(x0, st, fin, N)
    halves = [pl.solve_chunks(x0[h], st[h], fin[h], N[h]) for h in (slice(0, 80), slice(80, 160))]
    pl.close()
    print(f"set {name}: 160 chunks in one call, statuses {PP.counts(one['status'])}")
    for k in PP.OUTPUTS:
        assert np.array_equal(one[k], np.concatenate([h[k] for h in halves])), (name, k)


def test_set_params_on_a_device_context(env):
    mpcplan, PO, W = env
    check_set_params(mpcplan, W, 0)


def test_device_entry_equals_host_entry_under_set_B(env):
    import torch
    mpcplan, PO, W = env
    r = W.plan_route("synth1")
    ps = PP.pset("B")
    x0n, stn, finn, _ = PP.mixed_batch(W, r, ps, n=64)
    B, N = 64, 16
    pl = mpcplan.Planner(r, PP.lib_params(mpcplan, ps, N=N))
    h = pl.solve_chunks(x0n, stn, finn)
    dev = torch.device("cuda", 0)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=dev).contiguous()
    x0, st, fin = t(x0n), t(stn), t(finn, torch.int32)
    X = torch.empty((B, N + 1, 5), dtype=torch.float64, device=dev)
    U = torch.empty((B, N, 2), dtype=torch.float64, device=dev)
    S = torch.empty((B, N), dtype=torch.float64, device=dev)
    o = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3)]
    pl.solve_chunks_device(B, N, 0, x0.data_ptr(), st.data_ptr(), fin.data_ptr(), X.data_ptr(), U.data_ptr(),
                           S.data_ptr(), *[a.data_ptr() for a in o], stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    pl.close()
    print(f"set B device entry: statuses {PP.counts(h['status'])}")
    for a, k in ((X, "X"), (U, "U"), (S, "S"), (o[0], "status"), (o[1], "iters"), (o[2], "sqp")):
        assert np.array_equal(a.cpu().numpy(), h[k]), k
    assert np.isin(h["status"], (0, 4)).mean() >= 0.5


@pytest.mark.parametrize("name", PP.EV_SETS)
def test_device_evaluator_against_host_backend(env, name):
    mpcplan, PO, W = env
    Q = mpcplan.EVQ
    cs = list(PP.ev_cases(name))
    a = PC.pack(cs)
    r = W.plan_route(PP.EV_ROUTE)
    dev = mpcplan.Planner(r, PP.lib_params(mpcplan, PP.pset(name), N=20), device=0)
    host = mpcplan.Planner(r, PP.lib_params(mpcplan, PP.pset(name), N=20), device=-1)
    d, h = PC.evaluate(dev, a), PC.evaluate(host, a)
    dev.close()
    host.close()
    ed = float(np.nanmax(np.abs(d["defects"] - h["defects"])))
    es = max(float((np.abs(d["summary"][:, Q[c]] - h["summary"][:, Q[c]]) / (1.0 + np.abs(h["summary"][:, Q[c]]))).max())
             for c in PC.ARITH_COLUMNS)
    print(f"set {name}: device evaluator against host: defects {ed:.3e} (bound {PP.TOL_DEFECTS:.3e}), "
          f"COST / MAX_DEFECT / L1_EQ {es:.3e} (bound {PP.TOL_SUMS:.3e})")
    assert PC.same(np.isnan(d["defects"]), np.isnan(h["defects"]))
    assert PC.same(d["rows"], h["rows"])
    for col in PC.EXACT_COLUMNS:
        assert PC.same(d["summary"][:, Q[col]], h["summary"][:, Q[col]]), col
    assert ed <= PP.TOL_DEFECTS
    assert es <= PP.TOL_SUMS
    PC.errors_against_ref(cs, d)            # the exact parts against plan_ref: NaN patterns, N_NEG, ARGMIN_*


def test_device_optimize_loop_equals_oracle_loop_under_set_A(env):
    """plan_optimize_device under set A, three starts on synth1, against the package loop driven by the oracle under
    set A (the host version in test_plan_params_cpu.py is bit for bit; the device's sin / cos differ from libm's).
    Each plan is compared up to its first chunk that the oracle does not converge on (compare()'s rule: a chunk that
    stops at sqp_iters has no common point to agree on, and the next start is taken from it): the same horizons (by the
    set's dt) and statuses, the committed rows within compare()'s 1e-8.  The whole plans equal, bit for bit, the round
    loop's on the device (one batched launch per round), as test_gpu_plan.test_device_loop_equals_round_loop."""
    mpcplan, PO, W = env
    import trajectory_planning as TP
    from test_gpu_plan import TOL
    ref, qref, got, qgot = check_optimize_loop(mpcplan, PO, W, 0)
    worst, compared = 0.0, []
    for b in range(3):
        st = qref[b]["statuses"]
        j = next((i for i, v in enumerate(st) if v not in (0, 4)), len(st))
        assert qgot[b]["horizons"][:j + 1] == qref[b]["horizons"][:j + 1] and qgot[b]["statuses"][:j] == st[:j], b
        final = j == len(st)
        rows = sum(h // 2 for h in qref[b]["horizons"][:j - 1 if final else j]) + (qref[b]["horizons"][-1] if final else 0)
        for a, c, extra in zip(got[b], ref[b], (1, 0, 0)):
            worst = max(worst, float(np.abs(a[:rows + extra] - c[:rows + extra]).max()))
        compared.append(j)
    print(f"set A device loop against the oracle's loop: chunks compared {compared} of {[len(q['statuses']) for q in qref]}, "
          f"max err {worst:.1e}")
    assert worst <= TOL
    assert all(j >= 1 for j in compared)
    rnd, qrnd = TP.optimize_full_trajectory_batch(W.plan_route("synth1"), PP.loop_starts(W.plan_route("synth1")),
                                                  device_loop=False, optimizer=PP.loop_optimizer(TP, PP.pset("A"), 0))
    for b in range(3):
        assert qrnd[b]["statuses"] == qgot[b]["statuses"] and qrnd[b]["horizons"] == qgot[b]["horizons"], b
        for a, c in zip(got[b], rnd[b]):
            assert np.array_equal(a, c), b
