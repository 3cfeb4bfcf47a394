"""GPU tests of the host entries' staging (csrc/staging.h): a sequence of host-array calls of different shapes on ONE
context, so the context's arena is grown under live bindings, reused larger than needed and shared by every entry,
against the *_device entries driven with torch buffers on a SECOND context.  The kernels are the same, so every
comparison is bit for bit.  The entries that have no device twin (lookup, global_pose, noise_draw, route_eval) are
compared with the same call on a fresh context, whose arena holds exactly that call."""

import numpy as np
import pytest

from conftest import traj_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import torch
    import mpcqp
    import mpcplan
    import workloads as W
    return torch, mpcqp, mpcplan, W


def same(a, b, what):
    assert np.array_equal(a, b, equal_nan=True), what


def on_device(torch, call, ins, outs):
    """call(ptr) with ptr(name) -> the raw address of a torch copy of ins[name] (0 for None) or of an output tensor
    outs[name] = (shape, dtype) (0 for None); returns the outputs as numpy arrays."""
    dev = torch.device("cuda", 0)
    t = {k: None if v is None else torch.as_tensor(np.ascontiguousarray(v), device=dev) for k, v in ins.items()}
    for k, v in outs.items():
        t[k] = None if v is None else torch.full(v[0], -1 if v[1] == torch.int32 else float("nan"), dtype=v[1], device=dev)
    torch.cuda.synchronize()
    call(lambda k: 0 if t[k] is None else t[k].data_ptr())
    torch.cuda.synchronize()
    return {k: t[k].cpu().numpy() for k, v in outs.items() if v is not None}


def tracker_inputs(W, B, N, mo, seed):
    """x0, obstacles and n_obs of B egos of config C3 (a slab of 2), a control sequence and row weights."""
    wb = W.make_batch("C3", B=B, seed=seed)
    assert wb["max_obs"] == mo
    rng = np.random.default_rng(seed)
    return dict(traj=wb["traj"], x0=np.ascontiguousarray(wb["x0"]), obs=np.ascontiguousarray(wb["obs"]),
                n_obs=np.ascontiguousarray(wb["n_obs"], np.int32),
                U=rng.uniform(-0.2, 0.2, (B, N, 2)), lam=rng.uniform(0.0, 1.0, (B, N, 7 + mo)))


def dev_solve(torch, slv, w, N, obs):
    B, f, i = len(w["x0"]), torch.float64, torch.int32
    ins = dict(x0=w["x0"], obs=w["obs"] if obs else None, n_obs=w["n_obs"] if obs else None)
    outs = dict(u0=((B, 2), f), U=((B, N, 2), f), Xpred=((B, N + 1, 5), f), status=((B,), i), iters=((B,), i))
    return on_device(torch, lambda p: slv.solve_batch_device(B, p("x0"), p("obs"), p("n_obs"), 0, p("u0"), p("U"), p("Xpred"),
                                                             p("status"), p("iters")), ins, outs)


def dev_evaluate(torch, slv, w, N, mo):
    B, f = len(w["x0"]), torch.float64
    ins = dict(x0=w["x0"], obs=w["obs"], n_obs=w["n_obs"], U=w["U"])
    outs = dict(Xpred=((B, N + 1, 5), f), summary=((B, 10), f), terms=((B, 5), f), rows=((B, N, 7 + mo), f))
    return on_device(torch, lambda p: slv.evaluate_batch_device(B, p("x0"), p("obs"), p("n_obs"), p("U"), p("Xpred"),
                                                                p("summary"), p("terms"), p("rows")), ins, outs)


def dev_gradient(torch, slv, w, N, obs, lam, costate):
    B, f = len(w["x0"]), torch.float64
    ins = dict(x0=w["x0"], obs=w["obs"] if obs else None, n_obs=w["n_obs"] if obs else None, U=w["U"],
               lam=w["lam"] if lam else None)
    outs = dict(grad=((B, N, 2), f), jtl=((B, N, 2), f) if lam else None, gx0=((B, 5), f),
                costate=((B, N, 5), f) if costate else None, summary=((B, 6), f))
    return on_device(torch, lambda p: slv.gradient_batch_device(B, p("x0"), p("obs"), p("n_obs"), p("U"), p("lam"), p("grad"),
                                                                p("jtl"), p("gx0"), p("costate"), p("summary")), ins, outs)


def compare(host, dev, what):
    assert set(host) == set(dev), what
    for k in host:
        same(host[k], dev[k], (what, k))


def test_tracker_arena_one_context(env):
    """N = 5 (GL = 16, four instances per wavefront), max_obs = 2: the issue's nine calls on one context."""
    torch, mpcqp, _, W = env
    N, mo = 5, 2
    w3, w70, w5 = (tracker_inputs(W, B, N, mo, seed=100 + B) for B in (3, 70, 5))
    mk = lambda: mpcqp.Solver(*traj_arrays(w3["traj"]), mpcqp.default_params(N=N, max_obs=mo), device=0)
    host, dev = mk(), mk()
    # solve, B = 3, no obstacles
    compare(host.solve_batch(w3["x0"]), dev_solve(torch, dev, w3, N, obs=False), "solve B=3")
    # gradient, B = 3, with lam and costate
    compare(host.gradient_batch(w3["x0"], w3["U"], lam=w3["lam"], costate=True),
            dev_gradient(torch, dev, w3, N, obs=False, lam=True, costate=True), "gradient B=3")
    # evaluate, B = 70, obstacles and rows: grows the arena
    compare(host.evaluate_batch(w70["x0"], w70["U"], w70["obs"], w70["n_obs"], rows=True),
            dev_evaluate(torch, dev, w70, N, mo), "evaluate B=70")
    # solve, B = 70, obstacles and n_obs
    r70 = host.solve_batch(w70["x0"], w70["obs"], w70["n_obs"])
    compare(r70, dev_solve(torch, dev, w70, N, obs=True), "solve B=70")
    assert (r70["iters"] > 0).any()
    # lookup, global_pose, noise_draw: a fresh context each time is the reference
    s = np.linspace(1.0, 300.0, 7)
    fresh = mk()
    for a, b in zip(host.lookup(s), fresh.lookup(s)):
        same(a, b, "lookup n=7")
    same(host.global_pose(s, np.linspace(-1.0, 1.0, 7)), mk().global_pose(s, np.linspace(-1.0, 1.0, 7)), "pose n=7")
    draw = (11, np.arange(5, dtype=np.int64), np.arange(5, dtype=np.int32), np.array([0, 5, 7, 16, 47], np.int32))
    for a, b in zip(host.noise_draw(*draw), mk().noise_draw(*draw)):
        same(a, b, "noise_draw n=5")
    # solve, B = 5, U and Xpred NULL: u0 sits in a NaN block whose remainder must stay NaN
    d5 = dev_solve(torch, dev, w5, N, obs=True)
    block = np.full(2 * 5 + 2 * N * 5 + 5 * (N + 1) * 5, np.nan)
    st, it = np.full(5 + 8, -1, np.int32), np.full(5 + 8, -1, np.int32)
    L, p, pi = mpcqp.lib(), mpcqp._p, mpcqp._pi
    rc = L.mpc_solve_batch(host.h, 5, p(w5["x0"]), p(w5["obs"]), pi(w5["n_obs"]), None, p(block), None, None, pi(st), pi(it))
    assert rc == 0, mpcqp.last_error()
    same(block[:10].reshape(5, 2), d5["u0"], "solve B=5 u0")
    same(st[:5], d5["status"], "solve B=5 status")
    same(it[:5], d5["iters"], "solve B=5 iters")
    assert np.isnan(block[10:]).all() and (st[5:] == -1).all() and (it[5:] == -1).all()
    # gradient, B = 5, without lam: grad, gx0 and summary in one NaN block with gaps as wide as jtl and costate
    g5 = dev_gradient(torch, dev, w5, N, obs=True, lam=False, costate=False)
    n_u, n_c = 5 * N * 2, 5 * N * 5
    block = np.full(n_u + n_u + 5 * 5 + n_c + 5 * 6, np.nan)
    o_gx0, o_sum = 2 * n_u, 2 * n_u + 25 + n_c
    rc = L.mpc_gradient_batch(host.h, 5, p(w5["x0"]), p(w5["obs"]), pi(w5["n_obs"]), p(w5["U"]), None, p(block), None,
                              p(block[o_gx0:]), None, p(block[o_sum:]))
    assert rc == 0, mpcqp.last_error()
    same(block[:n_u].reshape(5, N, 2), g5["grad"], "gradient B=5 grad")
    same(block[o_gx0:o_gx0 + 25].reshape(5, 5), g5["gx0"], "gradient B=5 gx0")
    same(block[o_sum:].reshape(5, 6), g5["summary"], "gradient B=5 summary")
    assert np.isnan(block[n_u:o_gx0]).all() and np.isnan(block[o_gx0 + 25:o_sum]).all()
    assert not np.isnan(g5["grad"]).any()


def test_tracker_arena_gl32(env):
    """N = 16, the first horizon at GL = 32: solve and evaluate at B = 3, then at B = 35."""
    torch, mpcqp, _, W = env
    N, mo = 16, 2
    w3 = tracker_inputs(W, 3, N, mo, seed=203)
    mk = lambda: mpcqp.Solver(*traj_arrays(w3["traj"]), mpcqp.default_params(N=N, max_obs=mo), device=0)
    host, dev = mk(), mk()
    for B in (3, 35):
        w = tracker_inputs(W, B, N, mo, seed=200 + B)
        compare(host.solve_batch(w["x0"], w["obs"], w["n_obs"]), dev_solve(torch, dev, w, N, obs=True), ("solve", B))
        compare(host.evaluate_batch(w["x0"], w["U"], w["obs"], w["n_obs"], rows=True), dev_evaluate(torch, dev, w, N, mo),
                ("evaluate", B))


def plan_inputs(W, route, horizons, per, seed, final_frac=0.3):
    """per chunks at each of `horizons`, interleaved; N [B].  (A final chunk of 5 stages or fewer cannot stop in time
    and ends PLAN_QP_FAILED; it is compared like every other chunk.)"""
    bs = [W.plan_batch(route, n, per, seed=seed + n, final_frac=final_frac) for n in horizons]
    order = [(i, j) for j in range(per) for i in range(len(horizons))]
    return dict(x0=np.array([bs[i]["x0"][j] for i, j in order]), s_target=np.array([bs[i]["s_target"][j] for i, j in order]),
                is_final=np.array([bs[i]["is_final"][j] for i, j in order], np.int32),
                N=np.array([horizons[i] for i, _ in order], np.int32))


def dev_plan_solve(torch, pl, w, Nmax, with_N):
    B, f, i = len(w["x0"]), torch.float64, torch.int32
    ins = dict(x0=w["x0"], st=w["s_target"], fin=w["is_final"], N=w["N"] if with_N else None)
    outs = dict(X=((B, Nmax + 1, 5), f), U=((B, Nmax, 2), f), S=((B, Nmax), f), status=((B,), i), iters=((B,), i),
                sqp=((B,), i))
    return on_device(torch, lambda p: pl.solve_chunks_device(B, Nmax, p("N"), p("x0"), p("st"), p("fin"), p("X"), p("U"),
                                                             p("S"), p("status"), p("iters"), p("sqp")), ins, outs)


def compare_chunks(host, dev, Nv, what):
    """Rows past a chunk's horizon are not written by the kernel: compared up to N[b]."""
    for k in ("status", "iters", "sqp"):
        same(host[k], dev[k], (what, k))
    for b, n in enumerate(Nv):
        same(host["X"][b, :n + 1], dev["X"][b, :n + 1], (what, "X", b))
        same(host["U"][b, :n], dev["U"][b, :n], (what, "U", b))
        same(host["S"][b, :n], dev["S"][b, :n], (what, "S", b))


def test_planner_arena_one_context(env):
    """The issue's six planner calls on one context; B < 2 * 64 keeps every launch in index order."""
    torch, _, mpcplan, W = env
    route = W.plan_route("traj1")
    mk = lambda: mpcplan.Planner(route, mpcplan.default_params(N=5), device=0)
    host, dev = mk(), mk()
    f = torch.float64
    # solve_chunks, B = 2, N = None (params.N = 5)
    w2 = plan_inputs(W, route, (5,), 2, seed=1, final_frac=0.0)
    h2 = host.solve_chunks(w2["x0"], w2["s_target"], w2["is_final"])
    compare_chunks(h2, dev_plan_solve(torch, dev, w2, 5, with_N=False), w2["N"], "solve_chunks B=2")
    assert np.isin(h2["status"], (0, 4)).all()
    # evaluate_chunks on its result
    he = host.evaluate_chunks(w2["x0"], w2["s_target"], w2["is_final"], h2["X"], h2["U"], h2["S"])
    ins = dict(x0=w2["x0"], st=w2["s_target"], fin=w2["is_final"], X=h2["X"], U=h2["U"], S=h2["S"])
    outs = dict(summary=((2, mpcplan.PLAN_EV_NQ), f), defects=((2, 5, 5), f), rows=((2, 6, mpcplan.PLAN_EV_NR), f))
    de = on_device(torch, lambda p: dev.evaluate_chunks_device(2, 5, 0, p("x0"), p("st"), p("fin"), p("X"), p("U"), p("S"),
                                                               p("summary"), p("defects"), p("rows")), ins, outs)
    compare(he, de, "evaluate_chunks B=2")
    # solve_chunks, B = 9, per-chunk N in {3, 5, 17}
    w9 = plan_inputs(W, route, (3, 5, 17), 3, seed=2)
    compare_chunks(host.solve_chunks(w9["x0"], w9["s_target"], w9["is_final"], N=w9["N"]),
                   dev_plan_solve(torch, dev, w9, 17, with_N=True), w9["N"], "solve_chunks B=9")
    # plan_optimize, B = 2, max_chunks = 3, Nmax = 17
    vm = np.asarray(route.vmax, np.float64)
    avg = np.array([float(np.mean(vm[i:])) for i in range(vm.size)])
    starts = w9["x0"][[1, 4]].copy()
    ho = host.optimize_device(starts, 10.0, 3, avg, 17)
    i32 = torch.int32
    outs = dict(X=((2, 3, 18, 5), f), U=((2, 3, 17, 2), f), S=((2, 3, 17), f), nchunks=((2,), i32),
                **{k: ((2, 3), i32) for k in ("N", "is_final", "status", "iters", "sqp")})
    do = on_device(torch, lambda p: mpcplan._check(mpcplan.lib().plan_optimize_device(
        dev.h, 2, 17, p("starts"), 10.0, 3, p("avg"), avg.size, p("X"), p("U"), p("S"), p("N"), p("is_final"), p("status"),
        p("iters"), p("sqp"), p("nchunks"), None), "plan_optimize_device"), dict(starts=starts, avg=avg), outs)
    same(ho["nchunks"], do["nchunks"], "optimize nchunks")
    assert (ho["nchunks"] >= 1).all() and (ho["nchunks"] <= 3).all()
    for b in range(2):                      # slots past nchunks[b] are not written
        for ch in range(int(ho["nchunks"][b])):
            for k in ("N", "is_final", "status", "iters", "sqp"):
                same(ho[k][b, ch], do[k][b, ch], ("optimize", k, b, ch))
            n = int(ho["N"][b, ch])
            assert 1 <= n <= 17
            same(ho["X"][b, ch, :n + 1], do["X"][b, ch, :n + 1], ("optimize X", b, ch))
            same(ho["U"][b, ch, :n], do["U"][b, ch, :n], ("optimize U", b, ch))
            same(ho["S"][b, ch, :n], do["S"][b, ch, :n], ("optimize S", b, ch))
    # route_eval, n = 6, against a fresh context
    s = np.linspace(2.0, route.s_total - 2.0, 6)
    for a, b in zip(host.route_eval(s), mk().route_eval(s)):
        same(a, b, "route_eval n=6")
    # solve_chunks, B = 3 again: the arena is larger than needed now
    w3 = plan_inputs(W, route, (5,), 3, seed=3)
    compare_chunks(host.solve_chunks(w3["x0"], w3["s_target"], w3["is_final"]),
                   dev_plan_solve(torch, dev, w3, 5, with_N=False), w3["N"], "solve_chunks B=3")


def test_plan_evaluate_partial_copy_back(env):
    """plan_evaluate_chunks with N = [5, 0, 5]: chunk 1 is out of range, so its defects and rows keep what the caller's
    arrays held; chunks 0 and 2 are written and the summary is written for all three."""
    _, _, mpcplan, W = env
    route = W.plan_route("traj1")
    pl = mpcplan.Planner(route, mpcplan.default_params(N=5), device=0)
    w = plan_inputs(W, route, (5,), 3, seed=4)
    r = pl.solve_chunks(w["x0"], w["s_target"], w["is_final"])
    full = pl.evaluate_chunks(w["x0"], w["s_target"], w["is_final"], r["X"], r["U"], r["S"])
    Nv = np.array([5, 0, 5], np.int32)
    summary, defects, rows = np.full((3, mpcplan.PLAN_EV_NQ), 77.0), np.full((3, 5, 5), 77.0), np.full((3, 6, 12), 77.0)
    p = mpcplan._p
    rc = mpcplan.lib().plan_evaluate_chunks(pl.h, 3, 5, mpcplan._pi(Nv), p(w["x0"]), p(w["s_target"]),
                                            mpcplan._pi(w["is_final"]), p(r["X"]), p(r["U"]), p(r["S"]), p(summary),
                                            p(defects), p(rows))
    assert rc == 0, mpcplan.last_error()
    assert (defects[1] == 77.0).all() and (rows[1] == 77.0).all()
    for b in (0, 2):
        same(defects[b], full["defects"][b], ("defects", b))
        same(rows[b], full["rows"][b], ("rows", b))
        same(summary[b], full["summary"][b], ("summary", b))
    assert not (summary[1] == 77.0).any()
