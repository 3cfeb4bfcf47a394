"""The planner away from plan_default_params, without a GPU: the oracle (oracle/plan_oracle.c), the host backend
(device = -1: csrc/plan_host.h, plan_evaluate_host.h, plan_model.h), the drop-in and the emulated kernel
(tools/plan_emu.cpp: csrc/plan_kernel.h compiled for the host) under the parameter sets of tests/plan_params_cases.py.
Every other planner test runs at the defaults, where a literal left in place of a field, two swapped weights or
u_min read for u_max cannot show.

  - the oracle's NLP functions and its optimum against the parametrised numpy restatement (oracle/plan_ref.py) and
    scipy SLSQP on it, with the bounds of tests/test_plan_oracle.py;
  - the host backend against the oracle bit for bit per set, plan_set_params, the drop-in's params() and optimize,
    plan_optimize's loop against the package loop driven by the oracle;
  - the host evaluator against plan_ref per set, within 8 x the measured error (plan_params_cases.MEASURED_*);
  - the kernel's source on the CPU under set A against the oracle (1e-8, the GPU tests' bound);
  - the condition the GPU comparisons rest on: the oracle converges on at least half of every batch they use.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import plan_evaluate_cases as PC
import plan_params_cases as PP
from conftest import ROOT


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import mpcplan
    import plan_oracle as PO
    import plan_ref as PR
    import workloads as W
    return mpcplan, PO, PR, W


def test_default_parameter_object_is_the_reference(env):
    mpcplan, PO, PR, W = env
    d, p = PR.DEFAULT, mpcplan.default_params()
    assert (d.w_y, d.w_s, d.w_u, d.w_slack) == (10.0, 10.0, 0.1, 100.0) == (p.w_y, p.w_s, p.w_u, p.w_slack)
    assert d.u_min.tolist() == [-0.6, -5.0] == list(p.u_min) and d.u_max.tolist() == [0.6, 4.0] == list(p.u_max)
    assert (d.k_min, d.k_max, d.a_max, d.v_min, d.defect_sign) == (-0.8, 0.8, 6.0, 0.0, 1.0) == \
        (p.k_min, p.k_max, p.a_max, p.v_min, p.defect_sign)
    assert PP.fields(p) == PP.fields(PO.default_params())
    # every set changes what it says it changes, on both structures, and A and B between them every model field
    for name, ps in PP.SETS.items():
        for mod in (mpcplan, PO):
            q = PP.lib_params(mod, ps)
            for f in PP.MODEL_FIELDS:
                v = getattr(q, f)
                v = tuple(v) if f in ("u_min", "u_max") else v
                assert v == ps.get(f, tuple(getattr(p, f)) if f in ("u_min", "u_max") else getattr(p, f)), (name, f)
    moved = {f for n in ("A", "B", "S") for f in PP.SETS[n]}
    assert moved == set(PP.MODEL_FIELDS)


@pytest.mark.parametrize("name", ["A", "B", "S"])
def test_oracle_nlp_functions_match_plan_ref(env, name):
    mpcplan, PO, PR, W = env
    r = W.plan_route("traj2")
    orc = PO.PlanOracle(r)
    ps = PP.pset(name)
    p = PP.lib_params(PO, ps, N=10)
    params, dt = PP.ref_params(ps)
    rng = np.random.default_rng(1)
    for _ in range(50):
        xa = np.array([rng.uniform(5, r.s_total - 20), rng.normal(0, 0.3), rng.normal(0, 0.1), rng.normal(0, 0.2),
                       rng.uniform(0, 14)])
        xb = xa + np.array([rng.uniform(0, 4), *rng.normal(0, 0.05, 4)])
        u = rng.normal(0, 0.5, 2)
        ch = PR.Chunk(r, 1, dt, xa, xa[0] + 20, False, params)
        X = np.stack([xa, xb])
        assert np.abs(orc.defect(p, xa, xb, u) - ch.defect(X, u[None], 0)).max() <= 1e-12
        z = np.concatenate([X.ravel(), u, [0.05]])
        assert abs(orc.cost(p, 1, xa, X, u, np.array([0.05])) - ch.cost(z)) <= 1e-12 * (1 + abs(ch.cost(z)))


@pytest.mark.parametrize("name,N,final", [("A", 10, 0), ("A", 12, 1), ("B", 10, 0), ("S", 10, 0), ("S", 12, 1)])
def test_oracle_optimum_matches_slsqp(env, name, N, final):
    """test_plan_oracle.test_oracle_optimum_matches_slsqp under a set: chunks the oracle solves are feasible for the
    parametrised plan_ref to 1e-9, scipy SLSQP (analytic Jacobians, ftol 1e-14) started there moves <= 1e-6 and
    finds no cost lower by more than 1e-8.  The final batch only for the sets with v_min = 0 (a final chunk is
    infeasible in the reference at v_min > 0, see plan_params_cases)."""
    mpcplan, PO, PR, W = env
    ps = PP.pset(name)
    assert not (final and PP.intermediate_only(ps))
    r = W.plan_route("traj1")
    orc = PO.PlanOracle(r)
    params, dt = PP.ref_params(ps)
    wb = W.plan_batch(r, N, 6, seed=3, final_frac=float(final))
    o = orc.solve_batch(PP.lib_params(PO, ps, N=N), wb["x0"], wb["s_target"], wb["is_final"])
    checked, worst = 0, 0.0
    for b in range(6):
        if o["status"][b] != 0:
            continue
        ch = PR.Chunk(r, N, dt, wb["x0"][b], wb["s_target"][b], bool(wb["is_final"][b]), params)
        z = np.concatenate([o["X"][b].ravel(), o["U"][b].ravel(), o["S"][b]])
        assert np.abs(ch.eq(z)).max() <= 1e-9 and ch.ineq(z).min() >= -1e-9, (name, b)
        rt, _ = ch.slsqp(ftol=1e-14, maxiter=400, jac=True, z0=z)
        worst = max(worst, float(np.abs(rt.x - z).max()))
        assert np.abs(rt.x - z).max() <= 1e-6, (name, b, np.abs(rt.x - z).max())
        assert rt.fun >= ch.cost(z) - 1e-8
        checked += 1
        if checked == 3:
            break
    # Under S every final chunk of the batch is infeasible: time runs backwards, the start speed is positive, and the
    # control bounds cannot turn it round and still reach s_target with v_N = 0 inside the horizon.  The oracle says
    # PLAN_QP_FAILED; where no chunk converged, the agreement checked is that scipy SLSQP from the reference's own
    # initial guess finds no feasible point of the parametrised plan_ref either (equality residual ~ 1.5 to 2).
    infeasible = 0
    for b in range(6):
        if checked + infeasible >= 2 or o["status"][b] != mpcplan.PLAN_QP_FAILED:
            continue
        ch = PR.Chunk(r, N, dt, wb["x0"][b], wb["s_target"][b], bool(wb["is_final"][b]), params)
        rt, _ = ch.slsqp(ftol=1e-14, maxiter=400, jac=True)
        res = float(np.abs(ch.eq(rt.x)).max())
        print(f"set {name} N={N} chunk {b}: oracle PLAN_QP_FAILED, SLSQP status {rt.status}, max |eq| {res:.2e}")
        assert not rt.success and res > 1e-3, (name, b, rt.status, res)
        infeasible += 1
    print(f"set {name} N={N} final={final}: statuses {PP.counts(o['status'])}, checked {checked}, "
          f"largest SLSQP move {worst:.1e}, infeasible on both sides {infeasible}")
    assert checked + infeasible >= 2
    assert checked >= 2 or (name, final) == ("S", 1)


@pytest.mark.parametrize("name", list(PP.SETS))
def test_host_backend_equals_oracle_bit_for_bit(env, name):
    """test_plan_host.test_host_backend_equals_oracle_bit_for_bit under a set: the mixed batch of 48 chunks, N in
    {13, 16, 20, 26}, every output."""
    mpcplan, PO, PR, W = env
    r = W.plan_route("synth1")
    ps = PP.pset(name)
    x0, st, fin, N = PP.mixed_batch(W, r, ps)
    pl = mpcplan.Planner(r, PP.lib_params(mpcplan, ps, N=int(N.max())), device=-1)
    got = pl.solve_chunks(x0, st, fin, N)
    pl.close()
    ref = PO.PlanOracle(r).solve_batch(PP.lib_params(PO, ps, N=int(N.max())), x0, st, fin, N=N, num_threads=4)
    dflt = PO.PlanOracle(r).solve_batch(PO.default_params(N=int(N.max())), x0, st, fin, N=N, num_threads=4)
    print(f"set {name}: statuses {PP.counts(got['status'])}, QPs {int(got['sqp'].sum())}, largest |X - X at the "
          f"defaults| {np.abs(ref['X'] - dflt['X']).max():.2f}")
    for k in PP.OUTPUTS:
        assert np.array_equal(got[k], ref[k]), (name, k)
    assert np.isin(got["status"], (0, 4)).mean() >= 0.75
    assert np.abs(ref["X"] - dflt["X"]).max() > 1e-3         # the set is felt


def test_host_backend_on_the_chunk_that_freezes_under_set_A(env):
    """W.plan_batch(traj1, 10, 64, seed 10, final_frac 0.25): chunk 62 is PLAN_OK at the defaults and ends a 2-cycle
    as PLAN_FROZEN_LIMITS under set A (the oracle's freeze of the speed limits; no chunk is PLAN_NUMERICAL).  The
    host backend equals the oracle on the whole batch bit for bit."""
    mpcplan, PO, PR, W = env
    r = W.plan_route("traj1")
    ps = PP.pset("A")
    wb = PP.batch(W, r, 10, ps)
    ref = PO.PlanOracle(r).solve_batch(PP.lib_params(PO, ps, N=10), wb["x0"], wb["s_target"], wb["is_final"])
    pl = mpcplan.Planner(r, PP.lib_params(mpcplan, ps, N=10), device=-1)
    got = pl.solve_chunks(wb["x0"], wb["s_target"], wb["is_final"])
    pl.close()
    print(f"set A traj1 N=10: statuses {PP.counts(ref['status'])}")
    assert ref["status"][62] == mpcplan.PLAN_FROZEN_LIMITS and (ref["status"] != mpcplan.PLAN_NUMERICAL).all()
    for k in PP.OUTPUTS:
        assert np.array_equal(got[k], ref[k]), k


def test_set_params_on_a_host_context(env):
    """A context created with the defaults and then given set A equals a context created with set A, bit for bit;
    setting the defaults back restores the default results."""
    mpcplan, PO, PR, W = env
    check_set_params(mpcplan, W, -1)


def check_set_params(mpcplan, W, device):
    r = W.plan_route("synth1")
    ps = PP.pset("A")
    x0, st, fin, N = PP.mixed_batch(W, r, ps)
    Nm = int(N.max())
    pl = mpcplan.Planner(r, mpcplan.default_params(N=Nm), device=device)
    d0 = pl.solve_chunks(x0, st, fin, N)
    pl.set_params(PP.lib_params(mpcplan, ps, N=Nm))
    a1 = pl.solve_chunks(x0, st, fin, N)
    ev1 = PC.evaluate(pl, PC.pack(list(PP.ev_cases("A"))))
    pl.set_params(mpcplan.default_params(N=Nm))
    d1 = pl.solve_chunks(x0, st, fin, N)
    pl.close()
    pa = mpcplan.Planner(r, PP.lib_params(mpcplan, ps, N=Nm), device=device)
    a0 = pa.solve_chunks(x0, st, fin, N)
    ev0 = PC.evaluate(pa, PC.pack(list(PP.ev_cases("A"))))
    pa.close()
    for k in PP.OUTPUTS:
        assert np.array_equal(a1[k], a0[k]), k
        assert np.array_equal(d1[k], d0[k]), k
    for k in ev0:
        assert PC.same(ev1[k], ev0[k]), k
    assert not np.array_equal(a0["X"], d0["X"])


# ---------------------------------------------------------------------------------------------
# the evaluator
# ---------------------------------------------------------------------------------------------
def test_evaluator_seed_needs_at_most_a_handful_of_redraws():
    for name in PP.EV_SETS:
        cs = PP.ev_cases(name)
        assert len(cs) == 10 and [c["N"] for c in cs[::2]] == list(PP.EV_HORIZONS)
        assert sum(c["redraws"] for c in cs) <= PC.REDRAWS_MAX, (name, [c["redraws"] for c in cs])


@pytest.mark.parametrize("name", PP.EV_SETS)
def test_host_evaluator_against_plan_ref(env, name):
    mpcplan, PO, PR, W = env
    cs = list(PP.ev_cases(name))
    pl = mpcplan.Planner(W.plan_route(PP.EV_ROUTE), PP.lib_params(mpcplan, PP.pset(name), N=20), device=-1)
    out = PC.evaluate(pl, PC.pack(cs))
    pl.close()
    ed, er, es = PC.errors_against_ref(cs, out)
    print(f"set {name}: host evaluator against plan_ref: defects {ed:.17g} (bound {PP.TOL_DEFECTS:.3e}), rows {er:.17g} "
          f"(bound {PP.TOL_ROWS:.3e}), sums {es:.17g} (bound {PP.TOL_SUMS:.3e})")
    assert ed <= PP.TOL_DEFECTS
    assert er <= PP.TOL_ROWS
    assert es <= PP.TOL_SUMS
    # the set is felt: the same inputs under the defaults give other rows or another cost
    pd = mpcplan.Planner(W.plan_route(PP.EV_ROUTE), mpcplan.default_params(N=20), device=-1)
    od = PC.evaluate(pd, PC.pack(cs))
    pd.close()
    assert not (PC.same(od["rows"], out["rows"]) and PC.same(od["summary"], out["summary"]) and
                PC.same(od["defects"], out["defects"]))


# ---------------------------------------------------------------------------------------------
# the drop-in and the loop
# ---------------------------------------------------------------------------------------------
def test_dropin_params_and_optimize_under_set_A(env):
    """A TrajectoryOptimizer whose attributes are set A's gives params() equal to the set field for field, and its
    optimize on the host backend equals the oracle under the set bit for bit."""
    mpcplan, PO, PR, W = env
    import trajectory_planning as TP
    ps = PP.pset("A")
    r = W.plan_route("synth1")
    opt = PP.loop_optimizer(TP, ps, -1)
    opt.N, opt.T = 16, 16 * ps["dt"]
    assert PP.fields(opt.params()) == PP.fields(PP.lib_params(mpcplan, ps))
    assert PP.fields(opt.params(0.5)) == PP.fields(PP.lib_params(mpcplan, dict(ps, v_min=0.5)))
    x0, st, fin, _ = PP.mixed_batch(W, r, ps, n=8)
    orc = PO.PlanOracle(r)
    p = PP.lib_params(PO, ps, N=16, sqp_iters=TP.SQP_ITERS)
    for b in range(8):
        X, U, S = opt.optimize(x0[b], st[b], r.s_total, r.k_ref_fun, lambda s: 0, r.v_max_fun, bool(fin[b]))
        o = orc.solve_batch(p, x0[b][None], st[b], int(fin[b]))
        assert np.array_equal(X, o["X"][0]) and np.array_equal(U, o["U"][0]) and np.array_equal(S, o["S"][0]), b
        assert opt.last_status == o["status"][0]
    TP.release_planners()


def check_optimize_loop(mpcplan, PO, W, device):
    """plan_optimize under set A (three starts on synth1) gives the plans of the package loop driven by the oracle
    under set A: identical on the host backend, within `tol` of test_gpu_plan.py on the device.  The horizon rule
    divides by the set's dt (trajectory_planning._loop_dt), so the horizons are not the default loop's."""
    import trajectory_planning as TP
    ps = PP.pset("A")
    r = W.plan_route("synth1")
    orc = PO.PlanOracle(r)

    def solve_chunks(x0, st, fin, N):
        return orc.solve_batch(PP.lib_params(PO, ps, N=int(N.max()), sqp_iters=TP.SQP_ITERS), x0, st, fin, N=N,
                               num_threads=4)

    starts = PP.loop_starts(r)
    ref, qref = TP.optimize_full_trajectory_batch(r, starts, solve_chunks=solve_chunks,
                                                  optimizer=PP.loop_optimizer(TP, ps, device))
    got, qgot = TP.optimize_full_trajectory_batch(r, starts, optimizer=PP.loop_optimizer(TP, ps, device))
    # the first chunk's horizon by the reference's rule (:507-515) at the set's dt, not at 0.3
    first = 20.0 / r.avg_speed_from(0.0) * 2.0
    assert qref[0]["horizons"][0] == int(np.ceil(first / ps["dt"])) > int(np.ceil(first / 0.3))
    print(f"set A loop: chunks {[len(q['statuses']) for q in qgot]}, horizons {min(map(min, (q['horizons'] for q in qref)))}-"
          f"{max(map(max, (q['horizons'] for q in qref)))} (at dt 0.3 the first would be {int(np.ceil(first / 0.3))}), "
          f"statuses {PP.counts(np.concatenate([q['statuses'] for q in qref]))}")
    return ref, qref, got, qgot


def test_host_optimize_loop_equals_oracle_loop_under_set_A(env):
    mpcplan, PO, PR, W = env
    ref, qref, got, qgot = check_optimize_loop(mpcplan, PO, W, -1)
    for b in range(3):
        for a, c in zip(got[b], ref[b]):
            assert np.array_equal(a, c), b
        assert qgot[b]["statuses"] == qref[b]["statuses"] and qgot[b]["horizons"] == qref[b]["horizons"], b
        assert abs(got[b][0][-1, 0] - W.plan_route("synth1").s_total) < 1e-6
    # an optimizer and a device argument that names another device are refused
    import trajectory_planning as TP
    with pytest.raises(ValueError):
        TP.optimize_full_trajectory_batch(W.plan_route("synth1"), PP.loop_starts(W.plan_route("synth1")), device=0,
                                          optimizer=PP.loop_optimizer(TP, PP.pset("A"), -1))


# ---------------------------------------------------------------------------------------------
# the kernel's source on the CPU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tools/plan_emu.cpp built once: (the driver module, the executable)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import plan_emu
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    exe = str(tmp_path_factory.mktemp("emu") / "plan_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", plan_emu.SRC, "-o", exe, "-lpthread"])
    return plan_emu, exe


def emulate_and_compare(emu, PO, label, r, p, x0, st, fin):
    """The chunks through the emulated kernel and the oracle: statuses equal, plans within 1e-8 (compare()'s bound)."""
    plan_emu, exe = emu
    g = plan_emu.run(exe, r, p, x0, st, fin)
    o = PO.PlanOracle(r).solve_batch(p, x0, st, fin)
    both = np.isin(g["status"], (0, 4)) & np.isin(o["status"], (0, 4))
    err = max(float(np.abs(g[k][both] - o[k][both]).max()) for k in ("X", "U", "S")) if both.any() else np.nan
    print(f"emulated kernel, {label}: statuses {g['status'].tolist()}, oracle {o['status'].tolist()}, max err {err:.1e}")
    assert np.array_equal(g["status"], o["status"]), label
    assert both.sum() >= 0.75 * len(st), label
    assert err <= 1e-8, label


@pytest.mark.parametrize("name,count", [("A", 8), ("S", 2)])
def test_emulated_kernel_against_the_oracle(env, emu, name, count):
    """tools/plan_emu.cpp compiles csrc/plan_kernel.h for the host (64 threads per chunk); its input carries the
    whole plan_params.  8 chunks of N = 10 under set A against the oracle: statuses equal, plans within 1e-8 (the
    device comparison's bound), so a parameter misread in the kernel has a CPU reproduction.  Intermediate chunks:
    64 threads meet at a barrier for every shuffle, ~3 s per converging chunk, and a final chunk of N = 10 that ends
    PLAN_QP_FAILED after 100 interior-point iterations takes 30 s.  And 2 chunks under set S: set A keeps
    defect_sign = +1, under which a kernel that drops the sign from its defect values and Jacobians (interval_jac) is
    still right.  No lateral-acceleration or curvature row is active on these chunks (margins above 1.5 and 0.5):
    that group is test_emulated_kernel_on_chunks_with_an_active_lateral_row's."""
    mpcplan, PO, PR, W = env
    ps = PP.pset(name)
    r = W.plan_route("synth1")
    wb = W.plan_batch(r, 10, count, seed=10, final_frac=0.0)
    emulate_and_compare(emu, PO, f"set {name}", r, PP.lib_params(PO, ps, N=10), wb["x0"], wb["s_target"], wb["is_final"])


@pytest.mark.parametrize("name,N,route", [("G", 20, "traj2")])
def test_emulated_kernel_on_chunks_with_an_active_lateral_row(env, emu, name, N, route):
    """The first two intermediate chunks of the GPU comparison's batch that the oracle converges on with a
    lateral-acceleration row active at its optimum (a_max - |k| v^2 <= 1e-6 at some stage): there a_max decides the
    plan, so a literal in its place in the kernel's row values keeps the first chunk from converging (error 0.1)
    where on chunks without an active row it only moves the interior point's path.  G names the group.  (The same
    under set A on traj1, chunks 18 and 21, fails with that literal too, but chunk 18 takes 30 QPs: two minutes here.)"""
    mpcplan, PO, PR, W = env
    ps = PP.pset(name)
    r = W.plan_route(route)
    wb = PP.batch(W, r, N, ps)
    p = PP.lib_params(PO, ps, N=N)
    o = PO.PlanOracle(r).solve_batch(p, wb["x0"], wb["s_target"], wb["is_final"], num_threads=4)
    lat, _ = PP.active_rows(o, p)
    pick = np.flatnonzero(lat & (o["status"] == 0) & (wb["is_final"] == 0))[:2]
    print(f"set {name} N={N} {route}: chunks with an active lateral row {np.flatnonzero(lat).tolist()}, emulated {pick.tolist()}")
    assert len(pick) == 2
    emulate_and_compare(emu, PO, f"set {name} {route} chunks {pick.tolist()}", r, p, wb["x0"][pick], wb["s_target"][pick],
                        wb["is_final"][pick])


# ---------------------------------------------------------------------------------------------
# the condition the GPU comparisons rest on
# ---------------------------------------------------------------------------------------------
def test_oracle_converges_on_at_least_half_of_every_gpu_batch(env):
    mpcplan, PO, PR, W = env
    for name, N, rt in PP.GPU_CASES + (("A", 10, "traj1"),):
        r = W.plan_route(rt)
        ps = PP.pset(name)
        wb = PP.batch(W, r, N, ps)
        o = PO.PlanOracle(r).solve_batch(PP.lib_params(PO, ps, N=N), wb["x0"], wb["s_target"], wb["is_final"],
                                         num_threads=4)
        print(f"set {name} N={N} {rt}: oracle statuses {PP.counts(o['status'])}")
        assert np.isin(o["status"], (0, 4)).sum() >= 32, (name, N, rt)
    r = W.plan_route("synth1")
    for name in ("A", "GK"):
        x0, st, fin, N = PP.order_batch(W, r)
        o = PO.PlanOracle(r).solve_batch(PP.lib_params(PO, PP.pset(name), N=24), x0, st, fin, N=N, num_threads=4)
        print(f"set {name} order batch: oracle statuses {PP.counts(o['status'])}")
        assert np.isin(o["status"], (0, 4)).sum() >= 80, name
    for name, N in (("A", 26), ("B", 16)):
        x0, st, fin, Nv = PP.mixed_batch(W, r, PP.pset(name), n=64 if name == "B" else 48)
        Nv = Nv if name == "A" else np.full(64, 16, np.int32)
        o = PO.PlanOracle(r).solve_batch(PP.lib_params(PO, PP.pset(name), N=N), x0, st, fin, N=Nv, num_threads=4)
        print(f"set {name} mixed batch: oracle statuses {PP.counts(o['status'])}")
        assert np.isin(o["status"], (0, 4)).mean() >= 0.5, name
