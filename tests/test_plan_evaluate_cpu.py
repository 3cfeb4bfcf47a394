"""The planner's evaluator (plan_evaluate_chunks, plan_check_verdicts; include/mpcplan_evaluate.h) on the host backend
(device = -1) against the numpy restatement of the reference NLP (oracle/plan_ref.py) and against
sanity_checks.plan_check_summary.  Cases, reference values and the measured tolerances: tests/plan_evaluate_cases.py.

The check columns on the 14 plancheck goldens: each golden trajectory is evaluated as one final chunk on a straight
three-point route built with the golden's own s_total (cumulative chord length L/2 + L/2 = L, exact), so S_TOTAL is
the golden's and error_s is compared through the context's route; no other check column depends on the route."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import plan_evaluate_cases as PC
from conftest import PKG, ROOT, load_golden


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import mpcplan
    import workloads as W
    return mpcplan, W


@pytest.fixture(scope="module")
def planners(env):
    mpcplan, W = env
    pls = {rn: mpcplan.Planner(W.plan_route(rn), mpcplan.default_params(N=20), device=-1) for rn in PC.ROUTES}
    yield pls
    for p in pls.values():
        p.close()


@pytest.fixture(scope="module")
def mixed(planners):
    """The 12 cases of each route in one call with per-chunk N (final and intermediate chunks mixed)."""
    out = {}
    for rn in PC.ROUTES:
        out[rn] = PC.evaluate(planners[rn], PC.pack(PC.cases(rn)))
        for v in out[rn].values():
            v.setflags(write=False)
    return out


def test_committed_seed_needs_at_most_a_handful_of_redraws():
    for rn in PC.ROUTES:
        cs = PC.cases(rn)
        assert len(cs) == 12 and [c["N"] for c in cs[::2]] == list(PC.HORIZONS)
        assert sum(c["redraws"] for c in cs) <= PC.REDRAWS_MAX, [c["redraws"] for c in cs]


@pytest.mark.parametrize("rn", PC.ROUTES)
def test_against_plan_ref(mixed, rn):
    ed, er, es = PC.errors_against_ref(PC.cases(rn), mixed[rn])
    print(f"{rn}: host backend against plan_ref: defects {ed:.3e} (bound {PC.TOL_DEFECTS:.3e}), rows {er:.3e} "
          f"(bound {PC.TOL_ROWS:.3e}), sums {es:.3e} (bound {PC.TOL_SUMS:.3e})")
    assert ed <= PC.TOL_DEFECTS
    assert er <= PC.TOL_ROWS
    assert es <= PC.TOL_SUMS


def test_uniform_horizon_without_N(env, mixed):
    """N = NULL: every chunk has the params' N; the same bits as the per-chunk call."""
    mpcplan, W = env
    for rn in PC.ROUTES:
        idx = [b for b, c in enumerate(PC.cases(rn)) if c["N"] == 63]
        a = PC.pack([PC.cases(rn)[b] for b in idx])
        pl = mpcplan.Planner(W.plan_route(rn), mpcplan.default_params(N=63), device=-1)
        o = pl.evaluate_chunks(a["x0"], a["s_target"], a["is_final"], a["X"], a["U"], a["S"])
        pl.close()
        assert PC.same(o["summary"], mixed[rn]["summary"][idx])
        assert PC.same(o["defects"], mixed[rn]["defects"][idx, :63])
        assert PC.same(o["rows"], mixed[rn]["rows"][idx, :64])


def test_independent_of_B_padding_and_threads(env, planners, mixed):
    mpcplan, W = env
    rn = "synth1"
    cs = PC.cases(rn)
    # one chunk per call, at its own row stride
    for b in (0, 3, 7, 11):
        o = PC.evaluate(planners[rn], PC.pack([cs[b]]))
        N = cs[b]["N"]
        assert PC.same(o["summary"][0], mixed[rn]["summary"][b])
        assert PC.same(o["defects"][0], mixed[rn]["defects"][b, :N])
        assert PC.same(o["rows"][0], mixed[rn]["rows"][b, :N + 1])
    # a wider row stride with other padding, in reverse order
    a = PC.pack(cs[::-1], Nmax=200, pad=np.nan)
    o = PC.evaluate(planners[rn], a)
    assert PC.same(o["summary"][::-1], mixed[rn]["summary"])
    assert PC.same(o["defects"][::-1, :130], mixed[rn]["defects"]) and np.isnan(o["defects"][:, 130:]).all()
    assert PC.same(o["rows"][::-1, :131], mixed[rn]["rows"]) and np.isnan(o["rows"][:, 131:]).all()
    # the worker count (the library reads PLAN_CPU_THREADS when a context is created)
    code = ("import sys, numpy as np; sys.path[:0] = [%r, %r, %r]; import plan_evaluate_cases as PC, mpcplan, workloads as W;"
            "pl = mpcplan.Planner(W.plan_route(%r), mpcplan.default_params(N=20), device=-1);"
            "o = PC.evaluate(pl, PC.pack(PC.cases(%r)));"
            "sys.stdout.buffer.write(o['summary'].tobytes() + o['defects'].tobytes() + o['rows'].tobytes())"
            % (PKG, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), rn, rn))
    want = mixed[rn]["summary"].tobytes() + mixed[rn]["defects"].tobytes() + mixed[rn]["rows"].tobytes()
    for t in ("1", "5"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PLAN_CPU_THREADS=t), capture_output=True)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == want, t


def test_outputs_and_inputs_are_optional(planners, mixed):
    rn = "traj2"
    a = PC.pack(PC.cases(rn))
    for want in (("summary",), ("defects",), ("rows",), ("summary", "rows")):
        o = PC.evaluate(planners[rn], a, want=want)
        assert set(o) == set(want)
        for k in want:
            assert PC.same(o[k], mixed[rn][k]), (want, k)
    assert PC.evaluate(planners[rn], a, want=()) == {}
    # S = NULL is S = 0, is_final = NULL is all intermediate
    z = dict(a, S=np.zeros_like(a["S"]))
    n = dict(a, S=None)
    for k, v in PC.evaluate(planners[rn], z).items():
        assert PC.same(v, PC.evaluate(planners[rn], n)[k]), k
    i0 = dict(a, is_final=np.zeros(12, np.int32))
    i1 = dict(a, is_final=None)
    for k, v in PC.evaluate(planners[rn], i0).items():
        assert PC.same(v, PC.evaluate(planners[rn], i1)[k]), k


def test_device_pointer_entry_on_a_host_context_takes_host_pointers(env, planners, mixed):
    mpcplan, W = env
    rn = "traj2"
    a = PC.pack(PC.cases(rn))
    q = np.full((12, mpcplan.PLAN_EV_NQ), -1.0)
    d = np.full((12, a["Nmax"], 5), -1.0)
    r = np.full((12, a["Nmax"] + 1, 12), -1.0)
    planners[rn].evaluate_chunks_device(12, a["Nmax"], a["N"].ctypes.data, a["x0"].ctypes.data, a["s_target"].ctypes.data,
                                        a["is_final"].ctypes.data, a["X"].ctypes.data, a["U"].ctypes.data,
                                        a["S"].ctypes.data, q.ctypes.data, d.ctypes.data, r.ctypes.data)
    assert PC.same(q, mixed[rn]["summary"]) and PC.same(d, mixed[rn]["defects"]) and PC.same(r, mixed[rn]["rows"])


def test_out_of_range_horizon_and_misuse(env, planners):
    mpcplan, W = env
    rn = "traj2"
    pl = planners[rn]
    cs = PC.cases(rn)[:4]
    a = PC.pack(cs, Nmax=4)
    a["N"] = np.array([1, 0, 5, 2], np.int32)          # chunks 1 and 2 out of [1, Nmax]
    o = PC.evaluate(pl, a)
    assert np.isnan(o["summary"][[1, 2]]).all() and not np.isnan(o["summary"][[0, 3]][:, 0]).any()
    assert np.isnan(o["rows"][[1, 2]]).all() and np.isnan(o["defects"][[1, 2]]).all()      # nothing written
    L = mpcplan.lib()
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    q = np.zeros((4, mpcplan.PLAN_EV_NQ))
    Nv = np.array([1, 1, 2, 2], np.int32)
    args = lambda **kw: [kw.get("h", pl.h), kw.get("B", 4), kw.get("Nmax", 4), Nv.ctypes.data_as(C.POINTER(C.c_int)),
                         kw.get("x0", dp(a["x0"])),
                         dp(a["s_target"]), None, kw.get("X", dp(a["X"])), dp(a["U"]), None, dp(q), None, None]
    assert L.plan_evaluate_chunks(*args()) == 0
    assert L.plan_evaluate_chunks(*args(B=0)) == 0
    for bad in (dict(h=None), dict(B=-1), dict(Nmax=0), dict(x0=None), dict(X=None)):
        assert L.plan_evaluate_chunks(*args(**bad)) == -1, bad          # PLAN_E_ARG
        assert mpcplan.last_error()
    # N NULL and Nmax below the params' N (20)
    big = PC.pack(cs, Nmax=19)
    assert L.plan_evaluate_chunks(pl.h, 4, 19, None, dp(big["x0"]), dp(big["s_target"]), None, dp(big["X"]), dp(big["U"]),
                                  None, dp(q), None, None) == -1
    assert L.plan_check_verdicts(None, 1, dp(q), None, None) == -1
    assert L.plan_check_verdicts(pl.h, 1, None, None, None) == -1
    assert L.plan_check_verdicts(pl.h, 0, None, None, None) == 0


def test_nan_inputs_follow_numpy(planners):
    rn = "synth1"
    cs = PC.cases(rn)
    a = PC.pack([cs[4]])                # N = 63, intermediate
    a["X"][0, 10, 4] = np.nan           # v of stage 10
    a["U"][0, 3, 0] = np.nan
    import mpcplan
    Q = mpcplan.EVQ
    o = PC.evaluate(planners[rn], a)
    q = o["summary"][0]
    for col in ("min_v", "u1_min", "u1_max", "min_row", "max_defect", "l1_eq", "l1_ineq", "cost"):
        assert np.isnan(q[Q[col]]), col
    for col in ("u2_min", "u2_max", "max_abs_slack", "max_abs_d", "s_final"):
        assert not np.isnan(q[Q[col]]), col
    # np.argmin: the first NaN row in (stage, column) order, u1 - u_min[0] of stage 3
    assert (q[Q["argmin_stage"]], q[Q["argmin_kind"]]) == (3, 6)
    assert np.isnan(o["rows"][0, 3, 6:8]).all() and np.isnan(o["rows"][0, 10, :4]).all()
    assert np.isnan(o["defects"][0, 3]).any() and not np.isnan(o["defects"][0, 20:63]).any()


def test_check_columns_and_verdicts_on_the_goldens(env):
    mpcplan, W = env
    import routes
    import sanity_checks as SC
    g = load_golden("plancheck_golden")
    names = [str(n) for n in g["names"]]
    assert len(names) == 14
    Q = mpcplan.EVQ
    p = mpcplan.default_params()
    u_min, u_max = list(p.u_min), list(p.u_max)
    for n in names:
        X, U, S, L = g[f"{n}_X"], np.asarray(g[f"{n}_U"]).reshape(-1, 2), np.asarray(g[f"{n}_S"]).ravel(), float(g[f"{n}_s_total"])
        route = routes.Route([(0.0, 0.0), (L / 2, 0.0), (L, 0.0)], [10.0, 10.0, 10.0])
        assert route.s_total == L
        ref = SC.plan_check_summary(u_min, u_max, X, U, S, L)
        N = len(U)
        assert X.shape[0] == N + 1 and S.size == N, n
        pl = mpcplan.Planner(route, p, device=-1)
        q = pl.evaluate_chunks(X[0], L, 1, X[None], U[None], S[None], N=N, want=("summary",))["summary"]
        v = pl.check_verdicts(q)
        pl.close()
        q = q[0]
        assert abs(q[Q["s_final"]] - q[Q["s_total"]]) == ref["error_s"], n
        assert q[Q["v_final"]] == ref["v_final"] and q[Q["min_v"]] == ref["min_v"], n
        assert q[Q["max_abs_d"]] == ref["max_lat_dev"] and q[Q["max_abs_slack"]] == ref["max_slack"], n
        assert (q[Q["u1_min"]], q[Q["u1_max"]]) == (U[:, 0].min(), U[:, 0].max()), n
        assert (q[Q["u2_min"]], q[Q["u2_max"]]) == (U[:, 1].min(), U[:, 1].max()), n
        for k, name in enumerate(mpcplan.CHECK_NAMES):
            assert bool(v[name][0]) == bool(ref[name]), (n, name)
            assert v["counts"][k] == int(bool(ref[name])), (n, name)
        assert bool(v["passed"][0]) == ("===> Checks passed : True" in str(g[f"{n}_text"])), n


def test_committed_trajectories_obey_the_forward_rule(env):
    """The k and v components of the Hermite-Simpson defect of the three committed trajectories are <= 1e-7 (the
    bound of tests/test_plan_oracle.py), each evaluated as one final chunk of 1000 to 3000 intervals; and
    trajectory_planning.evaluate_plan reports the same summary."""
    mpcplan, W = env
    import trajectory_planning as TP
    for i in (1, 2, 3):
        route = W.plan_route(f"traj{i}")
        X, U = W.loader(i).X_ref, W.loader(i).U_ref
        N = len(U)
        assert N > mpcplan.PLAN_MAX_N
        pl = mpcplan.Planner(route, device=-1)
        o = pl.evaluate_chunks(X[0], route.s_total, 1, X[None, :N + 1], U[None], None, N=N, want=("summary", "defects"))
        pl.close()
        assert np.abs(o["defects"][0][:, 3:]).max() <= 1e-7, i
        e = TP.evaluate_plan(route, X[:N + 1], U, device=-1)
        assert PC.same([e[k] for k in mpcplan.EV_SUMMARY_NAMES], o["summary"][0])
        assert e["x0_res"] == 0.0 and isinstance(e["passed"], bool)
