"""Shared pieces of the planner evaluator's tests (test_plan_evaluate_cpu.py on the host backend,
test_gpu_plan_evaluate.py on the device): seeded evaluation inputs, their reference values under oracle/plan_ref.py
(the numpy restatement of the reference NLP) re-indexed into plan_evaluate_chunks' layout, and the tolerances.

Inputs.  Per route ('traj2', 'synth1') 12 chunks: the horizons N in {1, 2, 63, 64, 65, 130} (one and two stages, both
sides of the 64-stage pass of the kernel, and three passes), each as an intermediate and as a final chunk, posed like
workloads.plan_batch poses them.  z is the reference's initial guess (plan_ref.Chunk.z_init) plus normal
perturbations, sigma 0.05 on X, 0.3 on U, and S = |N(0, 0.05)|: no solver output, whose active rows sit at +-1e-12
and would make N_NEG / ARGMIN_* a coin toss.  A draw is rejected and redrawn when, under plan_ref, a row has
|g| < 1e-6, the two smallest rows are closer than 1e-6, a stage's s_k (or an interval's midpoint s) lies within 1e-6
of a route way-point (v_max_fun is a step there, and the curvature's spline piece changes), or |1 - d kappa| < 1e-3
at a dynamics evaluation (the guard_den branch).  So no case is left out of any comparison.  The committed seed needs
no redraw on either route (REDRAWS_MAX below; test_plan_evaluate_cpu.py asserts it).

Tolerances: measured, not chosen (the tests print every figure before they assert it).  The largest
absolute error of the host backend against plan_ref over these 24 cases, measured on the CPU:
    defects                         1.8e-15   (MEASURED_DEFECTS)
    rows                            8.9e-16   (MEASURED_ROWS)
    COST, L1_EQ, L1_INEQ, MIN_ROW   8.8e-16   (MEASURED_SUMS, relative to 1 + |ref|; MAX_DEFECT and X0_RES are held to
                                              the same bound)
The CPU test's bound is 8 x the figure (scipy's spline evaluation and the library's agree to 1e-10 relative in kappa,
test_route_functions_match_scipy, and another case set may land less favourably); the GPU test's device-against-host
bound is the same 8 x figure again (the device's sin / cos and nothing else differ, a few ulp at |s| <= 3000 m).
The end-to-end MAX_DEFECT bound is 10 x the largest MAX_DEFECT of the CPU oracle's converged solutions
(plan_oracle.solve_batch) of the same batch through the host evaluator (the device's and the oracle's plans differ
by <= 1e-12)."""
import numpy as np

HORIZONS = (1, 2, 63, 64, 65, 130)
ROUTES = ("traj2", "synth1")
SEED = 2024
DT = 0.3
REDRAWS_MAX = 4                   # "a handful"; the committed seed needs 0 on traj2 and 0 on synth1

# measured on the CPU, host backend against plan_ref over the 24 cases (see the module docstring)
MEASURED_DEFECTS = 1.7763568394002505e-15      # traj2 (synth1: 8.3e-17)
MEASURED_ROWS = 8.881784197001252e-16          # synth1 (traj2: 0)
MEASURED_SUMS = 8.814303220864607e-16          # synth1 (traj2: 7.8e-16)
MARGIN = 8.0
TOL_DEFECTS = MARGIN * MEASURED_DEFECTS
TOL_ROWS = MARGIN * MEASURED_ROWS
TOL_SUMS = MARGIN * MEASURED_SUMS
# end to end: W.plan_batch(traj1, N = 20, B = 64, seed = 20, final_frac = 0.25); the largest MAX_DEFECT of the
# oracle's PLAN_OK solutions through the host evaluator, and the 10 x bound on the device's
MEASURED_E2E_MAX_DEFECT = 3.979039320256561e-13   # 57 of the 64 chunks are PLAN_OK
E2E_MAX_DEFECT = 10.0 * MEASURED_E2E_MAX_DEFECT

_cache = {}


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def ref_rows(ch, z):
    """plan_ref.Chunk.ineq re-indexed to [N+1, 12] (columns PLAN_EVR_*), NaN where the reference has no row."""
    N = ch.N
    g = np.asarray(ch.ineq(z), np.float64)
    out = np.full((N + 1, 12), np.nan)
    o = 0
    if not ch.final:
        out[N, 11] = g[0]
        o = 1
    out[:, 0:4] = g[o:o + 4 * (N + 1)].reshape(N + 1, 4)
    o += 4 * (N + 1)
    out[:, 4:6] = g[o:o + 2 * (N + 1)].reshape(N + 1, 2)
    o += 2 * (N + 1)
    out[:N, 6:11] = g[o:o + 5 * N].reshape(N, 5)
    assert o + 5 * N == g.size
    return out


def _acceptable(ch, X, U, rows):
    """The acceptance rule of the module docstring, at the chunk's own dt."""
    r = np.sort(rows[~np.isnan(rows)])
    if np.abs(r).min() < 1e-6 or r[1] - r[0] < 1e-6:
        return False
    way = ch.r.s
    for k in range(ch.N + 1):
        pts = [X[k]]
        if k < ch.N:
            import plan_ref as PR
            f0 = PR.dyn(X[k], U[k], ch.r.k_ref_fun(X[k, 0]))
            f1 = PR.dyn(X[k + 1], U[k], ch.r.k_ref_fun(X[k + 1, 0]))
            pts.append(0.5 * (X[k] + X[k + 1]) + ch.dt / 8 * (f0 - f1))
        for x in pts:
            if np.abs(way - x[0]).min() < 1e-6 or abs(1.0 - x[1] * ch.r.k_ref_fun(x[0])) < 1e-3:
                return False
    return True


def _make(route, N, final, rng, dt=DT, params=None):
    """One case; dt and params (plan_ref.Params, None: the defaults) state the NLP it is evaluated under
    (tests/plan_params_cases.py regenerates the cases under its parameter sets)."""
    import plan_ref as PR
    redraws = 0
    while True:
        D = N * dt * route.avg_speed_from(0.5 * route.s_total) / 2.0
        if final:
            s0, target = route.s_total - D, route.s_total
            vcap = min(route.v_max_fun(s0), np.sqrt(2.0 * 2.5 * D))
        else:
            s0 = rng.uniform(1.0, route.s_total - D - 2.0)
            target = s0 + D
            vcap = route.v_max_fun(s0)
        x0 = np.array([s0, rng.normal(0, 0.05), rng.normal(0, 0.01), route.k_ref_fun(s0), rng.uniform(0.2, 0.9) * vcap])
        ch = PR.Chunk(route, N, dt, x0, target, bool(final), params)
        X, U, S = ch.unpack(ch.z_init())
        X = X + rng.normal(0, 0.05, X.shape)
        U = U + rng.normal(0, 0.3, U.shape)
        S = np.abs(rng.normal(0, 0.05, S.shape))
        z = np.concatenate([X.ravel(), U.ravel(), S])
        rows = ref_rows(ch, z)
        if _acceptable(ch, X, U, rows):
            break
        redraws += 1
        assert redraws <= 50, "the generator does not terminate"
    eq = np.asarray(ch.eq(z), np.float64)
    flat = rows.ravel()
    arg = int(np.nanargmin(flat))
    c = dict(N=N, final=int(final), x0=x0, st=float(target), X=X, U=U, S=S, redraws=redraws, rows=rows,
             defects=eq[:5 * N].reshape(N, 5), cost=float(ch.cost(z)), l1_eq=float(np.abs(eq).sum()),
             l1_ineq=float(np.maximum(-flat[~np.isnan(flat)], 0.0).sum()), min_row=float(flat[arg]),
             argmin_stage=arg // 12, argmin_kind=arg % 12, n_neg=int((flat < 0).sum()),
             max_defect=float(np.abs(eq[:5 * N]).max()), x0_res=float(np.abs(X[0] - x0).max()))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def cases(route_name):
    """The 12 cases of a route (computed once per process, read-only): horizon-major, intermediate then final."""
    if route_name not in _cache:
        import workloads as W
        route = W.plan_route(route_name)
        rng = np.random.default_rng([SEED, ROUTES.index(route_name)])
        _cache[route_name] = [_make(route, N, fin, rng) for N in HORIZONS for fin in (0, 1)]
    return _cache[route_name]


def pack(cs, Nmax=None, pad=7.0, with_S=True):
    """Cases -> plan_evaluate_chunks' arrays at row stride Nmax (default: the largest N); entries past a chunk's
    horizon hold `pad` (the evaluator must not read them)."""
    B = len(cs)
    Nmax = max(c["N"] for c in cs) if Nmax is None else Nmax
    X = np.full((B, Nmax + 1, 5), pad)
    U = np.full((B, Nmax, 2), pad)
    S = np.full((B, Nmax), pad)
    for b, c in enumerate(cs):
        N = c["N"]
        X[b, :N + 1], U[b, :N], S[b, :N] = c["X"], c["U"], c["S"]
    return dict(x0=np.array([c["x0"] for c in cs]), s_target=np.array([c["st"] for c in cs]),
                is_final=np.array([c["final"] for c in cs], np.int32), N=np.array([c["N"] for c in cs], np.int32),
                X=X, U=U, S=S if with_S else None, Nmax=Nmax)


def evaluate(pl, a, **kw):
    return pl.evaluate_chunks(a["x0"], a["s_target"], a["is_final"], a["X"], a["U"], a["S"], N=a["N"], **kw)


def errors_against_ref(cs, out):
    """(defects, rows, sums) largest errors of an evaluation of `cs` against plan_ref; asserts the exact parts:
    the NaN pattern of rows / defects, N_NEG, ARGMIN_*."""
    import mpcplan
    Q = mpcplan.EVQ
    ed = er = es = 0.0
    for b, c in enumerate(cs):
        N = c["N"]
        d, r, q = out["defects"][b], out["rows"][b], out["summary"][b]
        assert not np.isnan(d[:N]).any() and np.isnan(d[N:]).all(), (b, N)
        assert same(np.isnan(r[:N + 1]), np.isnan(c["rows"])) and np.isnan(r[N + 1:]).all(), (b, N)
        ed = max(ed, float(np.abs(d[:N] - c["defects"]).max()))
        er = max(er, float(np.nanmax(np.abs(r[:N + 1] - c["rows"]))))
        for col, key in (("cost", "cost"), ("l1_eq", "l1_eq"), ("l1_ineq", "l1_ineq"), ("min_row", "min_row"),
                         ("max_defect", "max_defect"), ("x0_res", "x0_res")):
            es = max(es, abs(q[Q[col]] - c[key]) / (1.0 + abs(c[key])))
        assert q[Q["n_neg"]] == c["n_neg"], (b, N, q[Q["n_neg"]], c["n_neg"])
        assert (q[Q["argmin_stage"]], q[Q["argmin_kind"]]) == (c["argmin_stage"], c["argmin_kind"]), (b, N)
        if c["final"]:
            assert q[Q["term_s"]] == c["X"][N, 0] - c["st"] and q[Q["term_v"]] == c["X"][N, 4]
        else:
            assert np.isnan(q[Q["term_s"]]) and np.isnan(q[Q["term_v"]])
    return ed, er, es


# the summary columns that are pure comparisons or copies of inputs: equal bit for bit on every backend
EXACT_COLUMNS = ("x0_res", "term_s", "term_v", "min_row", "argmin_stage", "argmin_kind", "l1_ineq", "n_neg", "s_final",
                 "s_total", "v_final", "min_v", "max_abs_d", "max_abs_slack", "u1_min", "u1_max", "u2_min", "u2_max")
ARITH_COLUMNS = ("cost", "max_defect", "l1_eq")
