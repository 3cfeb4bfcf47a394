"""Shared pieces of the Hessian-vector tests (test_hessvec_cpu.py on the host backend, test_gpu_hessvec.py on the
device): mpc_hessvec_batch against an independent restatement of the reference's dynamics / predict / cost /
constraints that carries every state's dense first and second derivatives in U, against central differences of
mpc_gradient_batch, its structure (symmetry, J against unit-lam jtl, curv and the summary against numpy on the
returned arrays), its independence of the other directions and of the batch, and the argument contract.

Tolerance of the restatement pin (RESTATE_BOUND).  restate() below, run in float64, was compared with itself run in
np.longdouble (x87 80-bit) on the 60 model_golden cases with the seeded lam of gradient_cases.golden_lam(), per case and
per output (the dense Hessian in both modes, the dense row Jacobian) as max |f64 - longdouble| / max(1, max |longdouble|):
    measured worst  1.741e-15, kept as RESTATE_F64_WORST = 1.75e-15 (test_restatement_error_budget re-measures it and
                    holds it to that)
    chosen bound    RESTATE_BOUND = 16 * RESTATE_F64_WORST = 2.8e-14
16x because the library adds in another order (a forward and a reverse chain per direction) than the restatement (dense
forward mode of second order).  HV, JV and curv of the library are held to it with the same error measure.

Finite differences.  A case is smooth when every rolled-out s of both shifted rollouts stays KNOT_MARGIN from a table
knot and the safe distance stays KNOT_MARGIN from its kink (gradient_cases.smooth_case on the evaluator's Xpred at
U + hV and U - hV).  The batch is the 60 golden cases; at most one in ten (6) may be skipped, which the test asserts.

env: dict(mpcqp=module, device=-1 or 0, ptr=callable) as in evaluate_cases.py."""
import ctypes as C
import warnings

import numpy as np

import evaluate_cases as EC
import gradient_cases as GC

RESTATE_F64_MEASURED = 1.741e-15
RESTATE_F64_WORST = 1.75e-15
RESTATE_BOUND = 16 * RESTATE_F64_WORST

same = EC.same
solver = EC.solver
close_solvers = EC.close_solvers
rel_err = GC.rel_err
OUT_KEYS = ("HV", "JV", "curv", "summary")
MODES = ("exact", "gauss_newton")


# ---------------------------------------------------------------------------------------------
# the restatement: dense forward mode of second order through the Euler steps, in any dtype
# ---------------------------------------------------------------------------------------------
def restate(traj, x0, U, obs, lam, dtype, m=None):
    """H [2N,2N] of cost - lam . g in U (exact), Hgn [2N,2N] of the cost with the second-order dynamics term dropped,
    and J [N,7+M,2N] of the rows of one instance, written from the reference's dynamics / predict / cost / constraints:
    every state carries its dense Jacobian and Hessian in U through the Euler steps; the table's values and slopes come
    from the trajectory arrays by np.searchsorted."""
    T = dtype
    m = GC.default_model() if m is None else m
    c = {k: T(v) for k, v in m.items()}
    s64, X64 = GC._table(traj)
    sv, tab = s64.astype(T), X64.astype(T)
    smax = sv[-1]
    N, M = U.shape[0], obs.shape[0]
    nv = 2 * N
    U, obs, lam = U.astype(T), obs.astype(T), lam.astype(T)

    def look(s):
        if s >= smax:
            return tab[-1], np.zeros(5, T)
        i = min(max(int(np.searchsorted(sv, s)), 1), len(sv) - 1)
        slope = (tab[i] - tab[i - 1]) / (sv[i] - sv[i - 1])
        return slope * (s - sv[i - 1]) + tab[i - 1], slope

    sym = lambda a, b: np.outer(a, b) + np.outer(b, a)
    x = np.asarray(x0).astype(T)
    J = np.zeros((5, nv), T)
    K = np.zeros((5, nv, nv), T)                 # the states' Hessians (exact); the Gauss-Newton run keeps them zero
    H, Hgn = np.zeros((nv, nv), T), np.zeros((nv, nv), T)
    Jr = np.zeros((N, 7 + M, nv), T)
    for k in range(N):
        ref, sl = look(x[0])
        _, d, o, kk, v = x
        w, Jw, Kw = kk - ref[3], J[3] - sl[3] * J[0], K[3] - sl[3] * K[0]
        xd = np.array([v, v * o, v * w, U[k, 0], U[k, 1]], T)
        Jd = np.zeros((5, nv), T)
        Kd = np.zeros((5, nv, nv), T)
        Jd[0], Kd[0] = J[4], K[4]
        Jd[1], Kd[1] = J[4] * o + v * J[2], K[4] * o + v * K[2] + sym(J[4], J[2])
        Jd[2], Kd[2] = J[4] * w + v * Jw, K[4] * w + v * Kw + sym(J[4], Jw)
        Jd[3, 2 * k] = 1
        Jd[4, 2 * k + 1] = 1
        x = x + c["dt"] * xd
        J = J + c["dt"] * Jd
        K = K + c["dt"] * Kd
        s, d, o, _, v = x
        ref, sl = look(s)
        for wt, a in ((c["w_d"], 1), (c["w_o"], 2), (c["w_v"], 4)):
            e, Je, Ke = x[a] - ref[a], J[a] - sl[a] * J[0], K[a] - sl[a] * K[0]
            Hgn = Hgn + 2 * wt * np.outer(Je, Je)
            H = H + 2 * wt * (np.outer(Je, Je) + e * Ke)
        g = []                                           # (column, gradient, Hessian)
        for i, a in enumerate((T(0), c["L"] / 2, c["L"])):
            de, he = J[1] + a * J[2], K[1] + a * K[2]
            g += [(2 * i, -de, -he), (2 * i + 1, de, he)]
        for i in range(M):
            gap = v * c["tgap"] > c["osd"]
            g.append((7 + i, -J[0] - (c["tgap"] * J[4] if gap else 0 * J[4]),
                      -K[0] - (c["tgap"] * K[4] if gap else 0 * K[4])))
        g.append((6, J[4], K[4]))
        for col, dg, hg in g:
            Jr[k, col] = dg
            H = H - lam[k, col] * hg
    for k in range(N):
        for Hm in (H, Hgn):
            Hm[2 * k, 2 * k] += 2 * c["w_u1"]
            Hm[2 * k + 1, 2 * k + 1] += 2 * c["w_u2"]
    return dict(exact=H, gauss_newton=Hgn, J=Jr)


def case_inputs(w, b):
    obs = np.zeros((0, 2)) if w["obs"] is None else w["obs"][b]
    return w["x0"][b], w["U"][b], obs, w["lam"][b]


_yardstick = {}


def yardstick():
    """restate() in np.longdouble on the 60 cases: {(key, b): result}, computed once."""
    if not _yardstick:
        for key, cs in sorted(EC.golden_groups().items()):
            w = GC.group_inputs(key, cs)
            for b in range(len(cs)):
                _yardstick[(key, b)] = restate(key[0], *case_inputs(w, b), np.longdouble)
    return _yardstick


def measure_restatement_error():
    """The worst error of restate() in float64 against the yardstick over the cases and (exact, gauss_newton, J)."""
    worst = 0.0
    for key, cs in sorted(EC.golden_groups().items()):
        w = GC.group_inputs(key, cs)
        for b in range(len(cs)):
            r64 = restate(key[0], *case_inputs(w, b), np.float64)
            ref = yardstick()[(key, b)]
            worst = max([worst] + [rel_err(r64[k], ref[k]) for k in ("exact", "gauss_newton", "J")])
    return worst


def hessvec(slv, w, V=None, M=None, mode="exact", outputs=OUT_KEYS, **kw):
    w = dict(w, **kw)
    return slv.hessvec_batch(w["x0"], w["U"], V, M, w.get("lam"), w["obs"], w["n_obs"], mode, outputs)


def pin_directions(key, B, N):
    """Three seeded random directions per case of a golden group, [B,3,N,2]."""
    return np.random.default_rng(777 + 10000 * key[0] + 100 * key[1] + key[2]).normal(size=(B, 3, N, 2))


def hessvec_golden(env):
    """[(key, cases, inputs, {mode: dense result}, {mode: result on pin_directions})] of the golden groups, once."""
    cache = env.setdefault("_hv_golden", {})
    if env["device"] not in cache:
        out = []
        for key, cs in sorted(EC.golden_groups().items()):
            ti, N, no = key
            slv = solver(env, ti, N, no)
            w = GC.group_inputs(key, cs)
            V = pin_directions(key, len(cs), N)
            dense = {mode: hessvec(slv, w, None, 2 * N, mode) for mode in MODES}
            rand = {mode: hessvec(slv, w, V, None, mode) for mode in MODES}
            out.append((key, cs, w, dense, rand))
        cache[env["device"]] = out
    return cache[env["device"]]


def check_restatement_pin(env):
    """HV, JV and curv of the library, with unit directions (the dense H and J) and with three random directions, in both
    modes, against the longdouble yardstick on all 60 cases within RESTATE_BOUND; the cost bits are the evaluator's."""
    n, worst, differ = 0, 0.0, 0
    for key, cs, w, dense, rand in hessvec_golden(env):
        ti, N, no = key
        V = pin_directions(key, len(cs), N).reshape(len(cs), 3, 2 * N).astype(np.longdouble)
        for b, c in enumerate(cs):
            ref = yardstick()[(key, b)]
            Jref = ref["J"].reshape(N * (7 + no), 2 * N)
            errs = []
            for mode in MODES:
                d, r, H = dense[mode], rand[mode], ref[mode]
                errs += [rel_err(d["HV"][b].reshape(2 * N, 2 * N), H),
                         rel_err(d["JV"][b].reshape(2 * N, -1).T, Jref),
                         rel_err(d["curv"][b, :, 0], np.diag(H)),
                         rel_err(r["HV"][b].reshape(3, 2 * N), V[b] @ H),
                         rel_err(r["JV"][b].reshape(3, -1), V[b] @ Jref.T),
                         rel_err(r["curv"][b, :, 0], np.einsum("mi,ij,mj->m", V[b], H, V[b])),
                         rel_err(r["curv"][b, :, 1], (V[b] ** 2).sum(axis=1))]
                assert (d["curv"][b, :, 1] == 1.0).all(), (key, b, mode)
                assert d["summary"][b, 0] == r["summary"][b, 0] == float(c["cost"]), (key, b, mode)
            worst = max([worst] + errs)
            assert max(errs) <= RESTATE_BOUND, (key, b, errs)
            differ += not same(dense["exact"]["HV"][b], dense["gauss_newton"]["HV"][b])
            assert same(dense["exact"]["JV"][b], dense["gauss_newton"]["JV"][b]), (key, b)
            n += 1
    assert n == 60 and differ >= 1, (n, differ)
    print(f"restatement pin: worst error {worst:.3e} (bound {RESTATE_BOUND:.3e}); exact and Gauss-Newton differ on "
          f"{differ} of {n} cases")


# ---------------------------------------------------------------------------------------------
# 2. central differences of mpc_gradient_batch
# ---------------------------------------------------------------------------------------------
FD_DIRS = 3


def check_finite_differences(env):
    """(r(U + hV) - r(U - hV)) / 2h with r = grad - jtl of mpc_gradient_batch against HV (exact mode), for FD_DIRS
    random unit directions per smooth case, with gradient_cases' FD_H and FD_REL."""
    used, total, worst = 0, 0, 0.0
    m = GC.default_model()
    h = GC.FD_H
    for key, cs, w, _, _ in hessvec_golden(env):
        ti, N, no = key
        slv = solver(env, ti, N, no)
        B = len(cs)
        total += B
        V = np.random.default_rng(1000 * ti + 10 * N + no + 5).normal(size=(B, FD_DIRS, N, 2))
        V /= np.sqrt((V ** 2).sum(axis=(2, 3), keepdims=True))
        rep = lambda a: None if a is None else np.repeat(a, FD_DIRS, axis=0)
        res, Xp = {}, {}
        for sgn in (1.0, -1.0):
            Us = (w["U"][:, None] + sgn * h * V).reshape(-1, N, 2)
            g = slv.gradient_batch(rep(w["x0"]), Us, rep(w["obs"]), rep(w["n_obs"]), lam=rep(w["lam"]))
            res[sgn] = (g["grad"] - g["jtl"]).reshape(B, FD_DIRS, N, 2)
            Xp[sgn] = slv.evaluate_batch(rep(w["x0"]), Us, rep(w["obs"]), rep(w["n_obs"]))["Xpred"].reshape(
                B, FD_DIRS, N + 1, 5)
        fd = (res[1.0] - res[-1.0]) / (2 * h)
        HV = hessvec(slv, w, V, None, "exact", ("HV",))["HV"]
        for b in range(B):
            if not all(GC.smooth_case(ti, Xp[sgn][b, j], m) for sgn in Xp for j in range(FD_DIRS)):
                continue
            used += 1
            for j in range(FD_DIRS):
                err = np.abs(fd[b, j] - HV[b, j]).max() / max(1.0, np.abs(HV[b, j]).max())
                worst = max(worst, err)
                assert err <= GC.FD_REL, (key, b, j, err)
    print(f"finite differences: {used} of {total} cases, worst error {worst:.3e} (bound {GC.FD_REL:.1e})")
    assert total == 60 and total - used <= total // 10, (used, total)


# ---------------------------------------------------------------------------------------------
# 3. structure: symmetry, J against unit-lam jtl, curv and summary against numpy on the returned arrays
# ---------------------------------------------------------------------------------------------
def numpy_curv(V, HV):
    """(v'Hv, v'v) of one direction as the header sums them: running sums from 0 over i = 0..2N-1."""
    a = b = 0.0
    for v, h in zip(np.asarray(V, np.float64).ravel().tolist(), np.asarray(HV).ravel().tolist()):
        a = a + v * h
        b = b + v * v
    return a, b


def numpy_summary(curv):
    """Columns 1..4 of the summary restated on the returned curv [M,2] of one instance."""
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore")
        r = curv[:, 0] / curv[:, 1]
        return np.array([np.min(r), np.max(r), float(np.argmin(r)), float((curv[:, 0] < 0).sum())])


def unit_directions(M, N):
    return np.eye(2 * N)[:M].reshape(M, N, 2)


def check_curv_and_summary(r, V, what=""):
    """curv under == and the summary of a result r with HV and curv for the directions V [B,M,N,2] (None: unit)."""
    B, M, N = r["HV"].shape[:3]
    for b in range(B):
        Vb = unit_directions(M, N) if V is None else V[b]
        for mm in range(M):
            assert same(r["curv"][b, mm], np.array(numpy_curv(Vb[mm], r["HV"][b, mm]))), (what, b, mm)
        assert same(r["summary"][b, 1:], numpy_summary(r["curv"][b])), (what, b, r["summary"][b])


def check_structure(env):
    """With V NULL and M = 2N: H symmetric within RESTATE_BOUND, J equal to the unit-lam jtl rows within it (all rows of
    the first case of every golden group), curv and the summary equal numpy on the returned arrays."""
    for key, cs, w, dense, rand in hessvec_golden(env):
        ti, N, no = key
        rw = 7 + no
        slv = solver(env, ti, N, no)
        for mode in MODES:
            H = dense[mode]["HV"].reshape(len(cs), 2 * N, 2 * N)
            for b in range(len(cs)):
                assert rel_err(H[b], H[b].T) <= RESTATE_BOUND, (key, b, mode)
            check_curv_and_summary(dense[mode], None, (key, mode, "dense"))
            check_curv_and_summary(rand[mode], pin_directions(key, len(cs), N), (key, mode, "random"))
        rep = lambda a: None if a is None else np.repeat(a[:1], N * rw, axis=0)
        jtl = slv.gradient_batch(rep(w["x0"]), rep(w["U"]), rep(w["obs"]), rep(w["n_obs"]),
                                 lam=np.eye(N * rw).reshape(N * rw, N, rw))["jtl"].reshape(N * rw, 2 * N)
        J = dense["exact"]["JV"][0].reshape(2 * N, N * rw).T
        assert rel_err(J, jtl) <= RESTATE_BOUND, key


def check_summary_cases(env):
    """The summary and curv under a zero direction (0 / 0), a NaN direction, a NaN control, negative curvature and an
    infinite quotient; lam past n_obs is never read; M = 1."""
    N, mo, B, M = 10, 2, 6, 7
    slv = solver(env, 2, N, mo)
    w = GC.lam_batch(EC.random_batch(2, N, B, mo, seed=141), mo, 142)
    w["n_obs"][:] = [2, 0, 1, 2, 1, 0]
    V = np.random.default_rng(143).normal(size=(B, M, N, 2))
    base = hessvec(slv, w, V)
    check_curv_and_summary(base, V, "base")
    assert np.isfinite(base["summary"]).all() and np.isfinite(base["HV"]).all()
    for b in range(B):
        assert np.isnan(base["JV"][b, :, :, 7 + int(w["n_obs"][b]):]).all()
        assert np.isfinite(base["JV"][b, :, :, :7 + int(w["n_obs"][b])]).all()
    lp = w["lam"].copy()
    for b in range(B):
        lp[b, :, 7 + int(w["n_obs"][b]):] = np.nan
    rp = hessvec(slv, dict(w, lam=lp), V)
    for k in OUT_KEYS:
        assert same(rp[k], base[k]), k
    # a zero direction first and later, a NaN direction, a negated Hessian's worth of negative curvature
    V2 = V.copy()
    V2[0, 0] = 0.0                   # 0 / 0 first: NaN from direction 0 on
    V2[1, 3] = 0.0                   # 0 / 0 later: argmin is 3
    V2[2, 2, 4, 1] = np.nan          # a NaN direction: argmin is 2
    V2[2, 5, 0, 0] = np.nan
    r2 = hessvec(slv, w, V2)
    check_curv_and_summary(r2, V2, "special")
    assert np.isnan(r2["summary"][:3, 1:3]).all() and r2["summary"][:3, 3].tolist() == [0.0, 3.0, 2.0]
    for k in OUT_KEYS:
        assert same(r2[k][3:], base[k][3:]), k
    keep = np.ones(M, bool)
    keep[[2, 5]] = False
    for k in ("HV", "JV", "curv"):
        assert same(r2[k][2][keep], base[k][2][keep]), k
        assert np.isnan(r2[k][2][~keep]).any(), k
    # negative curvature: large lam on the rows makes cost - lam . g concave along some unit directions or not; the
    # count must equal numpy's either way, and with lam = None the Gauss-Newton Hessian has none
    big = hessvec(slv, dict(w, lam=-50.0 * w["lam"]), None, 2 * N)
    check_curv_and_summary(big, None, "big lam")
    gn = hessvec(slv, dict(w, lam=None), None, 2 * N, "gauss_newton")
    check_curv_and_summary(gn, None, "gn")
    assert (gn["summary"][:, 4] == 0).all() and (gn["summary"][:, 1] > 0).all()
    # a NaN control stays in its instance
    Un = w["U"].copy()
    Un[4, N // 2, 0] = np.nan
    rn = hessvec(slv, dict(w, U=Un), V)
    keepb = np.arange(B) != 4
    for k in OUT_KEYS:
        assert same(rn[k][keepb], base[k][keepb]), k
    assert np.isnan(rn["summary"][4, :3]).all() and np.isnan(rn["HV"][4]).any()
    check_curv_and_summary(rn, V, "nan control")
    one = hessvec(slv, w, V[:, :1])
    check_curv_and_summary(one, V[:, :1], "M = 1")
    assert (one["summary"][:, 3] == 0).all() and same(one["summary"][:, 1], one["summary"][:, 2])


# ---------------------------------------------------------------------------------------------
# 4. independence of the other directions, of the pass and of the batch
# ---------------------------------------------------------------------------------------------
def check_independence(env, N=20, mo=3):
    """A direction's outputs are the same bits alone, among 128, in another pass of the kernel and in another batch
    position, for each output asked for alone, and with unit directions."""
    B = 5
    slv = solver(env, 2, N, mo)
    W = 64 if N <= 56 else 32
    w = GC.lam_batch(EC.random_batch(2, N, B, mo, seed=151 + N), mo, 152)
    V = np.random.default_rng(153).normal(size=(B, 128, N, 2))
    for mode in MODES:
        full = hessvec(slv, w, V, None, mode)
        for mm in (0, W - 1, W, 127):
            one = hessvec(slv, w, V[:, mm:mm + 1], None, mode)
            for k in ("HV", "JV", "curv"):
                assert same(one[k][:, 0], full[k][:, mm]), (mode, mm, k)
        # the same directions in another pass and another order
        perm = np.random.default_rng(154).permutation(128)
        pr = hessvec(slv, w, V[:, perm], None, mode)
        for k in ("HV", "JV", "curv"):
            assert same(pr[k], full[k][:, perm]), (mode, k)
        # another batch position, B = 1
        bp = np.random.default_rng(155).permutation(B)
        take = lambda idx: {k: (None if a is None else a[idx]) for k, a in w.items()}
        rb = hessvec(slv, take(bp), V[bp][:, :W + 1], None, mode)
        for k in OUT_KEYS[:3]:
            assert same(rb[k], full[k][bp][:, :W + 1]), (mode, k)
        r1 = hessvec(slv, take(slice(2, 3)), V[2:3], None, mode)
        for k in OUT_KEYS:
            assert same(r1[k][0], full[k][2]), (mode, k)
        for k in OUT_KEYS:
            assert same(hessvec(slv, w, V, None, mode, (k,))[k], full[k]), (mode, k)
        # unit directions by V and by NULL
        M = min(2 * N, 128)
        E = np.broadcast_to(unit_directions(M, N), (B, M, N, 2))
        ru, rv = hessvec(slv, w, None, M, mode), hessvec(slv, w, E, None, mode)
        for k in OUT_KEYS:
            assert same(ru[k], rv[k]), (mode, k)
    # a NaN instance and a NaN direction leave the others untouched
    full = hessvec(slv, w, V)
    x0n = w["x0"].copy()
    x0n[1, 4] = np.nan
    Vn = V.copy()
    Vn[3, 70, 0, 0] = np.nan
    rn = hessvec(slv, dict(w, x0=x0n), Vn)
    for k in OUT_KEYS[:3]:
        assert same(rn[k][[0, 2, 4]], full[k][[0, 2, 4]]), k
        keep = np.arange(128) != 70
        assert same(rn[k][3][keep], full[k][3][keep]), k
        assert np.isnan(rn[k][3][70]).any() and np.isnan(rn[k][1]).any(), k
    assert same(rn["summary"][[0, 2, 4]], full["summary"][[0, 2, 4]]) and rn["summary"][3, 3] == 70.0


# ---------------------------------------------------------------------------------------------
# 6. the argument contract
# ---------------------------------------------------------------------------------------------
def raw_hessvec(env, slv, w, want, B=None, M=None, V=None, mode=0):
    """mpc_hessvec_batch through ctypes with only the outputs named in `want`; returns (rc, outputs)."""
    mpcqp = env["mpcqp"]
    p = slv.params
    B = w["x0"].shape[0] if B is None else B
    nb, nm = max(B, 0), max(M, 0)
    shapes = dict(HV=(nb, nm, p.N, 2), JV=(nb, nm, p.N, 7 + p.max_obs), curv=(nb, nm, 2), summary=(nb, mpcqp.HV_NQ))
    out = {k: np.full(shapes[k], -7.0) for k in want}
    dp = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    rc = mpcqp.lib().mpc_hessvec_batch(slv.h, B, dp(w["x0"]), dp(w["obs"]), ip(w["n_obs"]), dp(w["U"]),
                                       dp(w.get("lam")), M, dp(V), mode, *(dp(out.get(k)) for k in OUT_KEYS))
    return rc, out


def check_contract(env):
    mpcqp = env["mpcqp"]
    N, mo, B, M = 10, 2, 6, 5
    slv = solver(env, 2, N, mo)
    w = GC.lam_batch(EC.random_batch(2, N, B, mo, seed=161), mo, 162)
    V = np.random.default_rng(163).normal(size=(B, 128, N, 2))

    def refused(rc):
        assert rc == -1 and len(mpcqp.last_error()) > 0, (rc, mpcqp.last_error())

    rc, ok = raw_hessvec(env, slv, w, OUT_KEYS, M=M, V=V[:, :M])
    assert rc == 0 and not any((ok[k] == -7.0).any() for k in OUT_KEYS)
    assert raw_hessvec(env, slv, w, OUT_KEYS, M=128, V=V)[0] == 0
    assert raw_hessvec(env, slv, w, OUT_KEYS, M=2 * N)[0] == 0
    assert raw_hessvec(env, slv, dict(w, lam=None), OUT_KEYS, M=1, mode=1)[0] == 0
    refused(raw_hessvec(env, slv, w, OUT_KEYS, M=0, V=V)[0])
    refused(raw_hessvec(env, slv, w, OUT_KEYS, M=-1, V=V)[0])
    refused(raw_hessvec(env, slv, w, ("summary",), M=129, V=V)[0])
    refused(raw_hessvec(env, slv, w, OUT_KEYS, M=2 * N + 1)[0])                  # V NULL with M > 2N
    refused(raw_hessvec(env, slv, w, OUT_KEYS, M=M, V=V[:, :M], mode=2)[0])
    refused(raw_hessvec(env, slv, w, OUT_KEYS, M=M, V=V[:, :M], mode=-1)[0])
    refused(raw_hessvec(env, slv, dict(w, U=None), OUT_KEYS, M=M, V=V[:, :M])[0])
    refused(raw_hessvec(env, slv, dict(w, x0=None), OUT_KEYS, B=B, M=M, V=V[:, :M])[0])
    refused(raw_hessvec(env, slv, w, OUT_KEYS, B=-1, M=M, V=V[:, :M])[0])
    with np.testing.assert_raises(ValueError):
        slv.hessvec_batch(w["x0"], None)
    s0 = solver(env, 2, N, 0)
    refused(raw_hessvec(env, s0, dict(w, lam=None), ("summary",), M=1)[0])      # obs with max_obs == 0
    with np.testing.assert_raises(ValueError):
        s0.hessvec_batch(w["x0"], w["U"], obs=w["obs"], n_obs=w["n_obs"])
    # B == 0 succeeds; all outputs NULL launches nothing and succeeds
    assert raw_hessvec(env, slv, w, OUT_KEYS, B=0, M=M, V=V[:, :M])[0] == 0
    assert raw_hessvec(env, slv, w, (), M=M, V=V[:, :M])[0] == 0
    # n_obs outside [0, max_obs] is clamped, NULL means all rows
    wild = np.array([5, -3, 2, 0, 1, 99], np.int32)
    a, b = hessvec(slv, w, V[:, :M], n_obs=wild), hessvec(slv, w, V[:, :M], n_obs=np.clip(wild, 0, mo))
    full, none = hessvec(slv, w, V[:, :M], n_obs=np.full(B, mo, np.int32)), hessvec(slv, w, V[:, :M], n_obs=None)
    for k in OUT_KEYS:
        assert same(a[k], b[k]) and same(full[k], none[k]), k
    # Solver.hessian_batch: the dense layout
    d = slv.hessian_batch(w["x0"], w["U"], w["lam"], w["obs"], w["n_obs"])
    r = hessvec(slv, w, None, 2 * N)
    assert d["H"].shape == (B, 2 * N, 2 * N) and d["J"].shape == (B, N * (7 + mo), 2 * N)
    assert same(d["H"], r["HV"].reshape(B, 2 * N, 2 * N))
    assert same(d["J"], r["JV"].reshape(B, 2 * N, -1).transpose(0, 2, 1)) and same(d["summary"], r["summary"])
    # the device entry: misaligned double arrays, n_obs without obs
    keep = []

    def ptr(a, off=0):
        if a is None:
            return None
        addr, k = env["ptr"](a)
        keep.append(k)
        return addr + off

    L = mpcqp.lib()
    x0p, Up, op, np_, lp, Vp = (ptr(w["x0"]), ptr(w["U"]), ptr(w["obs"]), ptr(w["n_obs"]), ptr(w["lam"]),
                                ptr(np.ascontiguousarray(V[:, :M])))
    hp, jp, cp, sp = (ptr(np.zeros((B, M, N, 2))), ptr(np.zeros((B, M, N, 7 + mo))), ptr(np.zeros((B, M, 2))),
                      ptr(np.zeros((B, mpcqp.HV_NQ))))
    call = lambda x0, o, n, U, l, V, H, J, c, s, M=M, mode=0: L.mpc_hessvec_batch_device(slv.h, B, x0, o, n, U, l, M, V,
                                                                                        mode, H, J, c, s, None)
    good = (x0p, op, np_, Up, lp, Vp, hp, jp, cp, sp)
    assert call(*good) == 0
    for i in (0, 1, 3, 4, 5, 6, 7, 8, 9):
        refused(call(*(a + 4 if j == i else a for j, a in enumerate(good))))
    refused(call(x0p, None, np_, Up, lp, Vp, hp, jp, cp, sp))                   # n_obs without obs
    refused(call(x0p, op, np_, None, lp, Vp, hp, jp, cp, sp))
    refused(call(*good, M=129))
    refused(call(*good, mode=7))
    refused(call(x0p, op, np_, Up, lp, None, hp, jp, cp, sp, M=2 * N + 1))
    assert call(x0p, op, np_, Up, lp, Vp, None, None, None, None) == 0
    assert L.mpc_hessvec_batch_device(slv.h, 0, None, None, None, None, None, M, None, 0, None, None, None, None,
                                      None) == 0
    env.get("sync", lambda: None)()          # the buffers in `keep` outlive the asynchronous call


# ---------------------------------------------------------------------------------------------
# 5. the shapes of the GPU == host test
# ---------------------------------------------------------------------------------------------
SHAPE_N = (1, 5, 15, 16, 31, 32, 63)
SHAPE_MO = (0, 3)
SHAPE_B = 5


def pass_width(N):
    """The header's table: 64 directions per pass for N <= MPC_HV_N64_MAX = 56, 32 beyond."""
    return 64 if N <= 56 else 32


def shape_runs(N, mo):
    """(what, batch, V, M, mode) of one (N, max_obs) on trajectory 1: M = 1, the dense call (V NULL, M = 2N, capped at
    128), one M that straddles a pass boundary and M = 128, in exact mode with lam; Gauss-Newton and no lam on the
    straddling M; n_obs mixed over {0, 1, 3}, NULL on the dense call.  Instance 3 rolls past s_max."""
    w = GC.lam_batch(EC.random_batch(1, N, SHAPE_B, mo, seed=4000 * N + mo, nobs_mode=None), mo, 5000 * N + mo)
    V = np.random.default_rng(6000 * N + mo).normal(size=(SHAPE_B, 128, N, 2))
    mixed = dict(w, n_obs=np.array([3, 0, 1, 3, 1], np.int32)) if mo else w
    ms = pass_width(N) + 1
    yield "M = 1", mixed, V[:, :1], None, "exact"
    yield "dense", w, None, min(2 * N, 128), "exact"
    yield "straddle", mixed, V[:, :ms], None, "exact"
    yield "M = 128", mixed, V, None, "exact"
    yield "gauss-newton", mixed, V[:, :ms], None, "gauss_newton"
    yield "no lam", dict(mixed, lam=None), V[:, :ms], None, "exact"
