"""Shared pieces of the convoy tests (test_convoy_cpu.py on the host backend, test_gpu_convoy.py on the device):
a numpy brute-force leader choice written from the definition in include/mpcqp.h, a stepwise restatement of
mpc_closed_loop_convoy built from pinned code (traffic_cases' per-actor ObstaclesFSM shims, Solver.solve_batch on
a context with max_obs = A + K, the Euler step in numpy), and the comparisons.  Every comparison is bit for bit
(sweep_cases.same): the references run the same solver on the same inputs.  Trajectory2, N = 20."""
import numpy as np

import sweep_cases as SC
import traffic_cases as TC

S0 = SC.S0
QCOLS = TC.QCOLS
LEADER = 1000          # marks a leader's slab entry where traffic_cases.quantities expects an actor index
HISTS = ("hist_x", "hist_u", "hist_car_s", "hist_slab", "hist_tl", "hist_status", "hist_nobs", "hist_lead")


def leaders(s, active, W, K, lead_range):
    """The definition, by brute force: for every ego still in the loop, the egos of its world that are ahead of
    it (s_j > s_i, or s_j == s_i and j < i) and still in the loop, nearest first in that order, at most K, cut
    at the first one with s_j - s_i >= lead_range.  Returns one list of batch indices per ego."""
    out = [[] for _ in range(s.size)]
    for i in np.flatnonzero(active):
        w0 = (i // W) * W
        cand = [j for j in range(w0, w0 + W)
                if j != i and active[j] and (s[j] > s[i] or (s[j] == s[i] and j < i))]
        # among the egos ahead of i, j is nearer than k iff k is ahead of j
        cand.sort(key=lambda j: (s[j], -j))
        for j in cand[:K]:
            if s[j] - s[i] >= lead_range:
                break
            out[i].append(int(j))
    return out


def driver(TT, mpcqp, shard, slv_obs, x_init, W, K, lead_range, scripts, max_steps, s_stop):
    """The stepwise restatement for B egos in worlds of W (scripts: None or one script of length A per ego;
    A + K == slv_obs.params.max_obs, K > 0 and W > 1 so that the solver runs with the slab).  Returns
    closed_loop_convoy's dict with every ego's history kept (step_ms excepted, quant columns 0 and 8 at 0)."""
    x = np.array(x_init, np.float64).reshape(-1, 5)
    B, dt = x.shape[0], slv_obs.params.dt
    scripts = [[] for _ in range(B)] if scripts is None else scripts
    A = len(scripts[0])
    AK = A + K
    assert AK == slv_obs.params.max_obs and all(len(s) == A for s in scripts) and K > 0 and W > 1 and B % W == 0
    fsms = [[TC.shim_fsm(TT, mpcqp, a) for a in scr] for scr in scripts]
    hx = np.full((B, max_steps + 1, 5), np.nan); hu = np.full((B, max_steps, 2), np.nan)
    hc = np.full((B, max_steps), np.nan); hl = np.full((B, max_steps, AK, 2), np.nan)
    ht = np.full((B, max_steps), -1, np.int32); hs = np.full((B, max_steps), -1, np.int32)
    hn = np.full((B, max_steps), -1, np.int32); hd = np.full((B, max_steps, K), -1, np.int32)
    who = np.full((B, max_steps, AK), -1, np.int32)          # script car: its actor index; leader: LEADER
    ns = np.zeros(B, np.int32)
    hx[:, 0] = x
    active = x[:, 0] <= s_stop
    for step in range(max_steps):
        idx = np.flatnonzero(active)
        if idx.size == 0:
            break
        lead = leaders(x[:, 0], active, W, K, lead_range)
        slab = np.zeros((idx.size, AK, 2)); nobs = np.zeros(idx.size, np.int32)
        for i, b in enumerate(idx):
            obs, green = TC.fsm_step(mpcqp, fsms[b], dt, x[b, 0], x[b, 4])
            for j, (os_, ov, a, typ) in enumerate(obs):
                slab[i, j] = (os_, ov)
                if typ == "car":
                    who[b, step, j] = a
            n = len(obs)
            for m, j in enumerate(lead[b]):
                slab[i, n + m] = (x[j, 0], x[j, 4])
                who[b, step, n + m] = LEADER
                hd[b, step, m] = j
            n += len(lead[b])
            nobs[i] = n
            cars = [o[0] for o in obs if o[3] == "car"]
            hc[b, step] = cars[0] if cars else np.nan
            ht[b, step], hn[b, step] = green, n
            hl[b, step, :n] = slab[i, :n]
        r = slv_obs.solve_batch(x[idx], slab, nobs)
        k_ref = slv_obs.lookup(x[idx, 0])[0][:, 3]
        for i, b in enumerate(idx):
            s, d, o, k, v = x[b]
            u = r["u0"][i]
            x[b] = x[b] + dt * np.array([v, v * o, v * (k - k_ref[i]), u[0], u[1]])
            hx[b, step + 1], hu[b, step], hs[b, step] = x[b], u, r["status"][i]
            ns[b] = step + 1
            if not x[b, 0] <= s_stop:
                active[b] = False
    out = dict(n_steps=ns, hist_x=hx, hist_u=hu, hist_car_s=hc, hist_tl=ht, hist_status=hs, hist_nobs=hn,
               hist_slab=hl, hist_lead=hd, hist_egos=np.arange(B))
    quant, ex3 = TC.quantities(mpcqp, shard, out, who, scripts)
    ex3[ex3[:, 2] == LEADER, 2] = -1.0                       # a leader holds the minimum
    out["quant"] = quant
    out["extra"] = np.concatenate([ex3, lead_extras(hx, hd, ns)], axis=1)
    return out


def lead_extras(hist_x, hist_lead, n_steps):
    """Extras 3..5 from full histories: the leaders' positions are their own states before the step."""
    B = n_steps.size
    ex = np.zeros((B, 3))
    for b in range(B):
        n = int(n_steps[b])
        ld = hist_lead[b, :n]
        if not (ld >= 0).any():
            ex[b] = (np.nan, -1.0, 0.0)
            continue
        steps = np.arange(n)[:, None] + 0 * ld
        gap = np.where(ld >= 0, hist_x[np.maximum(ld, 0), steps, 0] - hist_x[b, :n, 0][:, None], np.inf).ravel()
        k = int(np.argmin(gap))                              # first occurrence: earliest step, then slab order
        ex[b] = (gap[k], ld.ravel()[k], (ld >= 0).sum(axis=1).max())
    return ex


def assert_equals_driver(cv, d):
    """Every output of closed_loop_convoy with every ego kept equals the restatement."""
    assert np.array_equal(cv["n_steps"], d["n_steps"])
    for name in HISTS:
        assert cv[name].shape == d[name].shape, name
        for b in range(d["n_steps"].size):
            assert SC.same(cv[name][b].astype(np.float64), d[name][b].astype(np.float64)), (name, b)
    assert SC.same(cv["quant"][:, QCOLS], d["quant"][:, QCOLS]), (cv["quant"], d["quant"])
    assert SC.same(cv["extra"], d["extra"]), (cv["extra"], d["extra"])
    SC.assert_step_time_column(cv)


def ego(traj, s, v=9.0, d=0.0):
    return [s, d, 0.0, traj.get_state(s)[3], v]


# ---------------------------------------------------------------------------------------------
# the restatement cases.  W_R = 6, three worlds, one set of starts for the runs without a script:
#   world 0  a platoon at an even 10 m headway, ego 0 last
#   world 1  egos 6, 7 at the same s (7 the faster: it is behind 6 by the tie rule at step 0 and ahead of it
#            from step 1 on, so ranks change), egos 8, 9, 10 at one s with different d, ego 11 ahead of all
#   world 2  ego 12 leads and passes s_stop within a few steps while 13, 14, 15 go on; 16, 17 start past s_stop
# ---------------------------------------------------------------------------------------------
W_R = 6
S_STOP_R = S0 + 70.0
STEPS_R = 100


def plain_starts(traj):
    w0 = [ego(traj, S0 + 10.0 * i) for i in range(6)]
    w1 = [ego(traj, S0 + 20.0, v=5.0), ego(traj, S0 + 20.0, v=9.0),
          ego(traj, S0, d=-0.3), ego(traj, S0, d=0.0), ego(traj, S0, d=0.3), ego(traj, S0 + 45.0)]
    w2 = [ego(traj, S_STOP_R - 4.0), ego(traj, S_STOP_R - 14.0), ego(traj, S_STOP_R - 30.0),
          ego(traj, S_STOP_R - 31.0, v=7.0), ego(traj, S_STOP_R + 1.0), ego(traj, S_STOP_R + 5.0)]
    return np.array(w0 + w1 + w2)


PLAIN = {"k1": (1, np.inf), "k3": (3, np.inf), "k_over": (7, np.inf), "range_cut": (3, 15.0)}


def plain_driver(env, name):
    K, lead_range = PLAIN[name]
    x_init = plain_starts(env["traj"])
    d = driver(env["TT"], env["mpcqp"], env["shard"], env["solver"](max_obs=K), x_init, W_R, K, lead_range, None,
               STEPS_R, S_STOP_R)
    assert_plain_shape(name, d)
    return dict(x_init=x_init, d=d, K=K, lead_range=lead_range)


def assert_plain_shape(name, d):
    """The restatement shows what each case is for (a failure here means the inputs are wrong, not the library)."""
    K, lead_range = PLAIN[name]
    ns, ld = d["n_steps"], d["hist_lead"]
    nlead = (ld >= 0).sum(axis=2)
    # the platoon at step 0: ego i follows i + 1, i + 2, ..
    want = min(K, 1 if name == "range_cut" else 5)
    assert ld[0, 0, :want].tolist() == list(range(1, 1 + want)) and nlead[0, 0] == want
    assert nlead[5, :ns[5]].max() == 0 and np.isnan(d["extra"][5, 3]) and d["extra"][5, 4] == -1.0
    if name == "range_cut":     # two egos ahead within K, the second one 20 m away: cut
        assert (nlead[:4, 0] == 1).all() and d["hist_x"][2, 0, 0] - d["hist_x"][0, 0, 0] >= lead_range
    if name == "k_over":
        assert nlead.max() == W_R - 1
    # the tie and the change of ranks: 7 follows 6 at step 0 (gap 0), 6 follows 7 from step 1 on
    far = -1 if name == "range_cut" else 11                  # ego 11 is 25 m ahead of them
    assert ld[7, 0, 0] == 6 and d["hist_slab"][7, 0, 0, 0] == d["hist_x"][7, 0, 0] and ld[6, 0, 0] == far
    assert ld[6, 1, 0] == 7 and ld[7, 1, 0] == far
    # three egos at one s: the lower index is ahead
    assert ld[8, 0, 0] == (-1 if name == "range_cut" else 7) and ld[9, 0, 0] == 8 and ld[10, 0, 0] == 9
    assert d["extra"][9, 3] == 0.0 and d["extra"][9, 4] == 8.0 and d["quant"][9, 9] == 0.0
    # the departing leader: in 13's slab at step 0, gone once it has left, while 13 goes on
    assert ld[13, 0, 0] == 12 and ns[12] < 10 and ns[13] > ns[12] + 3
    assert not (ld[13, ns[12]:] == 12).any() and (ld[13, :ns[12]] == 12).any()
    # egos that start past s_stop never run and are never anyone's leader
    assert ns[16] == 0 and ns[17] == 0 and not np.isin(ld, (16, 17)).any()
    assert nlead[12, :ns[12]].max() == 0
    # leaders never come from another world
    for b in range(ld.shape[0]):
        seen = ld[b][ld[b] >= 0]
        assert ((seen // W_R) == b // W_R).all()


def check_plain(env, name, case):
    cv = env["solver"]().closed_loop_convoy(case["x_init"], W_R, case["K"], lead_range=case["lead_range"],
                                            max_steps=STEPS_R, s_stop=S_STOP_R, hist_egos=range(18))
    assert_equals_driver(cv, case["d"])
    assert np.array_equal(cv["quant"][:, 0], np.arange(18.0))


# a light ahead of two platoons (one shared script, A = 1): the lead stops and the rest queue behind it
W_Q, K_Q, STEPS_Q = 5, 2, 150
S_STOP_Q = S0 + 80.0


def queue_case(env):
    mpcqp, traj = env["mpcqp"], env["traj"]
    script = [mpcqp.light(S0 + 60.0, 100.0, 3.0)]
    w0 = [ego(traj, S0 + 8.0 * i) for i in range(W_Q)]
    w1 = [ego(traj, S0 + 1.0 + 5.0 * i, v=8.0) for i in range(W_Q)]
    x_init = np.array(w0 + w1)
    d = driver(env["TT"], mpcqp, env["shard"], env["solver"](max_obs=1 + K_Q), x_init, W_Q, K_Q, np.inf,
               [script] * (2 * W_Q), STEPS_Q, S_STOP_Q)
    ns, v = d["n_steps"], d["hist_x"][:, :, 4]
    lead = W_Q - 1
    stopped = [np.flatnonzero(v[b, :ns[b]] < 0.1) for b in range(W_Q)]
    assert stopped[lead].size, "the lead never stops at the light"
    assert all(st.size for st in stopped), "no queue behind the lead"
    assert stopped[0][0] >= stopped[lead][0]
    assert d["hist_tl"][lead, ns[lead] - 1] == 1 and d["extra"][:, 1].max() == 0.0      # GREEN, nobody ran the light
    assert d["quant"][:, 11].sum() > 0, "no elastic QP in the queue"
    assert d["hist_nobs"].max() == 1 + K_Q
    return dict(x_init=x_init, script=script, d=d)


def check_queue(env, case):
    cv = env["solver"]().closed_loop_convoy(case["x_init"], W_Q, K_Q, scripts=case["script"], max_steps=STEPS_Q,
                                            s_stop=S_STOP_Q, hist_egos=range(2 * W_Q))
    assert_equals_driver(cv, case["d"])


# scripted cars and leaders together, A + K = 16: traffic_cases' eight cars per ego and up to 8 leaders (W = 8
# gives 7; the slab is 16 wide)
def full_case(env):
    mpcqp, traj = env["mpcqp"], env["traj"]
    names, scripts = TC.many_scripts(mpcqp)
    eight = scripts[names.index("eight_cars")]
    three = scripts[names.index("three_cars")]
    x_init = np.array([ego(traj, S0 + 3.0 * i) for i in range(8)] +
                      [ego(traj, S0 - 2.0 * i, v=6.0 + 0.25 * i) for i in range(8)])
    rows = [eight] * 8 + [three] * 8
    d = driver(env["TT"], mpcqp, env["shard"], env["solver"](max_obs=16), x_init, 8, 8, np.inf, rows, 60,
               TC.S_STOP_MANY)
    assert d["hist_nobs"].max() == 15 and d["extra"][:, 5].max() == 7.0
    assert (d["extra"][:, 2] >= 0).any() and (d["extra"][:8, 2] == -1.0).any()    # a car here, a leader there
    return dict(x_init=x_init, rows=rows, d=d)


def check_full(env, case):
    cv = env["solver"]().closed_loop_convoy(case["x_init"], 8, 8, scripts=case["rows"], max_steps=60,
                                            s_stop=TC.S_STOP_MANY, hist_egos=range(16))
    assert cv["hist_slab"].shape == (16, 60, 16, 2)
    assert_equals_driver(cv, case["d"])


# ---------------------------------------------------------------------------------------------
# the other shared bodies
# ---------------------------------------------------------------------------------------------
def check_anchor(env):
    """Worlds of one ego with any K, and K = 0 with W = 4: mpc_closed_loop_traffic on the same inputs."""
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"]()
    names, scripts = TC.many_scripts(mpcqp)
    scripts, x_init = scripts + scripts[:2], SC.starts(traj, 8)
    A, ms = TC.A_MANY, TC.MAX_STEPS_MANY
    tr = slv.closed_loop_traffic(x_init, scripts, ms, s_stop=TC.S_STOP_MANY, hist_egos=range(8))
    assert tr["extra"][:, 0].max() == 8 and (tr["n_steps"] >= 20).all()
    for W, K in ((1, 0), (1, 3), (1, 8), (4, 0)):
        cv = slv.closed_loop_convoy(x_init, W, K, scripts=scripts, max_steps=ms, s_stop=TC.S_STOP_MANY,
                                    hist_egos=range(8))
        assert SC.same(cv["quant"][:, QCOLS], tr["quant"][:, QCOLS]), (W, K)
        assert SC.same(cv["extra"][:, :3], tr["extra"]), (W, K)
        assert np.isnan(cv["extra"][:, 3]).all() and (cv["extra"][:, 4] == -1.0).all() and (cv["extra"][:, 5] == 0.0).all()
        assert np.array_equal(cv["n_steps"], tr["n_steps"])
        for name in ("hist_x", "hist_u", "hist_car_s", "hist_tl", "hist_status", "hist_nobs"):
            assert SC.same(cv[name].astype(np.float64), tr[name].astype(np.float64)), (name, W, K)
        assert cv["hist_slab"].shape == (8, ms, A + K, 2) and cv["hist_lead"].shape == (8, ms, K)
        assert SC.same(cv["hist_slab"][:, :, :A], tr["hist_slab"]) and np.isnan(cv["hist_slab"][:, :, A:]).all()
        assert (cv["hist_lead"] == -1).all()
        SC.assert_step_time_column(cv)


def permuted_starts(traj, W, seed, spacing=0.5, v=6.0):
    """W starts on an even spacing from S0 on, in a fixed permutation (rank differs from index), with one tie
    pair: the ego at the second position takes the first position's s."""
    perm = np.random.default_rng(seed).permutation(W)
    s = S0 + spacing * perm
    if W > 1:
        s[np.flatnonzero(perm == 1)[0]] = S0
    return np.array([ego(traj, si, v=v, d=0.01 * (i % 3)) for i, si in enumerate(s)])


def brute_rows(cv, b, lead, K):
    """hist_lead, hist_nobs, hist_slab rows of ego b from `lead`, the brute-force choice per step (leaders() on
    the run's own hist_x, every ego kept and running every step, no script entries)."""
    hx = cv["hist_x"]
    T = cv["hist_lead"].shape[1]
    ld = np.full((T, K), -1, np.int32); nobs = np.full(T, -1, np.int32); slab = np.full((T, K, 2), np.nan)
    for step, per_ego in enumerate(lead):
        ld[step, :len(per_ego[b])] = per_ego[b]
        nobs[step] = len(per_ego[b])
        for m, j in enumerate(per_ego[b]):
            slab[step, m] = (hx[j, step, 0], hx[j, step, 4])
    return ld, nobs, slab


def check_boundaries(env, W, n_worlds):
    """Wave and workgroup boundaries: K = 2, 12 steps, every ego kept; a handful of egos against the brute force
    applied to the run's own hist_x."""
    traj, slv = env["traj"], env["solver"]()
    K, ms, B = 2, 12, W * n_worlds
    x_init = np.concatenate([permuted_starts(traj, W, 100 + w) for w in range(n_worlds)])
    cv = slv.closed_loop_convoy(x_init, W, K, max_steps=ms, s_stop=S0 + 200.0, hist_egos=range(B))
    assert (cv["n_steps"] == ms).all()
    ex = lead_extras(cv["hist_x"], cv["hist_lead"], cv["n_steps"])
    lead = [leaders(cv["hist_x"][:, step, 0], np.ones(B, bool), W, K, np.inf) for step in range(ms)]
    local = sorted({0, W - 1} | {i for m in range(64, W + 1, 64) for i in (m - 1, m) if i < W})
    ties = 0
    for w in range(n_worlds):
        for i in local:
            b = w * W + i
            ld, nobs, slab = brute_rows(cv, b, lead, K)
            assert np.array_equal(cv["hist_lead"][b], ld), (W, b)
            assert np.array_equal(cv["hist_nobs"][b], nobs), (W, b)
            assert SC.same(cv["hist_slab"][b], slab), (W, b)
            assert SC.same(cv["extra"][b, 3:], ex[b]), (W, b)
        s0 = x_init[w * W:(w + 1) * W, 0]
        lo, hi = np.flatnonzero(s0 == S0)
        ties += int(cv["hist_lead"][w * W + hi, 0, 0] == w * W + lo and cv["hist_slab"][w * W + hi, 0, 0, 0] == S0)
    assert ties == n_worlds                                  # the tie pair: the lower index is the leader, gap 0
    # every ego but each world's front one has a leader at step 0; rank differs from index
    assert ((cv["hist_lead"][:, 0, 0] >= 0).sum() == B - n_worlds)
    if W > 2:
        assert (cv["hist_lead"][:, 0, 0] != np.arange(B) + 1)[:-1].any()


def check_isolation(env):
    """5 worlds of W = 7, different permutations of the starts: world w cut out and run alone gives the same
    rows, with MIN_LEAD_EGO and hist_lead shifted by w * W."""
    traj, slv, mpcqp = env["traj"], env["solver"](), env["mpcqp"]
    W, K, ms, nw = 7, 3, 40, 5
    x_init = np.concatenate([permuted_starts(traj, W, 7 + w, spacing=6.0, v=5.0 + w) for w in range(nw)])
    cv = slv.closed_loop_convoy(x_init, W, K, max_steps=ms, s_stop=SC.S_STOP, hist_egos=range(W * nw), lead_range=25.0)
    assert cv["extra"][:, 5].max() == K and len(set(cv["n_steps"].tolist())) > 3
    for w in range(nw):
        sl = slice(w * W, (w + 1) * W)
        r1 = slv.closed_loop_convoy(x_init[sl], W, K, max_steps=ms, s_stop=SC.S_STOP, hist_egos=range(W),
                                    lead_range=25.0)
        assert np.array_equal(cv["n_steps"][sl], r1["n_steps"])
        assert SC.same(cv["quant"][sl][:, QCOLS], r1["quant"][:, QCOLS])
        e1 = r1["extra"].copy()
        e1[:, 4] += np.where(e1[:, 4] >= 0, w * W, 0)
        assert SC.same(cv["extra"][sl], e1), w
        for name in HISTS:
            a, b = cv[name][sl].astype(np.float64), r1[name].astype(np.float64)
            if name == "hist_lead":
                b = b + np.where(b >= 0, w * W, 0)
            assert SC.same(a, b), (name, w)
    # the shard offset moves the ego column and MIN_LEAD_EGO
    lo = slv.closed_loop_convoy(x_init[:W], W, K, max_steps=ms, s_stop=SC.S_STOP, lead_range=25.0, lo=100)
    assert np.array_equal(lo["quant"][:, 0], 100.0 + np.arange(W))
    assert SC.same(lo["extra"][:, 4], cv["extra"][:W, 4] + np.where(cv["extra"][:W, 4] >= 0, 100, 0))


def check_verdicts(env):
    """A two-ego world whose follower starts 0.5 m behind a standing leader."""
    from sanity_checks import check_verdicts as ref_verdicts
    from shard import CL_FIELDS
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"]()
    x_init = np.array([ego(traj, S0, v=1.0), ego(traj, S0 + 0.5, v=0.0)])
    cv = slv.closed_loop_convoy(x_init, 2, 1, max_steps=200, s_stop=S0 + 20.0)
    assert (cv["n_steps"] >= 2).all()
    p = slv.params
    v, counts = slv.cl_verdicts(cv["quant"], traj.s_max)
    exp = [ref_verdicts(dict(zip(CL_FIELDS, row[:11])), list(p.u_min), list(p.u_max), traj.s_max)
           for row in cv["quant"]]
    for b, e in enumerate(exp):
        for k, name in enumerate(mpcqp.CLV_NAMES):
            assert bool(v[b] & (1 << k)) == bool(e[name]), (b, name)
    assert counts.tolist() == [sum(bool(e[name]) for e in exp) for name in mpcqp.CLV_NAMES]
    bit = {name: 1 << k for k, name in enumerate(mpcqp.CLV_NAMES)}
    assert cv["quant"][0, 9] <= 0.5 and not v[0] & bit["obstacle_ok"] and v[1] & bit["obstacle_ok"]
    assert cv["extra"][0, mpcqp.CVX_MIN_LEAD_EGO] == 1.0 and cv["extra"][0, mpcqp.CVX_MIN_LEAD_GAP] <= 0.5
    assert cv["extra"][0, mpcqp.TRX_MIN_GAP_ACTOR] == -1.0 and cv["extra"][0, mpcqp.CVX_MAX_LEADERS] == 1.0


def check_misuse(env):
    """Every misuse case of include/mpcqp.h is MPC_E_ARG with a message; B == 0 succeeds; the version."""
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"]()
    L = mpcqp.lib()
    assert L.mpc_version() == 5
    B, A, W, K = 6, 2, 3, 2
    x = np.ascontiguousarray(SC.starts(traj, B))
    arr = (mpcqp.MpcActor * (B * A))(*([mpcqp.car(S0 + 5.0, S0 + 40.0, 4.0, TC.FAR), mpcqp.light(S0 + 30.0, 100.0, 1.0)] * B))
    bad = (mpcqp.MpcActor * (B * A))(*arr)
    bad[3].kind = 3
    neg = (mpcqp.MpcActor * (B * A))(*arr)
    neg[0].kind = -1
    wide = (mpcqp.MpcActor * (B * 15))()
    quant = np.empty((B, 13))
    hx = np.empty((2, 11, 5)); hl = np.empty((2, 10, 16, 2)); hd = np.empty((2, 10, 16), np.int32)

    def call(B=B, W=W, K=K, lead_range=np.inf, actors=arr, A=A, n_scripts=B, q=quant, n_hist=0, egos=None,
             hist_x=None, hist_slab=None, hist_lead=None):
        he = None if egos is None else np.asarray(egos, np.int32)
        rc = L.mpc_closed_loop_convoy(slv.h, B, W, K, lead_range, mpcqp._p(x), actors, A, n_scripts, 10, SC.S_STOP,
                                      mpcqp._p(q), None, n_hist, mpcqp._pi(he), mpcqp._p(hist_x), None, None, None,
                                      None, None, mpcqp._p(hist_slab), mpcqp._pi(hist_lead), None, None)
        return rc, mpcqp.last_error()

    assert call()[0] == 0                                        # the well-formed call these cases depart from
    none = dict(actors=None, A=0, n_scripts=0)
    for kw in (dict(A=-1), dict(A=17), dict(n_scripts=2), dict(n_scripts=0), dict(actors=None, n_scripts=1),
               dict(actors=None, n_scripts=B), dict(actors=None, n_scripts=0), dict(actors=bad), dict(actors=neg),
               dict(q=None), dict(n_hist=-1), dict(n_hist=0, hist_x=hx), dict(n_hist=0, hist_slab=hl),
               dict(n_hist=2, egos=[1, B], hist_x=hx), dict(n_hist=2, egos=[-1, 2], hist_x=hx),
               dict(n_hist=2, egos=[1, 1], hist_x=hx),
               dict(W=0), dict(W=-1), dict(W=257), dict(W=4), dict(W=5), dict(K=-1), dict(K=17), dict(K=15),
               dict(actors=wide, A=15, K=2), dict(lead_range=0.0), dict(lead_range=-1.0), dict(lead_range=np.nan),
               dict(none, K=0, n_hist=2, egos=[0, 1], hist_slab=hl), dict(K=0, n_hist=2, egos=[0, 1], hist_lead=hd),
               dict(n_hist=0, hist_lead=hd)):
        rc, msg = call(**kw)
        assert rc == -1 and msg, kw
    assert call(**none)[0] == 0 and call(n_scripts=1)[0] == 0 and call(K=0)[0] == 0 and call(W=6)[0] == 0
    assert call(W=1)[0] == 0 and call(lead_range=1.0e-3)[0] == 0 and call(actors=wide, A=15, K=1)[0] == 0
    assert call(n_hist=2, egos=[2, 0], hist_x=hx, hist_slab=hl, hist_lead=hd)[0] == 0
    assert call(K=0, n_hist=2, egos=[0, 1], hist_x=hx, **none)[0] == 0
    assert call(B=0, **none)[0] == 0 and call(B=0, n_scripts=1)[0] == 0 and call(B=0, W=256, K=16, **none)[0] == 0
    r0 = slv.closed_loop_convoy(np.empty((0, 5)), 4, 2, max_steps=10, s_stop=SC.S_STOP)
    assert r0["quant"].shape == (0, 13) and r0["extra"].shape == (0, 6) and r0["hist_lead"].shape == (0, 10, 2)


def check_pack_sweep(env):
    """shard.pack_sweep takes a convoy result as it stands and round-trips through unpack_closed_loop."""
    shard, traj, slv = env["shard"], env["traj"], env["solver"]()
    x_init = plain_starts(traj)[:6]
    ms, rows, he = 40, 8, 2
    cv = slv.closed_loop_convoy(x_init, 3, 2, max_steps=ms, s_stop=S_STOP_R, hist_egos=[4, 2], lo=10)
    q, hist = shard.unpack_closed_loop(shard.pack_sweep(cv, rows, he, ms), rows, he, ms)
    assert SC.same(q, cv["quant"][:, :11]) and q[:, 0].tolist() == [10.0 + b for b in range(6)]
    assert hist.shape == (he, ms, shard.HIST_COLS)
    assert SC.same(hist[:, :, :5], cv["hist_x"][:, 1:].astype(np.float32))
    assert SC.same(hist[:, :, 5:], cv["hist_u"].astype(np.float32))
    assert np.isfinite(cv["quant"][:, 9]).any()


def check_long_cap(env):
    """max_steps = 50 000 with a stop a few metres ahead, B = 512, W = 64, no history: allocates and returns; four
    egos are checked against a 60-step run of their world.  The egos of a world stand within 6 m and see leaders
    within 5 cm only (the tie pair at the start, whoever closes up later), so nobody waits for a queue to dissolve;
    the 60-step runs come first and show that every world ends inside them."""
    traj, slv = env["traj"], env["solver"]()
    B, W, K, lead_range = 512, 64, 2, 0.05
    s_stop = S0 + 8.0
    x_init = np.concatenate([permuted_starts(traj, W, 40 + w, spacing=6.0 / W, v=5.0 + 0.5 * w) for w in range(B // W)])
    short = [slv.closed_loop_convoy(x_init[w * W:(w + 1) * W], W, K, lead_range=lead_range, max_steps=60, s_stop=s_stop)
             for w in range(B // W)]
    assert all((r["n_steps"] < 60).all() for r in short)
    cv = slv.closed_loop_convoy(x_init, W, K, lead_range=lead_range, max_steps=50000, s_stop=s_stop)
    assert cv["hist_x"].shape[0] == 0 and cv["step_ms"].shape == (50000,) and cv["hist_lead"].shape == (0, 50000, K)
    assert (cv["n_steps"] > 0).all() and (cv["n_steps"] < 60).all()
    assert np.isfinite(cv["step_ms"][:cv["n_steps"].max()]).all() and np.isnan(cv["step_ms"][64:]).all()
    assert cv["extra"][:, 5].max() >= 1
    for b in (0, 1, B // 2, B - 1):
        w = b // W
        r1 = short[w]
        i = b - w * W
        assert int(cv["n_steps"][b]) == int(r1["n_steps"][i])
        assert SC.same(cv["quant"][b, QCOLS], r1["quant"][i, QCOLS])
        e1 = r1["extra"][i].copy()
        e1[4] += w * W if e1[4] >= 0 else 0
        assert SC.same(cv["extra"][b], e1)
    SC.assert_step_time_column(cv)
