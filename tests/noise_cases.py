"""Shared pieces of the disturbance-sweep tests (test_noise_cpu.py on the host backend, test_gpu_noise.py on the
device): a stepwise restatement of mpc_closed_loop_noisy built from pinned code (the numpy Philox of
trajectory_tracking.noise_variates, the pinned TrafficScript, convoy_cases' brute-force leader choice,
Solver.solve_batch on a context with max_obs = A + K, the plant in numpy), and the comparisons.  Every comparison
is bit for bit (sweep_cases.same): the restatement runs the same solver on the same perturbed inputs and uses
integer arithmetic and single rounded FP64 operations for the noise.  Trajectory2, N = 20, step caps of 24 (two of
the every-8-steps list compactions)."""
import ctypes

import numpy as np

import convoy_cases as CC
import sweep_cases as SC
import traffic_cases as TC

S0 = SC.S0
QCOLS = TC.QCOLS
STEPS = 24
S_STOP = S0 + 60.0
HISTS = CC.HISTS + ("hist_ua", "hist_xm")
FIELDS = (("meas_sigma", 5), ("act_sigma", 2), ("proc_sigma", 5), ("perc_sigma", 2))

# three known answers of Philox4x32-10: (counter, key, words)
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def states_before(r):
    """hist_x without each ego's final state: the states the steps started from, [n_hist, max_steps, 5], NaN from
    n_steps on (what hist_xm is when nothing is measured with noise)."""
    hx = r["hist_x"][:, :-1].copy()
    ns = r["n_steps"][r["hist_egos"]]
    hx[np.arange(hx.shape[1])[None, :] >= ns[:, None]] = np.nan
    return hx


def sigmas(nz):
    """The 14 sigmas of an MpcNoise as a dict of lists."""
    return {f: [float(v) for v in getattr(nz, f)] for f, _ in FIELDS}


def mild(mpcqp, scale=1.0):
    """Every channel on, small against the state it perturbs: the tracker keeps solving."""
    return mpcqp.default_noise(meas_sigma=np.array([0.05, 0.02, 0.005, 0.0005, 0.05]) * scale,
                               act_sigma=np.array([0.02, 0.2]) * scale,
                               proc_sigma=np.array([0.02, 0.01, 0.005, 0.0005, 0.05]) * scale,
                               perc_sigma=np.array([0.3, 0.2]) * scale)


# ---------------------------------------------------------------------------------------------
# the stepwise restatement
# ---------------------------------------------------------------------------------------------
def driver(env, x_init, W, K, lead_range, scripts, noise, seed, lo, max_steps, s_stop):
    """mpc_closed_loop_noisy restated for B egos in worlds of W.  scripts: None or one list of actors of length A
    per ego; noise: one MpcNoise per ego.  Returns closed_loop_noisy's dict with every ego's history kept
    (step_ms excepted, quant columns 0 and 8 at 0), the index columns without `lo`."""
    TT, mpcqp, shard = env["TT"], env["mpcqp"], env["shard"]
    x = np.array(x_init, np.float64).reshape(-1, 5)
    B = x.shape[0]
    scripts = [[] for _ in range(B)] if scripts is None else scripts
    A = len(scripts[0])
    AK = A + K
    with_slab = (K > 0 and W > 1) or any(a.kind != mpcqp.ACTOR_NONE for scr in scripts for a in scr)
    slv = env["solver"](max_obs=AK if with_slab else 0)
    p = slv.params
    dt, u_lo, u_hi = p.dt, list(p.u_min), list(p.u_max)
    assert len(noise) == B and all(len(s) == A for s in scripts) and B % W == 0
    sg = [sigmas(nz) for nz in noise]
    fsms = [TT.TrafficScript(scr) for scr in scripts]

    hx = np.full((B, max_steps + 1, 5), np.nan); hu = np.full((B, max_steps, 2), np.nan)
    ha = np.full((B, max_steps, 2), np.nan); hm = np.full((B, max_steps, 5), np.nan)
    hc = np.full((B, max_steps), np.nan); hl = np.full((B, max_steps, AK, 2), np.nan)
    ht = np.full((B, max_steps), -1, np.int32); hs = np.full((B, max_steps), -1, np.int32)
    hn = np.full((B, max_steps), -1, np.int32); hd = np.full((B, max_steps, K), -1, np.int32)
    who = np.full((B, max_steps, AK), -1, np.int32)
    ns = np.zeros(B, np.int32)
    n_clamped = np.zeros(B)
    hx[:, 0] = x
    active = x[:, 0] <= s_stop
    for step in range(max_steps):
        idx = np.flatnonzero(active)
        if idx.size == 0:
            break
        lead = CC.leaders(x[:, 0], active, W, K, lead_range)          # on the true positions
        # every draw of this step: [ego, channel]
        zs = TT.noise_variates(seed, lo + np.arange(B, dtype=np.int64)[:, None], step, np.arange(48)[None, :])[1]
        z = lambda b, step, channel: float(zs[b, channel])
        xm = np.zeros((idx.size, 5)); slab = np.zeros((idx.size, AK, 2)); nobs = np.zeros(idx.size, np.int32)
        for i, b in enumerate(idx):
            obs, states = fsms[b].update(dt, x[b, 0], x[b, 4])       # on the true state
            green = 0
            for a, act in enumerate(scripts[b]):
                if act.kind == mpcqp.ACTOR_LIGHT and states[a] == "GREEN":
                    green |= 1 << a
            # the cars emit in actor order: the actor behind each car entry
            on_road = iter([a for a, act in enumerate(scripts[b]) if act.kind == mpcqp.ACTOR_CAR and states[a] == "ACTIVE"])
            for j, o in enumerate(obs):
                if o["type"] == "car":
                    who[b, step, j] = next(on_road)
            true = [(o["s"], o["v"]) for o in obs]
            cars = [o["s"] for o in obs if o["type"] == "car"]
            for m, jj in enumerate(lead[b]):
                true.append((x[jj, 0], x[jj, 4]))
                who[b, step, len(true) - 1] = CC.LEADER
                hd[b, step, m] = jj
            n = len(true)
            nobs[i] = n
            hc[b, step] = cars[0] if cars else np.nan
            ht[b, step], hn[b, step] = green, n
            if n:
                hl[b, step, :n] = true
            # what the solver receives
            for c in range(5):
                xm[i, c] = x[b, c]
                if sg[b]["meas_sigma"][c] != 0.0:
                    xm[i, c] = x[b, c] + sg[b]["meas_sigma"][c] * z(b, step, c)
            hm[b, step] = xm[i]
            for e, (os_, ov) in enumerate(true):
                if sg[b]["perc_sigma"][0] != 0.0:
                    os_ = os_ + sg[b]["perc_sigma"][0] * z(b, step, 16 + 2 * e)
                if sg[b]["perc_sigma"][1] != 0.0:
                    ov = ov + sg[b]["perc_sigma"][1] * z(b, step, 17 + 2 * e)
                slab[i, e] = (os_, ov)
        r = slv.solve_batch(xm, slab, nobs) if with_slab else slv.solve_batch(xm)
        k_ref = slv.lookup(x[idx, 0])[0][:, 3]                        # at the true s
        for i, b in enumerate(idx):
            s, d, o, k, v = x[b]
            u = r["u0"][i]
            ua = [float(u[0]), float(u[1])]
            hit = False
            for c in range(2):
                if sg[b]["act_sigma"][c] != 0.0:
                    t = ua[c] + sg[b]["act_sigma"][c] * z(b, step, 5 + c)
                    ua[c] = u_lo[c] if t < u_lo[c] else (u_hi[c] if t > u_hi[c] else t)
                    hit = hit or t < u_lo[c] or t > u_hi[c]
            n_clamped[b] += hit
            xn = x[b] + dt * np.array([v, v * o, v * (k - k_ref[i]), ua[0], ua[1]])
            for c in range(5):
                if sg[b]["proc_sigma"][c] != 0.0:
                    xn[c] = xn[c] + (dt * sg[b]["proc_sigma"][c]) * z(b, step, 7 + c)
            x[b] = xn
            hx[b, step + 1], hu[b, step], ha[b, step], hs[b, step] = x[b], u, ua, r["status"][i]
            ns[b] = step + 1
            if not x[b, 0] <= s_stop:
                active[b] = False
    out = dict(n_steps=ns, hist_x=hx, hist_u=hu, hist_ua=ha, hist_xm=hm, hist_car_s=hc, hist_tl=ht, hist_status=hs,
               hist_nobs=hn, hist_slab=hl, hist_lead=hd, hist_egos=np.arange(B))
    quant, ex3 = TC.quantities(mpcqp, shard, out, who, scripts)
    ex3[ex3[:, 2] == CC.LEADER, 2] = -1.0
    applied = np.zeros((B, 5))
    for b in range(B):
        n = int(ns[b])
        if n:
            applied[b] = (ha[b, :n, 0].min(), ha[b, :n, 0].max(), ha[b, :n, 1].min(), ha[b, :n, 1].max(), n_clamped[b])
    out["quant"] = quant
    lead_ex = CC.lead_extras(hx, hd, ns) if K else np.tile([np.nan, -1.0, 0.0], (B, 1))
    out["extra"] = np.concatenate([ex3, lead_ex, applied], axis=1)
    return out


def assert_equals_driver(nz, d, lo=0):
    """Every output of closed_loop_noisy with every ego kept equals the restatement."""
    assert np.array_equal(nz["n_steps"], d["n_steps"])
    for name in HISTS:
        assert nz[name].shape == d[name].shape, name
        for b in range(d["n_steps"].size):
            assert SC.same(nz[name][b].astype(np.float64), d[name][b].astype(np.float64)), (name, b)
    assert SC.same(nz["quant"][:, QCOLS], d["quant"][:, QCOLS]), (nz["quant"], d["quant"])
    ex = d["extra"].copy()
    ex[:, 4] += np.where(ex[:, 4] >= 0, lo, 0)
    assert SC.same(nz["extra"], ex), (nz["extra"], ex)
    assert np.array_equal(nz["quant"][:, 0], lo + np.arange(d["n_steps"].size, dtype=np.float64))
    SC.assert_step_time_column(nz)


def one_script(mpcqp, s=S0):
    """One car from the first step on, 25 m ahead of an ego that starts at s, and one light."""
    return [mpcqp.car(S0 - 1.0, s + 25.0, 4.0, TC.FAR), mpcqp.light(S0 + 45.0, 100.0, 1.0)]


def restatement_cases(mpcqp, traj):
    """name -> dict(x_init, W, K, lead_range, scripts, noise (one per ego), seed, lo, max_steps, s_stop)."""
    ego = CC.ego
    cases = {}
    # W = 1, one scripted car and one light; egos 1 and 4 start so close to s_stop that they leave within the
    # first 8 steps: the list is compacted at step 7 while the others run on
    x = np.array([ego(traj, S0), ego(traj, S_STOP - 4.0), ego(traj, S0 + 3.0, v=7.0, d=0.2), ego(traj, S0 + 8.0),
                  ego(traj, S_STOP - 9.0, v=8.0), ego(traj, S0 + 12.0, d=-0.1)])
    cases["car_and_light"] = dict(x_init=x, W=1, K=0, lead_range=np.inf, scripts=[one_script(mpcqp, s) for s in x[:, 0]],
                                  noise=[mild(mpcqp)] * 6, seed=7, lo=0, max_steps=STEPS, s_stop=S_STOP)
    # two worlds of three with two leaders each, no script, a 64-bit seed and a shard offset past 2^32
    x = np.array([ego(traj, S0 + 9.0 * i) for i in range(3)] + [ego(traj, S0 + 6.0 * i, v=8.0) for i in range(3)])
    cases["convoy"] = dict(x_init=x, W=3, K=2, lead_range=np.inf, scripts=None, noise=[mild(mpcqp)] * 6,
                           seed=0xfedcba9876543210, lo=2 ** 32 + 3, max_steps=STEPS, s_stop=S_STOP)
    # per-ego noise: egos 0 and 15 all-zero, egos 1..14 with a single sigma on, one field after the other
    one = mild(mpcqp, 2.0)
    noise = [mpcqp.default_noise()]
    for f, n in FIELDS:
        for c in range(n):
            v = [0.0] * n
            v[c] = getattr(one, f)[c]
            noise.append(mpcqp.default_noise(**{f: v}))
    noise.append(mpcqp.default_noise())
    x = np.array([ego(traj, S0 + 0.5 * i, d=0.01 * (i % 3)) for i in range(16)])
    cases["single_channels"] = dict(x_init=x, W=1, K=0, lead_range=np.inf, scripts=[one_script(mpcqp)] * 16,
                                    noise=noise, seed=11, lo=5, max_steps=STEPS, s_stop=S_STOP)
    # B = 257: a second workgroup of the one-thread-per-ego kernels with a single lane in it; 10 steps
    x = np.array([ego(traj, S0 + 0.1 * i, d=0.01 * (i % 3), v=6.0 + 0.01 * i) for i in range(257)])
    x[100, 0] = x[256, 0] = S_STOP - 3.0                      # two of them leave before the first compaction
    cases["b257"] = dict(x_init=x, W=1, K=0, lead_range=np.inf, scripts=[[mpcqp.car(S0 - 1.0, S0 + 40.0, 5.0, TC.FAR)]] * 257,
                         noise=[mild(mpcqp)] * 257, seed=3, lo=0, max_steps=10, s_stop=S_STOP)
    # an actuator so sloppy that the clamp fires
    x = np.array([ego(traj, S0 + 2.0 * i) for i in range(4)])
    cases["clamp"] = dict(x_init=x, W=2, K=1, lead_range=np.inf, scripts=None,
                          noise=[mpcqp.default_noise(act_sigma=[0.6, 6.0])] * 4, seed=99, lo=0, max_steps=STEPS,
                          s_stop=S_STOP)
    return cases


CASES = ("car_and_light", "convoy", "single_channels", "b257", "clamp")


def assert_case_shape(name, case, d):
    """The restatement itself shows what each case is for (a failure here means the inputs are wrong)."""
    ns, ms = d["n_steps"], case["max_steps"]
    if name == "car_and_light":
        assert ns[1] < 8 and ns[4] < 8 and (ns[[0, 2, 3, 5]] == ms).all()
        assert d["hist_nobs"][0, 0] == 2 and d["hist_car_s"][0, 0] == S0 + 25.0 + 4.0 * 0.2 and d["quant"][1, 10] == 1.0
        assert not SC.same(d["hist_ua"][0, :ns[0]], d["hist_u"][0, :ns[0]])
        assert not SC.same(d["hist_xm"][0, :ns[0]], d["hist_x"][0, :ns[0]])
    if name == "convoy":
        assert d["hist_lead"][0, 0].tolist() == [1, 2] and d["extra"][:, 5].max() == 2.0
    if name == "single_channels":
        ex = d["extra"]
        assert SC.same(d["hist_ua"][0], d["hist_u"][0]) and SC.same(d["hist_xm"][15], d["hist_x"][15, :-1])
        for b in range(1, 6):                                   # one measured component differs, the rest are true
            diff = (d["hist_xm"][b, :ns[b]] != d["hist_x"][b, :ns[b]]).any(axis=0)
            assert diff.tolist() == [c == b - 1 for c in range(5)], b
        for b, c in ((6, 0), (7, 1)):                           # one applied control differs
            diff = (d["hist_ua"][b, :ns[b]] != d["hist_u"][b, :ns[b]]).any(axis=0)
            assert diff.tolist() == [c == 0, c == 1], b
        for b in list(range(8, 15)):                            # process and perception: the solver's view is true
            assert SC.same(d["hist_ua"][b], d["hist_u"][b])
        for b in (13, 14):
            assert SC.same(d["hist_xm"][b], d["hist_x"][b, :-1])
        assert (ex[[0, 15], 10] == 0).all() and SC.same(ex[0, 6:10], d["quant"][0, 4:8])
    if name == "b257":
        assert ns[100] < 8 and ns[256] < 8 and (np.delete(ns, [100, 256]) == ms).all()
    if name == "clamp":
        assert (d["extra"][:, 10] > 0).all(), d["extra"][:, 10]
        p = case["bounds"]
        assert d["extra"][:, 6].min() == p[0][0] and d["extra"][:, 9].max() == p[1][1]
        assert (d["hist_ua"][:, :, 0][~np.isnan(d["hist_ua"][:, :, 0])] <= p[1][0]).all()


def restatement(env, name):
    mpcqp = env["mpcqp"]
    case = restatement_cases(mpcqp, env["traj"])[name]
    p = env["solver"]().params
    case["bounds"] = (list(p.u_min), list(p.u_max))
    d = driver(env, **{k: v for k, v in case.items() if k != "bounds"})
    assert_case_shape(name, case, d)
    return case, d


def check_restatement(env, name):
    case, d = restatement(env, name)
    B = case["x_init"].shape[0]
    nz = env["solver"]().closed_loop_noisy(case["x_init"], case["W"], case["K"], lead_range=case["lead_range"],
                                           scripts=case["scripts"], max_steps=case["max_steps"],
                                           s_stop=case["s_stop"], hist_egos=range(B), noise=case["noise"],
                                           seed=case["seed"], lo=case["lo"])
    assert_equals_driver(nz, d, case["lo"])


# ---------------------------------------------------------------------------------------------
# the noise source
# ---------------------------------------------------------------------------------------------
def check_known_answers(env):
    """The three known answers on the numpy restatement; the one whose counter the channel range allows through
    mpc_noise_draw; a grid and n = 257 against noise_variates, words and z bit for bit."""
    TT, slv = env["TT"], env["solver"]()
    for counter, key, words in KAT:
        assert TT.philox4x32(counter, key).tolist() == list(words)
    # counter (0, 0, 0, 0), key (0, 0): seed 0, ego 0, step 0, channel 0
    w, z = slv.noise_draw(0, [0], [0], [0])
    assert w[0].tolist() == list(KAT[0][2])
    assert z[0] == (sum(KAT[0][2]) - 8589934590.0) * (1.7320508075688772 * 2.0 ** -32)
    # the other two have channels outside 0 .. 47 (and egos past 2^63): through noise_variates' packing only
    for counter, key, words in KAT[1:]:
        w, _ = TT.noise_variates(key[0] | (key[1] << 32), counter[0] | (counter[1] << 32), counter[2], counter[3])
        assert w.tolist() == list(words)
    egos = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7, 2 ** 62], np.int64)
    steps = np.array([0, 1, 23, 2 ** 31 - 1], np.int32)
    chans = np.array([0, 4, 5, 6, 7, 11, 16, 17, 46, 47], np.int32)
    E, S, Cn = (a.ravel() for a in np.meshgrid(egos, steps, chans, indexing="ij"))
    for seed in (0, 1, 2 ** 32 + 5, 2 ** 64 - 1):
        w, z = slv.noise_draw(seed, E, S, Cn)
        wr, zr = TT.noise_variates(seed, E, S, Cn)
        assert w.dtype == np.uint32 and np.array_equal(w, wr) and np.array_equal(z, zr), seed
    e257 = np.arange(257, dtype=np.int64) + 2 ** 32 - 100
    w, z = slv.noise_draw(12345678901234567, e257, 7, 13)
    wr, zr = TT.noise_variates(12345678901234567, e257, 7, 13)
    assert w.shape == (257, 4) and np.array_equal(w, wr) and np.array_equal(z, zr)


def check_distribution(env):
    """65 536 draws on the numpy restatement and on the backend alike: |mean| <= 0.02 (five standard errors of
    1/256), |var - 1| <= 0.03 (the standard error of z^2 is about 0.0051 at the Irwin-Hall(4) kurtosis of 2.7),
    max |z| <= 2 sqrt(3); the 48 channels of one (ego, step) differ."""
    TT, slv = env["TT"], env["solver"]()
    ego = np.arange(65536, dtype=np.int64)
    for z in (TT.noise_variates(2024, ego, 3, 5)[1], slv.noise_draw(2024, ego, 3, 5)[1]):
        assert z.shape == (65536,)
        assert abs(z.mean()) <= 0.02, z.mean()
        assert abs(z.var() - 1.0) <= 0.03, z.var()
        assert np.abs(z).max() <= 2.0 * np.sqrt(3.0)
    ch = np.arange(48, dtype=np.int32)
    for z in (TT.noise_variates(2024, 17, 3, ch)[1], slv.noise_draw(2024, 17, 3, ch)[1]):
        assert np.unique(z).size == 48


# ---------------------------------------------------------------------------------------------
# the other shared bodies
# ---------------------------------------------------------------------------------------------
def check_anchor(env):
    """noise = None, a shared all-zero struct and per-ego all-zero structs: mpc_closed_loop_convoy on every array
    the convoy has, and the new outputs say that nothing was perturbed."""
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"]()
    ego = CC.ego
    x_init = np.array([ego(traj, S0 + 7.0 * i, d=0.01 * (i % 3)) for i in range(5)] + [ego(traj, S_STOP - 5.0)] +
                      [ego(traj, S0 + 4.0 * i, v=7.0) for i in range(5)] + [ego(traj, S_STOP + 2.0)])
    B, W, K = 12, 6, 2
    scripts = [one_script(mpcqp)] * B
    kw = dict(lead_range=40.0, scripts=scripts, max_steps=STEPS, s_stop=S_STOP, hist_egos=range(B))
    cv = slv.closed_loop_convoy(x_init, W, K, **kw)
    assert cv["n_steps"][5] < 8 and cv["n_steps"][11] == 0 and cv["extra"][:, 5].max() == 2.0
    zero = mpcqp.default_noise()
    for noise in (None, zero, [mpcqp.default_noise() for _ in range(B)]):
        nz = slv.closed_loop_noisy(x_init, W, K, noise=noise, seed=123, lo=0, **kw)
        assert np.array_equal(nz["n_steps"], cv["n_steps"])
        assert SC.same(nz["quant"][:, QCOLS], cv["quant"][:, QCOLS]) and SC.same(nz["extra"][:, :6], cv["extra"])
        for name in CC.HISTS:
            assert SC.same(nz[name].astype(np.float64), cv[name].astype(np.float64)), name
        assert SC.same(nz["hist_ua"], nz["hist_u"]) and SC.same(nz["hist_xm"], states_before(nz))
        assert SC.same(nz["extra"][:, 6:10], nz["quant"][:, 4:8]) and (nz["extra"][:, 10] == 0.0).all()
        assert nz["extra"].shape == (B, 11) and len(mpcqp.NZX_FIELDS) == 11
        SC.assert_step_time_column(nz)


def assert_row(a, i, b, j, shift=0):
    """Ego i of run a == ego j of run b (W = 1: no index columns but the ego id)."""
    assert a["n_steps"][i] == b["n_steps"][j]
    assert SC.same(a["quant"][i, QCOLS], b["quant"][j, QCOLS]) and SC.same(a["extra"][i], b["extra"][j])
    assert a["quant"][i, 0] == b["quant"][j, 0] + shift
    for name in HISTS:
        assert SC.same(a[name][i].astype(np.float64), b[name][j].astype(np.float64)), name


def check_composition(env):
    """W = 1: an ego's row depends on (seed, global index, its own start and script) only."""
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"]()
    B = 8
    x_init = SC.starts(traj, B, spread=2.0)
    x_init[3, 0] = S_STOP - 4.0                                # one ego leaves early: the list is compacted
    kw = dict(scripts=[one_script(mpcqp)] * B, max_steps=STEPS, s_stop=S_STOP, noise=mild(mpcqp), seed=42)
    sub = lambda idx: dict(kw, scripts=[kw["scripts"][i] for i in idx])
    whole = slv.closed_loop_noisy(x_init, hist_egos=range(B), **kw)
    assert whole["n_steps"][3] < 8 and whole["n_steps"].max() == STEPS
    again = slv.closed_loop_noisy(x_init, hist_egos=range(B), **kw)
    for i in range(B):
        assert_row(again, i, whole, i)
    for g in (0, 3, 7):                                        # ego g alone, as global ego g
        solo = slv.closed_loop_noisy(x_init[g:g + 1], hist_egos=[0], lo=g, **sub([g]))
        assert_row(solo, 0, whole, g)
    half = [slv.closed_loop_noisy(x_init[lo:lo + B // 2], hist_egos=range(B // 2), lo=lo, **sub(range(lo, lo + B // 2)))
            for lo in (0, B // 2)]
    for i in range(B):
        assert_row(half[i // (B // 2)], i % (B // 2), whole, i)
    other = slv.closed_loop_noisy(x_init, hist_egos=range(B), **dict(kw, seed=43))
    assert (other["hist_xm"][:, 0] != whole["hist_xm"][:, 0]).all()
    assert SC.same(other["hist_x"][:, 0], whole["hist_x"][:, 0])
    # the other egos of the batch shuffled around ego g, which keeps its place
    g = 5
    perm = np.array([6, 4, 7, 0, 2, 5, 1, 3])
    assert perm[g] == g
    mixed = slv.closed_loop_noisy(x_init[perm], hist_egos=range(B), **kw)
    assert_row(mixed, g, whole, g)
    assert not SC.same(mixed["hist_x"][0], whole["hist_x"][0])


def check_truth_and_perception(env):
    """Only perc_sigma > 0: the world's slab and the leaders are the noise-free convoy run's at step 0, the gap
    quantity comes from the true states, and the solver's step-0 control differs."""
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"]()
    ego = CC.ego
    B, W, K = 4, 2, 1
    x_init = np.array([ego(traj, S0), ego(traj, S0 + 8.0, v=6.0), ego(traj, S0 + 2.0), ego(traj, S0 + 9.0, v=5.0)])
    scripts = [[mpcqp.car(S0 - 1.0, S0 + 20.0, 3.0, TC.FAR)]] * B
    kw = dict(scripts=scripts, max_steps=STEPS, s_stop=S_STOP, hist_egos=range(B))
    cv = slv.closed_loop_convoy(x_init, W, K, **kw)
    nz = slv.closed_loop_noisy(x_init, W, K, noise=mpcqp.default_noise(perc_sigma=[2.0, 1.0]), seed=8, **kw)
    assert SC.same(nz["hist_slab"][:, 0], cv["hist_slab"][:, 0]) and np.array_equal(nz["hist_lead"][:, 0], cv["hist_lead"][:, 0])
    assert np.array_equal(nz["hist_nobs"][:, 0], cv["hist_nobs"][:, 0]) and nz["hist_nobs"][0, 0] == 2
    assert SC.same(nz["hist_xm"], states_before(nz)) and SC.same(nz["hist_ua"], nz["hist_u"])
    assert (nz["hist_u"][:, 0] != cv["hist_u"][:, 0]).any()
    for b in range(B):                                         # every entry here is a car or a leader
        n = int(nz["n_steps"][b])
        gaps = nz["hist_slab"][b, :n, :, 0] - nz["hist_x"][b, :n, 0][:, None]
        assert SC.same(nz["quant"][b, 9], np.nanmin(gaps))
    # the slab entries are the leaders' true states in the run's own histories
    assert nz["hist_lead"][0, 0, 0] == 1 and SC.same(nz["hist_slab"][0, :3, 1], nz["hist_x"][1, :3][:, [0, 4]])


def check_misuse(env):
    """Every misuse case of include/mpcqp.h is MPC_E_ARG with a message; the well-formed neighbours succeed."""
    mpcqp, traj, slv = env["mpcqp"], env["traj"], env["solver"]()
    L = mpcqp.lib()
    assert L.mpc_version() == 5
    B, A, W, K = 6, 2, 3, 2
    x = np.ascontiguousarray(SC.starts(traj, B))
    arr = (mpcqp.MpcActor * (B * A))(*(one_script(mpcqp) * B))
    bad = (mpcqp.MpcActor * (B * A))(*arr)
    bad[3].kind = 3
    wide = (mpcqp.MpcActor * (B * 15))()
    nzs = (mpcqp.MpcNoise * B)(*[mild(mpcqp) for _ in range(B)])
    quant = np.empty((B, 13))
    hx = np.empty((2, 11, 5)); hl = np.empty((2, 10, 16, 2)); hd = np.empty((2, 10, 16), np.int32)
    ha = np.empty((2, 10, 2)); hm = np.empty((2, 10, 5))

    def with_sigma(field, c, v, n=B, at=0):
        out = (mpcqp.MpcNoise * n)(*[mild(mpcqp) for _ in range(n)])
        getattr(out[at], field)[c] = v
        return out

    def call(B=B, W=W, K=K, lead_range=np.inf, actors=arr, A=A, n_scripts=B, noise=nzs, n_noise=B, seed=1,
             ego_offset=0, q=quant, n_hist=0, egos=None, hist_x=None, hist_ua=None, hist_xm=None, hist_slab=None,
             hist_lead=None):
        he = None if egos is None else np.asarray(egos, np.int32)
        rc = L.mpc_closed_loop_noisy(slv.h, B, W, K, lead_range, mpcqp._p(x), actors, A, n_scripts, noise, n_noise,
                                     seed, ego_offset, 10, SC.S_STOP, mpcqp._p(q), None, n_hist, mpcqp._pi(he),
                                     mpcqp._p(hist_x), None, mpcqp._p(hist_ua), mpcqp._p(hist_xm), None, None, None,
                                     None, mpcqp._p(hist_slab), mpcqp._pi(hist_lead), None, None)
        return rc, mpcqp.last_error()

    assert call()[0] == 0                                        # the well-formed call these cases depart from
    none = dict(actors=None, A=0, n_scripts=0)
    convoy_cases = (dict(A=-1), dict(A=17), dict(n_scripts=2), dict(n_scripts=0), dict(actors=None, n_scripts=1),
                    dict(actors=None, n_scripts=B), dict(actors=None, n_scripts=0), dict(actors=bad), dict(q=None),
                    dict(n_hist=-1), dict(n_hist=0, hist_x=hx), dict(n_hist=0, hist_slab=hl),
                    dict(n_hist=2, egos=[1, B], hist_x=hx), dict(n_hist=2, egos=[-1, 2], hist_x=hx),
                    dict(n_hist=2, egos=[1, 1], hist_x=hx), dict(W=0), dict(W=257), dict(W=4), dict(K=-1), dict(K=17),
                    dict(K=15), dict(actors=wide, A=15, K=2), dict(lead_range=0.0), dict(lead_range=np.nan),
                    dict(none, K=0, n_hist=2, egos=[0, 1], hist_slab=hl),
                    dict(K=0, n_hist=2, egos=[0, 1], hist_lead=hd), dict(n_hist=0, hist_lead=hd))
    noise_cases = (dict(noise=with_sigma("meas_sigma", 2, -1.0e-9)), dict(noise=with_sigma("act_sigma", 1, np.nan)),
                   dict(noise=with_sigma("proc_sigma", 4, -1.0, at=B - 1)), dict(noise=with_sigma("perc_sigma", 0, np.nan, at=3)),
                   dict(noise=with_sigma("perc_sigma", 1, -2.0, n=1), n_noise=1),
                   dict(n_noise=2), dict(n_noise=0), dict(n_noise=-1), dict(noise=None, n_noise=1),
                   dict(noise=None, n_noise=B), dict(ego_offset=-1), dict(ego_offset=-2 ** 40),
                   dict(n_hist=0, hist_ua=ha), dict(n_hist=0, hist_xm=hm))
    for kw in convoy_cases + noise_cases:
        rc, msg = call(**kw)
        assert rc == -1 and msg, kw
    assert call(noise=None, n_noise=0)[0] == 0 and call(n_noise=1)[0] == 0 and call(ego_offset=2 ** 40)[0] == 0
    assert call(seed=2 ** 64 - 1)[0] == 0 and call(noise=with_sigma("act_sigma", 0, 0.0))[0] == 0
    assert call(n_hist=2, egos=[2, 0], hist_x=hx, hist_ua=ha, hist_xm=hm, hist_slab=hl, hist_lead=hd)[0] == 0
    assert call(**none)[0] == 0 and call(W=1)[0] == 0 and call(B=0, n_noise=1, **none)[0] == 0
    assert call(B=0, noise=None, n_noise=0, n_scripts=1)[0] == 0
    r0 = slv.closed_loop_noisy(np.empty((0, 5)), 4, 2, max_steps=10, s_stop=SC.S_STOP)
    assert r0["extra"].shape == (0, 11) and r0["hist_ua"].shape == (0, 10, 2) and r0["hist_xm"].shape == (0, 10, 5)
    # mpc_noise_draw: a channel outside 0 .. 47, a negative ego, n < 0, a missing index array
    e1, s1 = (ctypes.c_longlong * 2)(0, 1), (ctypes.c_int * 2)(0, 0)
    w = (ctypes.c_uint * 8)(); z = (ctypes.c_double * 2)()
    for ch in ((0, 48), (-1, 0), (2 ** 31 - 1, 0)):
        assert L.mpc_noise_draw(slv.h, 0, 2, e1, s1, (ctypes.c_int * 2)(*ch), w, z) == -1 and mpcqp.last_error()
    c1 = (ctypes.c_int * 2)(0, 47)
    assert L.mpc_noise_draw(slv.h, 0, 2, (ctypes.c_longlong * 2)(0, -1), s1, c1, w, z) == -1 and mpcqp.last_error()
    assert L.mpc_noise_draw(slv.h, 0, -1, e1, s1, c1, w, z) == -1 and L.mpc_noise_draw(slv.h, 0, 2, e1, None, c1, w, z) == -1
    assert L.mpc_noise_draw(slv.h, 0, 2, e1, s1, c1, w, z) == 0 and L.mpc_noise_draw(slv.h, 0, 2, e1, s1, c1, None, z) == 0
    assert L.mpc_noise_draw(slv.h, 0, 2, e1, s1, c1, w, None) == 0 and L.mpc_noise_draw(slv.h, 0, 0, None, None, None, None, None) == 0
    assert list(w[:4]) == list(KAT[0][2])
