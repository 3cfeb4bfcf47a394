"""GPU tests of the solver kernel instantiations and of the horizons on the lane-group boundaries.

launch_solve (csrc/mpcqp.hip) picks one of the 50 instantiations of mpc_solve_kernel<GL, OBS, MODE, NT>
(csrc/solve_kernel.h; its stage recursions: csrc/riccati_lanes.h) from the
horizon (GL = 16 for N <= 15, 32 for N <= 31, else 64; NT = N at the specialised horizons 20, 30, 40, else 0 =
runtime horizon), from whether obstacles were passed (OBS), from sqp_iters and the batch size (MODE: the split
pair XO + IPM for single-QP solves with two or more instances per wavefront, ONE for the other single-QP
solves, FULL for every other sqp_iters) and from the switches read at mpc_create (MPC_TWO_PHASE,
MPC_STAGE_CACHE, MPC_IPM_GL64).  The tests here run the horizons 15, 16, 31, 32 where the lane group is full
or changes, the runtime-horizon kernels between the specialised ones, the launch paths against each other
(bit identity), batch positions, the MPC_IPM_GL64=1 kernels and the obstacle slab up to MPC_MAX_OBS.

Coverage map: every key (GL, OBS, MODE, NT) of the library and one test that launches it ("here": this file;
parity: test_gpu_parity; entry: test_gpu_device_entry; nlp: test_gpu_nlp).

  key                    launched by
  (16, 0, XO,   0)       here test_horizon_sweep_vs_oracle[C2-15]; parity test_vs_oracle_full_batch[C1]
  (16, 0, IPM,  0)       here test_horizon_sweep_vs_oracle[C2-15]; parity test_vs_oracle_full_batch[C1]
  (16, 0, ONE,  0)       here test_split_pair_equals_one_launch[C2-15]; entry test_two_phase_equals_single_kernel[C2-1024-10]
  (16, 0, FULL, 0)       parity test_closed_loop_config1 (N = 10, the shim's SQP); parity test_predict_matches_reference_model_golden
  (16, 1, XO,   0)       here test_horizon_sweep_vs_oracle[C3-15], [C5-15]; here test_obstacle_slab_edges[10]
  (16, 1, IPM,  0)       here test_horizon_sweep_vs_oracle[C3-15], [C5-15]; here test_obstacle_slab_edges[10]
  (16, 1, ONE,  0)       here test_split_pair_equals_one_launch[C3-15]
  (16, 1, FULL, 0)       nlp test_device_closed_loop_vs_reference_run (N = 5, FSM obstacles); parity test_warm_start_and_predict_bit_exact
  (32, 0, XO,   0)       here test_horizon_sweep_vs_oracle[C2-16|17|25|31]
  (32, 0, IPM,  0)       here test_horizon_sweep_vs_oracle[C2-16|17|25|31]
  (32, 0, ONE,  0)       here test_split_pair_equals_one_launch[C2-16|25|31]
  (32, 0, FULL, 0)       here test_sqp_horizons_vs_oracle[C2-17], [C2-31]
  (32, 1, XO,   0)       here test_horizon_sweep_vs_oracle[C3-16|17|25|31], [C5-16|17|25|31]
  (32, 1, IPM,  0)       here test_horizon_sweep_vs_oracle[C3-16|17|25|31], [C5-16|17|25|31]
  (32, 1, ONE,  0)       here test_split_pair_equals_one_launch[C3-16|25|31]
  (32, 1, FULL, 0)       here test_sqp_horizons_vs_oracle[C3-17], [C3-31]
  (32, 0, XO,   20)      parity test_vs_oracle_full_batch[C2]; here test_stage_cache_on_equals_off[C2-20]
  (32, 0, IPM,  20)      parity test_vs_oracle_full_batch[C2]; here test_stage_cache_on_equals_off[C2-20]
  (32, 0, ONE,  20)      entry test_two_phase_equals_single_kernel[C2-1024-None]
  (32, 0, FULL, 20)      parity test_sqp_relinearisation_vs_oracle[C2-4096-3]
  (32, 1, XO,   20)      parity test_vs_oracle_full_batch[C3]; here test_batch_position_invariance[20]
  (32, 1, IPM,  20)      parity test_vs_oracle_full_batch[C3]; here test_batch_position_invariance[20]
  (32, 1, ONE,  20)      entry test_two_phase_equals_single_kernel[C3-1024-None]
  (32, 1, FULL, 20)      parity test_sqp_relinearisation_vs_oracle[C3-2048-10]
  (32, 0, XO,   30)      here test_specialised_kernels_without_obstacles[30]
  (32, 0, IPM,  30)      here test_specialised_kernels_without_obstacles[30]
  (32, 0, ONE,  30)      here test_specialised_kernels_without_obstacles[30] (its MPC_TWO_PHASE=0 leg)
  (32, 0, FULL, 30)      here test_sqp_horizons_vs_oracle[C4-30-noobs]
  (32, 1, XO,   30)      parity test_vs_oracle_full_batch[C4]
  (32, 1, IPM,  30)      parity test_vs_oracle_full_batch[C4]
  (32, 1, ONE,  30)      entry test_two_phase_equals_single_kernel[C4-1024-None]
  (32, 1, FULL, 30)      parity test_sqp_relinearisation_vs_oracle[C4-1024-10]
  (64, 0, ONE,  0)       here test_horizon_sweep_vs_oracle[C2-32|33|47|63]
  (64, 0, FULL, 0)       here test_sqp_horizons_vs_oracle[C2-33]
  (64, 1, ONE,  0)       here test_horizon_sweep_vs_oracle[C3-32|33|47|63], [C5-32|33|47|63]; parity test_edge_cases (N = 63)
  (64, 1, FULL, 0)       here test_sqp_horizons_vs_oracle[C3-33]
  (64, 0, ONE,  40)      here test_specialised_kernels_without_obstacles[40]
  (64, 0, FULL, 40)      here test_sqp_horizons_vs_oracle[C5-40-noobs]
  (64, 1, ONE,  40)      parity test_vs_oracle_full_batch[C5]; here test_batch_position_invariance[40]
  (64, 1, FULL, 40)      here test_sqp_horizons_vs_oracle[C5-40]
  (64, 0, IPM,  20)      here test_ipm_gl64_vs_oracle_and_default[C2] (MPC_IPM_GL64=1)
  (64, 1, IPM,  20)      here test_ipm_gl64_vs_oracle_and_default[C3] (MPC_IPM_GL64=1)
  unreachable from launch_solve (one instance per wavefront never takes the split launch); they are in the
  library (tests/test_kernel_resources.py pins the count), and nothing can launch them:
  (64, 0, XO,   0)       unreachable
  (64, 1, XO,   0)       unreachable
  (64, 0, XO,   40)      unreachable
  (64, 1, XO,   40)      unreachable
  (64, 0, IPM,  0)       unreachable
  (64, 1, IPM,  0)       unreachable
  (64, 0, IPM,  40)      unreachable
  (64, 1, IPM,  40)      unreachable

Workloads: the generators of workloads.make_batch do not depend on the horizon, so the C2 (traj1, no
obstacles), C3 (traj2, 0-2 FSM obstacles) and C5 (traj3, 8 obstacles) egos are solved at every horizon.
B = 203 = 4 * 50 + 3 leaves a partial last wavefront at 1, 2 and 4 instances per wavefront.
"""
import functools
import os

import numpy as np
import pytest

from conftest import traj_arrays
from test_gpu_device_entry import assert_identical, device_solve, make_solver, to_host
from test_gpu_parity import TOL_U, check_vs_oracle, set_p, tol_u

pytestmark = pytest.mark.gpu

B = 203
SWEEP_N = (15, 16, 17, 25, 31, 32, 33, 47, 63)
# name -> (configuration whose egos and obstacles are generated, seed)
WORKLOADS = {"C2": ("C2", 71), "C3": ("C3", 73), "C4": ("C4", 74), "C5": ("C5", 75)}
KEYS = ("u0", "U", "Xpred", "status", "iters")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import mpcqp
    return mpcqp


@functools.lru_cache(maxsize=None)
def _generated(cfg, seed, nb):
    import workloads as W
    return W.make_batch(cfg, B=nb, seed=seed)


def sweep_batch(name, N, with_obs=True, nb=B):
    """The workload `name` at horizon N (a copy of the dict; the arrays are shared and never written)."""
    wb = dict(_generated(*WORKLOADS[name], nb))
    wb["N"] = int(N)
    if not with_obs:
        wb.update(obs=None, n_obs=None, max_obs=0)
    return wb


@functools.lru_cache(maxsize=None)
def _oracle(traj):
    import oracle as O
    return O.Oracle(*traj_arrays(traj))


@functools.lru_cache(maxsize=None)
def oracle_solve(name, N, sqp=1, with_obs=True, pset=()):
    """(oracle result, ctx of check_vs_oracle) of sweep_batch(name, N, with_obs): computed once per case and
    shared by the tests (read only).  pset: ((field, value), ...) of the mpc_params fields that differ from the
    defaults (hashable: u_min / u_max as tuples)."""
    import oracle as O
    wb = sweep_batch(name, N, with_obs)
    orc = _oracle(wb["traj"])
    po = O.default_params(N=wb["N"], max_obs=wb["max_obs"], sqp_iters=sqp, **dict(pset))
    ro = orc.solve_batch(po, wb["x0"], wb["obs"], wb["n_obs"])
    return ro, (orc, po, wb["x0"], wb["obs"], wb["n_obs"])


def env_solver(lib, traj, env):
    """A GPU context created under the environment switches `env` (read by mpc_create only): set around the
    construction and restored afterwards."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return lib.Solver(*traj_arrays(traj), lib.default_params(), device=0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctxs(lib):
    """get(traj, **env): one context per trajectory and switch setting, shared by the module's tests."""
    made = {}

    def get(traj, **env):
        key = (traj, tuple(sorted(env.items())))
        if key not in made:
            made[key] = env_solver(lib, traj, env)
        return made[key]
    yield get
    for s in made.values():
        s.close()


def solve(lib, slv, wb, **kw):
    set_p(lib, slv, wb["N"], wb["max_obs"], **kw)
    return slv.solve_batch(wb["x0"], wb["obs"], wb["n_obs"])


def assert_sweep_paths(name, N, r):
    """The batch still runs the paths the sweep is there for (the oracle alone meets these on every case:
    33 (C2, N = 63) to 170 (C3, N = 15) crossover-certified instances, 12 to 33 elastic ones)."""
    xo, deferred = int((r["iters"] == 0).sum()), int((r["iters"] > 0).sum())
    elastic = int(((r["status"] & 15) == 2).sum())
    print(f"{name} N={N}: crossover-certified {xo}, deferred {deferred}, elastic {elastic}")
    if name in ("C2", "C3"):
        assert xo >= 30 and deferred >= 30, (name, N, xo, deferred)
        assert elastic >= 12, (name, N, elastic)
    elif name == "C5" and N <= 33:
        assert xo >= 1 and deferred >= 1, (name, N, xo, deferred)


# ---------------------------------------------------------------------------------------------------------
# 1. horizons against the oracle
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SWEEP_N)
@pytest.mark.parametrize("name", ["C2", "C3", "C5"])
def test_horizon_sweep_vs_oracle(lib, ctxs, name, N):
    """Default launch (the split pair for N <= 31, MODE_ONE above) at the lane-group boundaries 15 | 16 and
    31 | 32, at runtime horizons between the specialised ones and at the longest one: GPU == oracle to tol_u(N)."""
    wb = sweep_batch(name, N)
    r = solve(lib, ctxs(wb["traj"]), wb)
    ro, ctx = oracle_solve(name, N)
    check_vs_oracle(r, ro, ctx=ctx, label=f"sweep {name} N={N}", tol=tol_u(N))
    assert np.array_equal(r["u0"], r["U"][:, 0, :])
    assert np.isfinite(r["Xpred"]).all()
    assert_sweep_paths(name, N, r)


def test_sweep_runs_full_and_spare_last_ipm_wave(lib, ctxs):
    """The interior-point launch of the split pair runs with an even and with an odd number of deferred
    instances (two per wavefront at these horizons), so with a full last wave and with one whose spare group
    repeats the last record (oracle: 46 deferred on C2 at N = 16, 47 at N = 17)."""
    par = set()
    for N in (16, 17):
        wb = sweep_batch("C2", N)
        r = solve(lib, ctxs(wb["traj"]), wb)
        n = int((r["iters"] > 0).sum())
        print(f"C2 N={N}: {n} deferred")
        par.add(n % 2)
    assert par == {0, 1}


SQP_CASES = [("C2", 17, True), ("C2", 31, True), ("C2", 33, True), ("C3", 17, True), ("C3", 31, True),
             ("C3", 33, True), ("C4", 30, False), ("C5", 40, False), ("C5", 40, True)]


def last_linearisation_point(name, N, sqp, with_obs, pset=()):
    """[B, N, 2]: the point each instance's last QP was linearised at in the oracle's run of at most `sqp` QPs:
    the warm start, or U after k QPs wherever QP k + 1 still ran (the run capped at k + 1 returns another U)."""
    _, (orc, po, x0, obs, n_obs) = oracle_solve(name, N, 1, with_obs, pset)
    ub = np.stack([orc.warm_start(po, x0[i], None if obs is None else obs[i, :n_obs[i]]) for i in range(len(x0))])
    ub = ub.reshape(len(x0), N, 2)
    for k in range(1, sqp):
        uk, uk1 = (oracle_solve(name, N, j, with_obs, pset)[0]["U"] for j in (k, k + 1))
        ran = (uk != uk1).reshape(len(x0), -1).any(axis=1)
        ub[ran] = uk[ran]
    return ub


@pytest.mark.parametrize("name,N,with_obs", SQP_CASES,
                         ids=[f"{n}-{N}" + ("" if w else "-noobs") for n, N, w in SQP_CASES])
def test_sqp_horizons_vs_oracle(lib, ctxs, name, N, with_obs):
    """sqp_iters = 3 (MODE_FULL) at runtime horizons either side of the 31 | 32 boundary, and the specialised
    N = 30 and N = 40 kernels with and without obstacles; the bar of test_sqp_relinearisation_vs_oracle.
    check_vs_oracle gets the last QP's linearisation point, so that an infeasible / numerical status flip is
    judged by the elastic objective of that QP as in the single-QP tests (C2 at N = 33 has one: the oracle's
    last interior point ends "numerical" on an elastic instance that the GPU certifies)."""
    wb = sweep_batch(name, N, with_obs)
    r = solve(lib, ctxs(wb["traj"]), wb, sqp_iters=3)
    ro, ctx = oracle_solve(name, N, 3, with_obs)
    ctx = ctx + (last_linearisation_point(name, N, 3, with_obs),)
    s = check_vs_oracle(r, ro, ctx=ctx, label=f"SQP {name} N={N} obs={with_obs}", tol=1e-8, xtol=1e-7)
    assert s["elastic_alt_optima"] == 0       # as without the context: U within tol wherever both certified
    assert (r["iters"] >= 0).all()


@pytest.mark.parametrize("N", [30, 40])
def test_specialised_kernels_without_obstacles(lib, ctxs, N):
    """The OBS = false kernels of the specialised horizons 30 and 40 (the configurations that use these horizons
    always carry obstacles): GPU == oracle; at N = 30 the one-launch kernel equals the split pair bit for bit."""
    name = "C4" if N == 30 else "C5"
    wb = sweep_batch(name, N, with_obs=False)
    r = solve(lib, ctxs(wb["traj"]), wb)
    ro, ctx = oracle_solve(name, N, 1, False)
    check_vs_oracle(r, ro, ctx=ctx, label=f"no obstacles {name} N={N}", tol=tol_u(N))
    assert (r["iters"] == 0).any() and (r["iters"] > 0).any()
    if N == 30:
        r1 = solve(lib, ctxs(wb["traj"], MPC_TWO_PHASE=0), wb)
        assert_identical(r, r1, "split pair vs one launch")


# ---------------------------------------------------------------------------------------------------------
# 2. launch paths give the same bits
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [15, 16, 25, 31])
@pytest.mark.parametrize("name", ["C2", "C3"])
def test_split_pair_equals_one_launch(lib, ctxs, name, N):
    """MODE_XO + MODE_IPM == MODE_ONE (MPC_TWO_PHASE=0) on full lane groups (N = 15, 31), on the first horizon of
    the 32-lane group and in between, through the host entry and the device entry."""
    torch = pytest.importorskip("torch")
    wb = sweep_batch(name, N)
    two, one = ctxs(wb["traj"]), ctxs(wb["traj"], MPC_TWO_PHASE=0)
    r2, r1 = solve(lib, two, wb), solve(lib, one, wb)
    assert_identical(r2, r1, "host entry")
    assert (r2["iters"] == 0).any() and (r2["iters"] > 0).any()
    d2, _ = device_solve(two, wb, torch)
    d1, _ = device_solve(one, wb, torch)
    d2, d1 = to_host(d2, torch), to_host(d1, torch)
    assert_identical(d2, d1, "device entry")
    assert_identical(d2, r2, "device vs host entry")


@pytest.mark.parametrize("N", [16, 20, 31])
@pytest.mark.parametrize("name", ["C2", "C3"])
def test_stage_cache_on_equals_off(lib, ctxs, name, N):
    """include/mpcqp.h: a call without the stage cache recomputes the interior point's start bit for bit."""
    wb = sweep_batch(name, N)
    on, off = solve(lib, ctxs(wb["traj"]), wb), solve(lib, ctxs(wb["traj"], MPC_STAGE_CACHE=0), wb)
    assert (on["iters"] > 0).any()
    assert_identical(on, off, f"stage cache on vs off, {name} N={N}")


def test_captured_equals_eager_runtime_horizon(lib):
    """One captured-graph replay of the runtime-horizon 32-lane kernels (N = 25, obstacles) equals the eager
    call (the captured call runs without the stage cache)."""
    torch = pytest.importorskip("torch")
    wb = sweep_batch("C3", 25)
    slv = make_solver(lib, wb["traj"], wb["N"], wb["max_obs"])
    ra = slv.solve_batch(wb["x0"], wb["obs"], wb["n_obs"])
    out, keep = device_solve(slv, wb, torch)                  # eager warm-up (records the ordering event)
    assert_identical(to_host(out, torch), ra, "eager")
    x0, obs, nob = keep
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        slv.solve_batch_device(B, x0.data_ptr(), obs.data_ptr(), nob.data_ptr(), 0, out["u0"].data_ptr(),
                               out["U"].data_ptr(), out["Xpred"].data_ptr(), out["status"].data_ptr(),
                               out["iters"].data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    for k in out:
        out[k].zero_()
    g.replay()
    assert_identical(to_host(out, torch), ra, "replay")
    slv.close()


# ---------------------------------------------------------------------------------------------------------
# 3. batch position
# ---------------------------------------------------------------------------------------------------------
def reorder(wb, idx):
    return dict(wb, x0=wb["x0"][idx], obs=wb["obs"][idx], n_obs=wb["n_obs"][idx])


def check_position_invariance(lib, slv, N):
    wb = sweep_batch("C3", N)
    r = solve(lib, slv, wb)
    for what, idx in (("permuted", np.random.default_rng(N).permutation(B)), ("reversed", np.arange(B)[::-1])):
        rp = solve(lib, slv, reorder(wb, idx))
        assert_identical(rp, {k: r[k][idx] for k in KEYS}, f"N={N} {what}")
    xo, deferred = np.flatnonzero(r["iters"] == 0), np.flatnonzero(r["iters"] > 0)
    assert len(xo) >= 4 and len(deferred) >= 4
    for i in np.concatenate([xo[:4], deferred[:4]]):
        r1 = solve(lib, slv, reorder(wb, slice(i, i + 1)))
        assert_identical(r1, {k: r[k][i:i + 1] for k in KEYS}, f"N={N} instance {i} alone")


@pytest.mark.parametrize("N", [10, 17, 20, 40])
def test_batch_position_invariance(lib, ctxs, N):
    """An instance's outputs do not depend on its place in the batch, on the instances that share its wavefront
    (3 at N = 10, 1 at N = 17 and 20, none at N = 40), on its place in the interior-point launch's work list,
    or on being the only instance of the call (whose spare groups repeat it): bit-identical."""
    check_position_invariance(lib, ctxs(2), N)


def test_batch_position_invariance_ipm_gl64(lib, ctxs):
    """The same with the one-instance-per-wavefront interior-point kernels of MPC_IPM_GL64=1 (N = 20)."""
    check_position_invariance(lib, ctxs(2, MPC_IPM_GL64=1), 20)


# ---------------------------------------------------------------------------------------------------------
# 4. the MPC_IPM_GL64=1 kernels
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C2", "C3"])
def test_ipm_gl64_vs_oracle_and_default(lib, ctxs, name):
    """MPC_IPM_GL64=1 (N = 20: the deferred instances on 64-lane interior-point kernels, one per wavefront):
    GPU == oracle to TOL_U, with the statuses and iteration counts of the default path."""
    wb = sweep_batch(name, 20)
    r = solve(lib, ctxs(wb["traj"], MPC_IPM_GL64=1), wb)
    ro, ctx = oracle_solve(name, 20)
    check_vs_oracle(r, ro, ctx=ctx, label=f"IPM_GL64 {name}", tol=TOL_U)
    rd = solve(lib, ctxs(wb["traj"]), wb)
    assert (r["iters"] > 0).any()
    assert np.array_equal(r["status"], rd["status"]) and np.array_equal(r["iters"], rd["iters"])


@pytest.mark.parametrize("name", ["C2", "C3"])
def test_ipm_gl64_stage_cache_on_equals_off(lib, ctxs, name):
    """The header's claim holds under MPC_IPM_GL64=1 too: without the stage cache the 64-lane interior-point
    kernel recomputes the start in the crossover kernel's solve form, bit for bit."""
    wb = sweep_batch(name, 20)
    on = solve(lib, ctxs(wb["traj"], MPC_IPM_GL64=1), wb)
    off = solve(lib, ctxs(wb["traj"], MPC_IPM_GL64=1, MPC_STAGE_CACHE=0), wb)
    assert (on["iters"] > 0).any()
    assert_identical(on, off, f"IPM_GL64 stage cache on vs off, {name}")


# ---------------------------------------------------------------------------------------------------------
# 5. obstacle slab edges
# ---------------------------------------------------------------------------------------------------------
SLAB_B, SLAB_MAX_OBS = 67, 64


@functools.lru_cache(maxsize=None)
def slab_batch():
    """67 traj3 egos with a 64-row slab: obstacle j at s0 + 12 + 30 j + U(0, 10) with speed U(0, 10), and
    n_obs cycling through 0, 1, 2, 8, 33, 64; the rows at and past n_obs are zeros."""
    wb = dict(_generated("C5", 77, SLAB_B))
    rng = np.random.default_rng(5)
    obs = np.zeros((SLAB_B, SLAB_MAX_OBS, 2))
    obs[..., 0] = (wb["x0"][:, None, 0] + 12.0 + 30.0 * np.arange(SLAB_MAX_OBS)[None, :]
                   + rng.uniform(0.0, 10.0, (SLAB_B, SLAB_MAX_OBS)))
    obs[..., 1] = rng.uniform(0.0, 10.0, (SLAB_B, SLAB_MAX_OBS))
    n_obs = np.array([(0, 1, 2, 8, 33, 64)[b % 6] for b in range(SLAB_B)], np.int32)
    obs[np.arange(SLAB_MAX_OBS)[None, :] >= n_obs[:, None]] = 0.0
    wb.update(obs=obs, n_obs=n_obs, max_obs=SLAB_MAX_OBS)
    return wb


@functools.lru_cache(maxsize=None)
def slab_oracle(N):
    import oracle as O
    wb = slab_batch()
    orc = _oracle(wb["traj"])
    po = O.default_params(N=N, max_obs=SLAB_MAX_OBS)
    return orc.solve_batch(po, wb["x0"], wb["obs"], wb["n_obs"]), (orc, po, wb["x0"], wb["obs"], wb["n_obs"])


@pytest.mark.parametrize("N", [10, 20, 40])
def test_obstacle_slab_edges(lib, ctxs, N):
    """max_obs = MPC_MAX_OBS with n_obs mixed from 0 to 64: GPU == oracle; the rows at and past n_obs are never
    read (NaN there changes no bit); an instance with n_obs = 0 equals its no-obstacle solve."""
    wb = dict(slab_batch(), N=N)
    slv = ctxs(wb["traj"])
    r = solve(lib, slv, wb)
    ro, ctx = slab_oracle(N)
    # what the oracle gives on these inputs: both statuses and both launch phases are well populated
    n0, n2, nxo = (int((ro["status"] == 0).sum()), int((ro["status"] == 2).sum()), int((ro["iters"] == 0).sum()))
    print(f"slab N={N}: oracle status 0: {n0}, status 2: {n2}, crossover-certified {nxo}")
    assert 39 <= n0 <= 41 and 26 <= n2 <= 28 and 13 <= nxo <= 19, (n0, n2, nxo)
    check_vs_oracle(r, ro, ctx=ctx, label=f"slab N={N}", tol=tol_u(N))
    poisoned = wb["obs"].copy()
    poisoned[np.arange(SLAB_MAX_OBS)[None, :] >= wb["n_obs"][:, None]] = np.nan
    rn = solve(lib, slv, dict(wb, obs=poisoned))
    assert_identical(rn, r, f"slab N={N}: NaN past n_obs")
    none = np.flatnonzero(wb["n_obs"] == 0)
    assert len(none) == 12
    r0 = solve(lib, slv, dict(wb, x0=wb["x0"][none], obs=None, n_obs=None, max_obs=0))
    err = float(np.abs(r["U"][none] - r0["U"]).max())
    print(f"slab N={N}: n_obs = 0 vs no-obstacle solve: max|dU| {err:.3e}")
    assert np.array_equal(r["status"][none], r0["status"])
    assert err <= tol_u(N)
