"""First-order optimality of the solver's answers on the reference's own nonlinear problem (mpc_gradient_batch).

For a config of workloads.py (default C2; C3..C5 selectable) the batch is solved twice, once as bench.py does
(sqp_iters = 1: the single tracking QP at the warm start) and once with the drop-in default (the Gauss-Newton SQP,
trajectory_tracking.SQP_ITERS).  For a sample of instances, evenly spaced over the batch, and each answer U:
  - the active rows are those of evaluate_batch(rows=True) at U that are <= --active-tol;
  - each active row's gradient in U is J' e_r, from one gradient_batch call over unit lam vectors;
  - the multipliers are estimated by numpy.linalg.lstsq on the controls strictly inside their bounds (a control at
    a bound carries the bound's own multiplier, which the projected-gradient measure accounts for);
  - gradient_batch at (U, lam) gives LAG_INF = max |grad - J' lam|, PG_INF (the same after projection on the
    bounds), COMPL = max |lam g| and MIN_LAM.
Per status class (OK / MAX_ITER / INFEASIBLE / NUMERICAL, with the MPC_SQP_UNCONVERGED flag as a class of its own)
the tool prints the count and the median and worst LAG_INF, PG_INF and COMPL and the least MIN_LAM.  A stationary
point of the reference's problem has PG_INF ~ 0, COMPL ~ 0 and MIN_LAM >= 0.

Times are reported as measured, no target: on a GPU the device-pointer entries on resident buffers, HIP events
around `--inner` back-to-back calls, the median of `--runs` such windows after `--warmup` untimed ones, the entries
alternating (the whole batch); with --device -1 the wall clock of the host backend's calls, the median of `--runs`.

With --multipliers device the multipliers come from mpc_multipliers_batch instead (Solver.certify_batch) and the
WHOLE batch is certified, not the sample: the same per-class tables, plus the instances per MPC_MU_* status and the
rows the drop rule left out; the entry is timed beside the others, and the host estimate of the sample is timed
once (wall clock) for comparison.  The default stays the host estimate on the sample.

    python tools/optimality_report.py [--config C2] [--B n] [--sample 256] [--device 0 | -1] [--multipliers host | device] [--json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "safe-autonomous-driving-mpc_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

CLASSES = ("OK", "MAX_ITER", "INFEASIBLE", "NUMERICAL", "SQP_UNCONVERGED")
CHUNK = 32768          # unit-lam instances per gradient_batch call


def estimate_multipliers(slv, x0, U, obs, n_obs, active_tol, bound_tol=1e-9):
    """lam [S,N,7+max_obs] >= or < 0 as least squares gives it: per instance the lstsq solution of
    grad[free] = (J' e_r)[free] lam_r over its active rows r, zero elsewhere; also the active-row counts [S]."""
    p = slv.params
    S, N, rw = x0.shape[0], p.N, 7 + p.max_obs
    sub = lambda a, i: None if a is None else a[i]
    rows = slv.evaluate_batch(x0, U, obs, n_obs, rows=True)["rows"]
    with np.errstate(invalid="ignore"):
        inst, stage, col = np.nonzero(rows <= active_tol)            # NaN (past n_obs) is never active
    grad = slv.gradient_batch(x0, U, obs, n_obs)["grad"].reshape(S, 2 * N)
    rg = np.empty((len(inst), 2 * N))
    for a in range(0, len(inst), CHUNK):
        i, k, c = inst[a:a + CHUNK], stage[a:a + CHUNK], col[a:a + CHUNK]
        unit = np.zeros((len(i), N, rw))
        unit[np.arange(len(i)), k, c] = 1.0
        rg[a:a + CHUNK] = slv.gradient_batch(x0[i], U[i], sub(obs, i), sub(n_obs, i), lam=unit)["jtl"].reshape(-1, 2 * N)
    lo = np.tile(np.array(list(p.u_min)), N) + bound_tol
    hi = np.tile(np.array(list(p.u_max)), N) - bound_tol
    lam = np.zeros((S, N, rw))
    first = np.searchsorted(inst, np.arange(S + 1))                   # np.nonzero returns inst sorted
    for b in range(S):
        r = slice(first[b], first[b + 1])
        if r.start == r.stop:
            continue
        u = U[b].reshape(-1)
        free = (u > lo) & (u < hi) & np.isfinite(grad[b])
        if not free.any():
            continue
        sol = np.linalg.lstsq(rg[r][:, free].T, grad[b][free], rcond=None)[0]
        lam[b, stage[r], col[r]] = sol
    return lam, np.diff(first)


def class_table(status, summary, n_active):
    """{class: dict(count, lag / pg / compl as (median, worst), min_lam, active (median))} of one answer's sample."""
    import mpcqp
    code = status & mpcqp.MPC_STATUS_MASK
    masks = [code == c for c in range(4)] + [(status & mpcqp.MPC_SQP_UNCONVERGED) != 0]
    out = {}
    for name, mask in zip(CLASSES, masks):
        q = summary[mask]
        if not len(q):
            out[name] = dict(count=0)
            continue
        mw = lambda k: (float(np.median(q[:, k])), float(np.max(q[:, k])))
        out[name] = dict(count=int(len(q)), lag=mw(mpcqp.GRQ_LAG_INF), pg=mw(mpcqp.GRQ_PG_INF),
                         compl=mw(mpcqp.GRQ_COMPL), min_lam=float(np.min(q[:, mpcqp.GRQ_MIN_LAM])),
                         active=float(np.median(n_active[mask])))
    return out


def print_table(title, table):
    print(title)
    print(f"  {'class':<16}{'count':>6}  {'LAG med':>10} {'LAG worst':>10}  {'PG med':>10} {'PG worst':>10}  "
          f"{'COMPL med':>10} {'COMPL worst':>11}  {'min lam':>10}  {'active med':>10}")
    for name in CLASSES:
        t = table[name]
        if not t["count"]:
            print(f"  {name:<16}{0:>6}")
            continue
        print(f"  {name:<16}{t['count']:>6}  {t['lag'][0]:>10.3g} {t['lag'][1]:>10.3g}  {t['pg'][0]:>10.3g} "
              f"{t['pg'][1]:>10.3g}  {t['compl'][0]:>10.3g} {t['compl'][1]:>11.3g}  {t['min_lam']:>10.3g}  "
              f"{t['active']:>10.0f}")


def device_times(a, solvers, wb, answers, B, N, mo):
    """Median / min / max ms per call of the device entries on resident buffers (HIP events)."""
    import torch
    import mpcqp
    dev = torch.device("cuda", 0)
    t = lambda x, dt=torch.float64: None if x is None else torch.as_tensor(x, dtype=dt, device=dev).contiguous()
    e = lambda *s, dt=torch.float64: torch.empty(s, dtype=dt, device=dev)
    p = lambda x: None if x is None else x.data_ptr()
    x0, obs, nob = t(wb["x0"]), t(wb["obs"]), t(wb["n_obs"], torch.int32)
    U = t(answers["bench"]["U"])
    lam = torch.zeros((B, N, 7 + mo), dtype=torch.float64, device=dev)
    mu = dict(lam=e(B, N, 7 + mo), act=e(B, mpcqp.MAX_ACTIVE, dt=torch.int32), s=e(B, mpcqp.MU_NQ))
    o = dict(u0=e(B, 2), U=e(B, N, 2), X=e(B, N + 1, 5), st=e(B, dt=torch.int32), it=e(B, dt=torch.int32),
             ev=e(B, mpcqp.EV_NQ), grad=e(B, N, 2), jtl=e(B, N, 2), gx0=e(B, 5), gr=e(B, mpcqp.GR_NQ))
    stream = torch.cuda.current_stream(dev).cuda_stream
    bench = solvers["bench"]

    def solve(which):
        solvers[which].solve_batch_device(B, p(x0), p(obs), p(nob), None, p(o["u0"]), p(o["U"]), p(o["X"]), p(o["st"]),
                                          p(o["it"]), stream=stream)

    sqp = f"solve sqp_iters={solvers['dropin'].params.sqp_iters}"
    entries = {"solve sqp_iters=1": (lambda: solve("bench"), a.inner),
               sqp: (lambda: solve("dropin"), max(1, a.inner // 10)),
               "evaluate (summary)": (lambda: bench.evaluate_batch_device(
                   B, p(x0), p(obs), p(nob), p(U), None, p(o["ev"]), None, None, stream=stream), a.inner),
               "gradient (grad, summary)": (lambda: bench.gradient_batch_device(
                   B, p(x0), p(obs), p(nob), p(U), None, p(o["grad"]), None, None, None, p(o["gr"]), stream=stream),
                   a.inner),
               "gradient (all, with lam)": (lambda: bench.gradient_batch_device(
                   B, p(x0), p(obs), p(nob), p(U), p(lam), p(o["grad"]), p(o["jtl"]), p(o["gx0"]), None, p(o["gr"]),
                   stream=stream), a.inner)}
    if a.multipliers == "device":
        entries["multipliers (all)"] = (lambda: bench.multipliers_batch_device(
            B, p(x0), p(obs), p(nob), p(U), p(mu["lam"]), p(mu["act"]), p(mu["s"]), active_tol=a.active_tol,
            stream=stream), a.inner)
    ms = {k: [] for k in entries}
    for r in range(a.warmup + a.runs):
        for k, (fn, inner) in entries.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(inner):
                fn()
            t1.record()
            t1.synchronize()
            if r >= a.warmup:
                ms[k].append(t0.elapsed_time(t1) / inner)
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))
            for k, v in ms.items()}


def host_times(a, solvers, wb, answers):
    """Median / min / max wall-clock ms per call of the host-buffer entries (the host backend)."""
    bench = solvers["bench"]
    U = answers["bench"]["U"]
    lam = np.zeros((U.shape[0], U.shape[1], 7 + bench.params.max_obs))
    args = (wb["x0"], wb["obs"], wb["n_obs"])
    entries = {"solve sqp_iters=1": lambda: solvers["bench"].solve_batch(*args),
               f"solve sqp_iters={solvers['dropin'].params.sqp_iters}": lambda: solvers["dropin"].solve_batch(*args),
               "evaluate (summary)": lambda: bench.evaluate_batch(wb["x0"], U, wb["obs"], wb["n_obs"]),
               "gradient (grad, summary)": lambda: bench.gradient_batch(wb["x0"], U, wb["obs"], wb["n_obs"]),
               "gradient (all, with lam)": lambda: bench.gradient_batch(wb["x0"], U, wb["obs"], wb["n_obs"], lam=lam)}
    if a.multipliers == "device":
        entries["multipliers (all)"] = lambda: bench.multipliers_batch(wb["x0"], U, wb["obs"], wb["n_obs"],
                                                                       active_tol=a.active_tol)
    ms = {k: [] for k in entries}
    for r in range(a.warmup + a.runs):
        for k, fn in entries.items():
            t0 = time.perf_counter()
            fn()
            if r >= a.warmup:
                ms[k].append(1e3 * (time.perf_counter() - t0))
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="C2", choices=["C2", "C3", "C4", "C5"])
    ap.add_argument("--B", type=int, default=None)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--device", type=int, default=0, help="HIP device, or -1 for the host backend")
    ap.add_argument("--active-tol", type=float, default=1e-6)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--multipliers", default="host", choices=["host", "device"],
                    help="host: numpy least squares on the sample (default); device: mpc_multipliers_batch on the whole batch")
    ap.add_argument("--json", action="store_true", help="also print one JSON line with every figure")
    a = ap.parse_args()

    if a.device >= 0:
        import torch                      # torch's HIP runtime first (bench.py does the same)
        if not torch.cuda.is_available():
            sys.exit("optimality_report: no GPU (--device -1 selects the host backend; nothing falls back)")
    import mpcqp
    import trajectory_tracking as TT
    import workloads as W

    cfg = W.CONFIGS[a.config]
    B = min(cfg["B"], 8192) if a.B is None else a.B          # one GPU's share of the multi-GPU configs
    wb = W.make_batch(a.config, B=B)
    N, mo = wb["N"], wb["max_obs"]
    ld = W.loader(wb["traj"])
    solvers = dict(bench=mpcqp.Solver(ld.X_ref, ld.U_ref, mpcqp.default_params(N=N, max_obs=mo), device=a.device),
                   dropin=mpcqp.Solver(ld.X_ref, ld.U_ref,
                                       mpcqp.default_params(N=N, max_obs=mo, sqp_iters=TT.SQP_ITERS), device=a.device))
    idx = np.unique(np.linspace(0, B - 1, min(a.sample, B)).astype(int))
    sub = lambda x: None if x is None else x[idx]
    answers, tables, mu_counts, host_ms = {}, {}, {}, None
    for which, slv in solvers.items():
        answers[which] = slv.solve_batch(wb["x0"], wb["obs"], wb["n_obs"])
        xs, Us, os_, ns = wb["x0"][idx], answers[which]["U"][idx], sub(wb["obs"]), sub(wb["n_obs"])
        if a.multipliers == "device":
            c = solvers["bench"].certify_batch(wb["x0"], answers[which]["U"], wb["obs"], wb["n_obs"],
                                               active_tol=a.active_tol)
            m = c["multipliers"]
            tables[which] = class_table(answers[which]["status"], c["summary"], m[:, mpcqp.MUQ_N_ACTIVE])
            ok = m[:, mpcqp.MUQ_STATUS] == mpcqp.MU_OK
            mu_counts[which] = dict({n: int((m[:, mpcqp.MUQ_STATUS] == i).sum()) for i, n in enumerate(mpcqp.MU_NAMES)},
                                    dropped_rows=int((m[ok, mpcqp.MUQ_N_ACTIVE] - m[ok, mpcqp.MUQ_N_USED]).sum()),
                                    instances_with_drops=int((m[ok, mpcqp.MUQ_N_ACTIVE] > m[ok, mpcqp.MUQ_N_USED]).sum()))
            if which == "bench":
                t0 = time.perf_counter()
                estimate_multipliers(solvers["bench"], xs, Us, os_, ns, a.active_tol)
                host_ms = 1e3 * (time.perf_counter() - t0)
            continue
        lam, n_active = estimate_multipliers(solvers["bench"], xs, Us, os_, ns, a.active_tol)
        summary = solvers["bench"].gradient_batch(xs, Us, os_, ns, lam=lam)["summary"]
        tables[which] = class_table(answers[which]["status"][idx], summary, n_active)
    timing = (device_times(a, solvers, wb, answers, B, N, mo) if a.device >= 0
              else host_times(a, solvers, wb, answers))

    where = f"HIP device {a.device}" if a.device >= 0 else "host backend"
    print(f"optimality report {a.config} on the {where}: trajectory{wb['traj']}, N = {N}, B = {B}, max_obs = {mo}, "
          f"sample = {len(idx)}, active rows <= {a.active_tol:g}")
    if a.multipliers == "device":
        print(f"multipliers from mpc_multipliers_batch: the tables cover the whole batch of {B}")
    print_table("single QP at the warm start (sqp_iters = 1, what bench.py times):", tables["bench"])
    print_table(f"drop-in default (Gauss-Newton SQP, sqp_iters = {TT.SQP_ITERS}):", tables["dropin"])
    for which, c in mu_counts.items():
        print(f"  multiplier status ({which}): " + ", ".join(f"{k} {v}" for k, v in c.items()))
    if a.device >= 0:
        print(f"device time per call over the whole batch, median of {a.runs} windows of {a.inner} calls "
              f"({max(1, a.inner // 10)} for the SQP solve), min .. max:")
    else:
        print(f"wall clock per call over the whole batch, median of {a.runs} calls, min .. max:")
    for k, v in timing.items():
        print(f"  {k:<26}{v['median_ms']:>10.4f} ms   ({v['min_ms']:.4f} .. {v['max_ms']:.4f})")
    if host_ms is not None:
        print(f"  {'host estimate of the sample':<26}{host_ms:>10.4f} ms   (estimate_multipliers on {len(idx)} instances, "
              f"wall clock, one call)")
    if a.json:
        print(json.dumps(dict(multipliers=a.multipliers, mu_counts=mu_counts, host_estimate_ms=host_ms, config=a.config, device=a.device, traj=wb["traj"], N=N, B=B, max_obs=mo,
                              sample=int(len(idx)), active_tol=a.active_tol, tables=tables, timing_ms=timing)))
    for slv in solvers.values():
        slv.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
