"""What carrying each plan forward as the next linearisation point does to the closed loop (mpc_closed_loop_warm).

C2-style egos (workloads.make_batch("C2"): trajectory1, N = 20, no obstacles) drive to the end of the route three ways:
the reference warm start with a single QP per step (the headline path), the carried plan with a single QP per step
(the real-time iteration) and the reference warm start with full SQP; each with every sigma 0 and with
noise_cases' mild noise (tests/noise_cases.py, mild(1.0)).  Per variant the tool prints
  ego-steps/s            sum(n_steps) / sum(step_ms), the median of `--runs` runs (device events around every step)
  pass counts            mpc_cl_verdicts on the run's quantities
  gap columns            median and worst MAX_DS / MAX_DD / MAX_DV of every lookahead over the egos that have pairs
  MAX_MOVE / SUM_MOVE    quartiles and maximum over the egos that ran
  plan cost and L1       the mean of mpc_evaluate_batch's cost and l1 over every kept plan of the named egos
and, last, the carried loop's speed as a ratio to mpc_closed_loop_traced with the same outputs on the same build.
`--traced-only` times mpc_closed_loop_traced alone (it runs on a library without the warm entry too, so the same
command on two builds compares them).  A report: no thresholds are checked.

    python tools/warm_report.py [--B 4096] [--steps 200] [--named 64] [--runs 3] [--sqp 10] [--json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "safe-autonomous-driving-mpc_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED = 2024


def mild(mpcqp):
    """tests/noise_cases.py's mild(1.0): every channel on, small against the state it perturbs."""
    return mpcqp.default_noise(meas_sigma=[0.05, 0.02, 0.005, 0.0005, 0.05], act_sigma=[0.02, 0.2],
                               proc_sigma=[0.02, 0.01, 0.005, 0.0005, 0.05], perc_sigma=[0.3, 0.2])


def steps_per_s(r):
    return float(r["n_steps"].sum() / (np.nansum(r["step_ms"]) / 1e3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200, help="step cap of every loop")
    ap.add_argument("--named", type=int, default=64, help="egos whose plans are kept and evaluated")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sqp", type=int, default=10, help="sqp_iters of the full-SQP variant")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--traced-only", action="store_true")
    ap.add_argument("--json", action="store_true", help="also print one JSON line with every figure")
    a = ap.parse_args()

    if a.device >= 0:
        import torch                  # torch's HIP runtime first (bench.py does the same)
        if not torch.cuda.is_available():
            sys.exit("warm_report: no GPU (--device -1 reports the host backend)")
    import mpcqp
    import workloads as W

    wb = W.make_batch("C2", a.B)
    traj, N, x0 = W.loader(wb["traj"]), wb["N"], wb["x0"]
    look = [1, 5, N]
    named = np.linspace(0, a.B - 1, min(a.named, a.B)).astype(int)
    solvers = {k: mpcqp.Solver(traj.X_ref, traj.U_ref, mpcqp.default_params(N=N, sqp_iters=k), device=a.device)
               for k in (1, a.sqp)}
    kw = dict(max_steps=a.steps, s_max=traj.s_max, hist_egos=named, seed=SEED, lookahead=look, plans=True)
    noises = {"quiet": None, "mild": mild(mpcqp)}

    def timed(fn):
        rs = [fn() for _ in range(a.runs + 1)][1:]                   # the first run warms up
        return rs[0], float(np.median([steps_per_s(r) for r in rs]))

    out = {}
    if a.traced_only:
        for nz, noise in noises.items():
            _, sps = timed(lambda: solvers[1].closed_loop_traced(x0, noise=noise, **kw))
            out[nz] = sps
            print(f"closed_loop_traced, {nz}: {sps / 1e6:.3f} M ego-steps/s (B = {a.B}, N = {N})")
        if a.json:
            print(json.dumps(dict(B=a.B, N=N, traced_steps_per_s=out)))
        return 0

    carry = mpcqp.default_warm(mode=mpcqp.WARM_CARRY)
    variants = {"reference, 1 QP": (1, None), "carry, 1 QP": (1, carry), f"reference, SQP {a.sqp}": (a.sqp, None)}
    print(f"warm-start report: trajectory{wb['traj']} ({traj.s_max:.0f} m), B = {a.B} C2 egos, N = {N}, step cap {a.steps}, "
          f"{named.size} named egos, device {a.device}")
    for nz, noise in noises.items():
        for name, (sqp, warm) in variants.items():
            slv = solvers[sqp]
            r, sps = timed(lambda: slv.closed_loop_warm(x0, noise=noise, warm=warm, warmq=True, **kw))
            _, counts = slv.cl_verdicts(r["quant"], traj.s_max)
            ns = r["n_steps"]
            ran = ns > 0
            gaps = {}
            for i, j in enumerate(look):
                g = r["gapq"][r["gapq"][:, i, 0] > 0, i]
                gaps[j] = {c: (float(np.median(g[:, k])), float(np.max(g[:, k])))
                           for k, c in ((1, "ds"), (2, "dd"), (3, "dv"))}
            wq = r["warmq"][ran]
            dist = lambda v: [float(x) for x in np.percentile(v, [25, 50, 75, 100])]
            valid = np.arange(a.steps)[None, :] < ns[named][:, None]
            ev = slv.evaluate_batch(r["hist_xm"][valid], r["hist_plan"][valid])["summary"]
            rec = dict(steps_per_s=sps, passed=int(counts[7]), counts=[int(c) for c in counts], ran=int(ran.sum()),
                       mean_steps=float(ns[ran].mean()), gaps=gaps, n_reset_mean=float(wq[:, 0].mean()),
                       max_move=dist(wq[:, 1]), sum_move=dist(wq[:, 3]), plan_cost=float(ev[:, mpcqp.EVQ_COST].mean()),
                       plan_l1=float(ev[:, mpcqp.EVQ_L1].mean()), n_not_ok=float(r["quant"][:, 12].sum()))
            out[f"{nz} / {name}"] = rec
            print(f"\n{nz} noise, {name}: {sps / 1e6:.3f} M ego-steps/s; {rec['ran']} egos ran {rec['mean_steps']:.1f} steps "
                  f"on average, {int(rec['n_not_ok'])} steps not MPC_OK")
            print("  passed " + ", ".join(f"{n} {c}" for n, c in zip(mpcqp.CLV_NAMES, rec["counts"])))
            for j, g in gaps.items():
                print(f"  lookahead {j:>2}: " + "  ".join(f"max_{c} med {m:.4g} worst {w:.4g}" for c, (m, w) in g.items()))
            print(f"  resets per ego {rec['n_reset_mean']:.2f}; MAX_MOVE q25/q50/q75/max " +
                  "/".join(f"{v:.4g}" for v in rec["max_move"]) + "; SUM_MOVE " +
                  "/".join(f"{v:.4g}" for v in rec["sum_move"]))
            print(f"  kept plans of the named egos ({len(ev)}): mean cost {rec['plan_cost']:.6g}, mean L1 {rec['plan_l1']:.4g}")
    ratio = {}
    for nz, noise in noises.items():
        _, tr = timed(lambda: solvers[1].closed_loop_traced(x0, noise=noise, **kw))
        ratio[nz] = dict(traced_steps_per_s=tr, carry_over_traced=out[f"{nz} / carry, 1 QP"]["steps_per_s"] / tr)
        print(f"\n{nz}: closed_loop_traced {tr / 1e6:.3f} M ego-steps/s; the carried loop runs at "
              f"{ratio[nz]['carry_over_traced']:.3f} of it")
    for s in solvers.values():
        s.close()
    if a.json:
        print(json.dumps(dict(B=a.B, N=N, steps=a.steps, variants=out, ratio=ratio)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
