"""Closed-loop throughput of mpc_closed_loop_traced against mpc_closed_loop_noisy on one GPU (a measurement, not a
gate): trajectory1, N = 20, the solver settings, starts and base sigmas of tools/noise_timing.py, the same context,
B egos and step cap in every run.  Alternately and in rotating order:

    noisy      mpc_closed_loop_noisy at --level times the base sigmas
    off        mpc_closed_loop_traced with nothing requested: the noisy entry's launches, so the ratio to `noisy`
               is the run-to-run spread
    gaps       mpc_closed_loop_traced with --lookahead: the solver also writes its U and Xpred, and tg_gap_kernel
               runs per step
    gaps+hist  the same plus hist_pred and hist_plan of --hist egos: tg_hist_kernel runs per step as well

    python tools/trace_timing.py [--egos 512] [--world 64] [--leaders 8] [--steps 200] [--repeats 3] [--level 1.0]
                                 [--lookahead 1 5 20] [--hist 16] [--seed 1] [--out FILE.json]

Per run: ego-steps/s of the library call (a host clock around a call that ends in a device synchronise); per path
the median and the min-max spread over the repeats, and the ratio of its median to the noisy entry's.  The runs of
one repeat solve the same problems (the same seed), so the ratios are what the extra outputs and kernels cost.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "safe-autonomous-driving-mpc_amd"), os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--egos", type=int, default=512)
    ap.add_argument("--world", type=int, default=64)
    ap.add_argument("--leaders", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--level", type=float, default=1.0)
    ap.add_argument("--lookahead", type=int, nargs="+", default=[1, 5, 20])
    ap.add_argument("--hist", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch                      # its HIP runtime first, as in bench.py
    if not torch.cuda.is_available():
        sys.exit("trace_timing: no GPU (a timing needs one)")
    import __graft_entry__ as g
    g.build()
    import mpcqp
    import trajectory_tracking as TT
    from noise_timing import BASE
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    ld = TrajectoryLoader(builtin_trajectory(1))
    slv = mpcqp.Solver(ld.X_ref, ld.U_ref, mpcqp.default_params(N=20, sqp_iters=TT.SQP_ITERS), device=args.device)
    B, W, K, steps = args.egos, args.world, args.leaders, args.steps
    if B % W:
        sys.exit(f"trace_timing: --egos {B} is not a multiple of --world {W}")
    s_stop = ld.s_max - 1.0
    perm = np.random.default_rng(W).permutation(W)
    x = np.tile(np.array([[0.5 * k, 0.0, 0.0, ld.get_state(0.5 * k)[3], 1.0] for k in perm]), (B // W, 1))
    noise = mpcqp.default_noise(**{k: np.array(v) * args.level for k, v in BASE.items()})
    named = np.linspace(0, B - 1, min(args.hist, B)).astype(int)
    kw = dict(max_steps=steps, s_stop=s_stop, noise=noise, seed=args.seed)
    paths = {
        "noisy": lambda: slv.closed_loop_noisy(x, W, K, **kw),
        "off": lambda: slv.closed_loop_traced(x, W, K, **kw),
        "gaps": lambda: slv.closed_loop_traced(x, W, K, lookahead=args.lookahead, **kw),
        "gaps+hist": lambda: slv.closed_loop_traced(x, W, K, lookahead=args.lookahead, preds=True, plans=True,
                                                    hist_egos=named, **kw),
    }
    names = list(paths)
    for name in names:                                      # warm-up: code objects, the stage cache
        paths[name]()
    runs = {name: [] for name in names}
    for rep in range(len(names) * args.repeats):
        k = rep % len(names)
        for name in names[k:] + names[:k]:
            t0 = time.perf_counter()
            r = paths[name]()
            t = time.perf_counter() - t0
            runs[name].append(int(r["n_steps"].sum()) / t)
    out = {"egos": B, "N": 20, "trajectory": 1, "steps": steps, "world": W, "leaders": K, "level": args.level,
           "lookahead": args.lookahead, "hist_egos": int(named.size), "repeats": len(names) * args.repeats,
           "rates": {}, "ratio_to_noisy": {}}
    base = float(np.median(runs["noisy"]))
    for name, v in runs.items():
        v = np.array(v)
        out["rates"][name] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}
        out["ratio_to_noisy"][name] = float(np.median(v)) / base
        print(f"{name:9s} {B} egos, W = {W}, K = {K}, {steps} steps: median {np.median(v):.0f} ego-steps/s "
              f"(min {v.min():.0f}, max {v.max():.0f}); {np.median(v) / base:.3f} of the noisy entry")
    slv.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
