"""Closed-loop throughput of mpc_closed_loop_noisy against mpc_closed_loop_convoy on one GPU, and the per-check
pass rates at a few noise levels (a measurement, not a gate): trajectory1, N = 20, the solver settings and starts
of tools/convoy_timing.py, the same B egos and step cap in every run.  Alternately and in rotating order:

    convoy     mpc_closed_loop_convoy, K leaders, no script, worlds of W egos
    zero       mpc_closed_loop_noisy with an all-zero struct: the same problems through nz_measure_kernel and
               nz_plant_kernel, so the ratio to `convoy` is what the two kernels cost
    noisy      mpc_closed_loop_noisy at --level times the base sigmas: other problems (noise changes how many QPs
               go elastic), so this ratio shows what a disturbed step costs

    python tools/noise_timing.py [--egos 512] [--world 64] [--leaders 8] [--steps 200] [--repeats 3]
                                 [--level 1.0] [--levels 0 0.5 1 2 4] [--seed 1] [--out FILE.json]

Base sigmas (level 1): measurement (0.10 m, 0.05 m, 0.01, 0.001 1/m, 0.10 m/s), actuation (0.02 1/(m s),
0.20 m/s^2), process (0.05 m/s, 0.02 m/s, 0.01 1/s, 0.001 1/(m s), 0.10 m/s^2) and perception (0.5 m, 0.3 m/s).
Per run: ego-steps/s of the library call (a host clock around a call that ends in a device synchronise); the
median and the min-max spread over the repeats.  Per level: the fraction of egos passing each restated check
(mpc_cl_verdicts) after --steps steps; a step cap below the route length fails `destination` for everybody.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "safe-autonomous-driving-mpc_amd")]

BASE = dict(meas_sigma=[0.10, 0.05, 0.01, 0.001, 0.10], act_sigma=[0.02, 0.20],
            proc_sigma=[0.05, 0.02, 0.01, 0.001, 0.10], perc_sigma=[0.5, 0.3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--egos", type=int, default=512)
    ap.add_argument("--world", type=int, default=64)
    ap.add_argument("--leaders", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--level", type=float, default=1.0)
    ap.add_argument("--levels", type=float, nargs="+", default=[0.0, 0.5, 1.0, 2.0, 4.0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch                      # its HIP runtime first, as in bench.py
    if not torch.cuda.is_available():
        sys.exit("noise_timing: no GPU (a timing needs one)")
    import __graft_entry__ as g
    g.build()
    import mpcqp
    import trajectory_tracking as TT
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    ld = TrajectoryLoader(builtin_trajectory(1))
    slv = mpcqp.Solver(ld.X_ref, ld.U_ref, mpcqp.default_params(N=20, sqp_iters=TT.SQP_ITERS), device=args.device)
    B, W, K, steps = args.egos, args.world, args.leaders, args.steps
    if B % W:
        sys.exit(f"noise_timing: --egos {B} is not a multiple of --world {W}")
    s_stop = ld.s_max - 1.0
    perm = np.random.default_rng(W).permutation(W)
    x = np.tile(np.array([[0.5 * k, 0.0, 0.0, ld.get_state(0.5 * k)[3], 1.0] for k in perm]), (B // W, 1))

    def level(f):
        return mpcqp.default_noise(**{k: np.array(v) * f for k, v in BASE.items()})

    kw = dict(max_steps=steps, s_stop=s_stop)
    paths = {
        "convoy": lambda: slv.closed_loop_convoy(x, W, K, **kw),
        "zero": lambda: slv.closed_loop_noisy(x, W, K, noise=level(0.0), seed=args.seed, **kw),
        "noisy": lambda: slv.closed_loop_noisy(x, W, K, noise=level(args.level), seed=args.seed, **kw),
    }
    names = list(paths)
    for name in names:                                      # warm-up: code objects, the stage cache
        paths[name]()
    runs = {name: [] for name in names}
    elastic = {name: 0.0 for name in names}
    for rep in range(len(names) * args.repeats):
        k = rep % len(names)
        for name in names[k:] + names[:k]:
            t0 = time.perf_counter()
            r = paths[name]()
            t = time.perf_counter() - t0
            runs[name].append(int(r["n_steps"].sum()) / t)
            elastic[name] = float(r["quant"][:, 12].sum() / max(int(r["n_steps"].sum()), 1))
    out = {"egos": B, "N": 20, "trajectory": 1, "steps": steps, "world": W, "leaders": K, "level": args.level,
           "repeats": len(names) * args.repeats, "base_sigmas": BASE, "rates": {}, "pass_rates": {}}
    for name, v in runs.items():
        v = np.array(v)
        out["rates"][name] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
                              "not_ok_share": elastic[name]}
        print(f"{name:7s} {B} egos, W = {W}, K = {K}, {steps} steps: median {np.median(v):.0f} ego-steps/s "
              f"(min {v.min():.0f}, max {v.max():.0f}); {100.0 * elastic[name]:.1f}% of the steps not MPC_OK")
    for f in args.levels:
        r = slv.closed_loop_noisy(x, W, K, noise=level(f), seed=args.seed, **kw)
        _, counts = slv.cl_verdicts(r["quant"], ld.s_max)
        rates = {k: float(counts[i]) / B for i, k in enumerate(mpcqp.CLV_NAMES)}
        rates["clamped_share"] = float(r["extra"][:, mpcqp.NZX_N_CLAMPED].sum() / max(int(r["n_steps"].sum()), 1))
        out["pass_rates"][str(f)] = rates
        print(f"level {f:4.1f}: " + "  ".join(f"{k} {v:.3f}" for k, v in rates.items()))
    slv.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
