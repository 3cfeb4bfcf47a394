"""Closed-loop throughput of mpc_closed_loop_convoy against mpc_closed_loop_traffic on one GPU (a measurement,
not a gate): trajectory1, N = 20, the solver settings of tools/traffic_timing.py, the same B egos, start states
and step cap in both runs; an ego that reaches the end of the line leaves the loop as usual, and the rate counts
the ego-steps actually run.  Per world size W, alternately and in rotating order:

    traffic    mpc_closed_loop_traffic with A scripted cars per ego, all in the slab from the first step on
    convoy     mpc_closed_loop_convoy with K = A leaders and no script, worlds of W egos

    python tools/convoy_timing.py [--egos 512] [--worlds 16 64 256] [--actors 8] [--steps 200] [--repeats 3]
                                  [--out FILE.json]

Per run: ego-steps/s of the library call (a host clock around a call that ends in a device synchronise).  Prints
the median and the min-max spread over the repeats.  The two runs do not solve the same problems (scripted cars
drive away, leaders are followed), so the ratio shows what a step costs, not what the ranking kernel alone costs:
that is in the kernel trace.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "safe-autonomous-driving-mpc_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--egos", type=int, default=512)
    ap.add_argument("--worlds", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--actors", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch                      # its HIP runtime first, as in bench.py
    if not torch.cuda.is_available():
        sys.exit("convoy_timing: no GPU (a timing needs one)")
    import __graft_entry__ as g
    g.build()
    import mpcqp
    import trajectory_tracking as TT
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    ld = TrajectoryLoader(builtin_trajectory(1))
    slv = mpcqp.Solver(ld.X_ref, ld.U_ref, mpcqp.default_params(N=20, sqp_iters=TT.SQP_ITERS), device=args.device)
    B, A, steps = args.egos, args.actors, args.steps
    s_stop = ld.s_max - 1.0
    cars = [mpcqp.car(-1.0e9, 150.0 + 25.0 * k, 30.0 + k, 1.0e12) for k in range(A)]
    out = {"egos": B, "N": 20, "trajectory": 1, "steps": steps, "actors": A, "repeats": 2 * args.repeats, "worlds": {}}
    for W in args.worlds:
        if B % W:
            sys.exit(f"convoy_timing: --egos {B} is not a multiple of W = {W}")
        # a world's egos 0.5 m apart in a fixed permutation (rank differs from index)
        perm = np.random.default_rng(W).permutation(W)
        x = np.tile(np.array([[0.5 * k, 0.0, 0.0, ld.get_state(0.5 * k)[3], 1.0] for k in perm]), (B // W, 1))
        paths = {
            "traffic": lambda: slv.closed_loop_traffic(x, cars, steps, s_stop=s_stop),
            "convoy": lambda: slv.closed_loop_convoy(x, W, A, max_steps=steps, s_stop=s_stop),
        }
        names = list(paths)
        for name in names:                                  # warm-up: code objects, the stage cache
            paths[name]()
        runs = {name: [] for name in names}
        most = 0.0
        for rep in range(2 * args.repeats):
            for name in names[rep % 2:] + names[:rep % 2]:
                t0 = time.perf_counter()
                r = paths[name]()
                t = time.perf_counter() - t0
                runs[name].append(int(r["n_steps"].sum()) / t)
                if name == "convoy":
                    most = max(most, float(r["extra"][:, mpcqp.CVX_MAX_LEADERS].max()))
        row = {"max_leaders": most}
        for name, v in runs.items():
            v = np.array(v)
            row[name] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}
            print(f"W = {W:3d} {name:8s} {B} egos, {steps} steps: median {row[name]['median']:.0f} ego-steps/s "
                  f"(min {row[name]['min']:.0f}, max {row[name]['max']:.0f})")
        out["worlds"][str(W)] = row
    slv.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
