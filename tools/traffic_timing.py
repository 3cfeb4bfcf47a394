"""Closed-loop throughput of mpc_closed_loop_traffic against mpc_closed_loop_sweep on one GPU (a measurement,
not a gate): trajectory1, N = 20, 512 egos, the start distribution, solver settings and 3000-step cap of
tools/sweep_timing.py.  Three runs, alternately and in rotating order:

    sweep      mpc_closed_loop_sweep with one shared scenario, the default mpc_fsm with both switches on
    traffic2   mpc_closed_loop_traffic with the same scenario through mpc_actors_from_fsm (A = 2)
    traffic8   mpc_closed_loop_traffic with A = 8, all cars, every one in the slab from the first step on

    python tools/traffic_timing.py [--egos 512] [--repeats 3] [--out FILE.json]

Per run: ego-steps/s of the library call (a host clock around a call that ends in a device synchronise).
Prints the median and the min-max spread over the repeats, and checks that sweep and traffic2 computed the same
n_steps and quantities.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "safe-autonomous-driving-mpc_amd")]

MAX_STEPS = 3000
COLS = [1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--egos", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch                      # its HIP runtime first, as in bench.py
    if not torch.cuda.is_available():
        sys.exit("traffic_timing: no GPU (a timing needs one)")
    import __graft_entry__ as g
    g.build()
    import mpcqp
    import trajectory_tracking as TT
    from trajectory_loader import TrajectoryLoader, builtin_trajectory
    ld = TrajectoryLoader(builtin_trajectory(1))
    slv = mpcqp.Solver(ld.X_ref, ld.U_ref, mpcqp.default_params(N=20, sqp_iters=TT.SQP_ITERS), device=args.device)
    rng = np.random.default_rng(1)
    B = args.egos
    s0, v0 = rng.uniform(0.0, 2.0, B), rng.uniform(0.5, 2.0, B)
    x = np.array([[s0[i], 0.0, 0.0, ld.get_state(s0[i])[3], v0[i]] for i in range(B)])
    fsm = mpcqp.default_fsm(dynamic_obstacle=1, traffic_light=1)
    two = mpcqp.actors_from_fsm(fsm)
    # eight cars well ahead of every ego and faster than it, spawned at once and never retired
    eight = [mpcqp.car(-1.0, 150.0 + 25.0 * k, 30.0 + k, 1.0e9) for k in range(8)]

    def timed(call):
        t0 = time.perf_counter()
        r = call()
        return r, time.perf_counter() - t0

    paths = {
        "sweep": lambda: slv.closed_loop_sweep(x, fsm, MAX_STEPS, s_max=ld.s_max),
        "traffic2": lambda: slv.closed_loop_traffic(x, two, MAX_STEPS, s_max=ld.s_max),
        "traffic8": lambda: slv.closed_loop_traffic(x, eight, MAX_STEPS, s_max=ld.s_max),
    }
    names = list(paths)
    for name in names:                                      # warm-up: code objects, the stage cache
        paths[name]()
    runs = {name: [] for name in names}
    ref, same, max_nobs = None, True, 0.0
    for rep in range(2 * args.repeats):
        for name in names[rep % 3:] + names[:rep % 3]:
            r, t = timed(paths[name])
            runs[name].append({"ego_steps": int(r["n_steps"].sum()), "loop_steps": int(r["n_steps"].max()), "call_s": t})
            if name == "sweep" and ref is None:
                ref = (r["n_steps"].copy(), r["quant"][:, COLS].copy())
            if name == "traffic2" and ref is not None:
                same = same and np.array_equal(r["n_steps"], ref[0]) and \
                    np.array_equal(r["quant"][:, COLS], ref[1], equal_nan=True)
            if name == "traffic8":
                max_nobs = max(max_nobs, float(r["extra"][:, mpcqp.TRX_MAX_NOBS].min()))
    slv.close()
    out = {"egos": B, "N": 20, "trajectory": 1, "max_steps": MAX_STEPS, "repeats": 2 * args.repeats,
           "sweep_equals_traffic2": bool(same), "traffic8_min_over_egos_of_max_nobs": max_nobs}
    for name, rs in runs.items():
        v = np.array([r["ego_steps"] / r["call_s"] for r in rs])
        out[name] = {"ego_steps": rs[0]["ego_steps"], "loop_steps": rs[0]["loop_steps"],
                     "ego_steps_per_s": {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())},
                     "call_s_median": float(np.median([r["call_s"] for r in rs]))}
        s = out[name]["ego_steps_per_s"]
        print(f"{name:9s} {B} egos, {rs[0]['loop_steps']} loop steps: median {s['median']:.0f} ego-steps/s "
              f"(min {s['min']:.0f}, max {s['max']:.0f})")
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
