"""Whole-batch quality of the offline planner by the reference NLP's own measures (plan_evaluate_chunks).

workloads.plan_batch_ref on trajectory3's route (the chunks optimize_full_trajectory poses, each with its own
horizon) is solved on the device in one launch and every chunk plan is evaluated; per status class
(PLAN_OK .. PLAN_FROZEN_LIMITS) the tool prints the count and, for MAX_DEFECT, L1_INEQ, MIN_ROW and the reference's
cost, the median and the worst value.  On a sample of `--slsqp` chunks the same columns are printed for the answer of
the reference's own solver (scipy SLSQP on oracle/plan_ref.py's restatement, analytic Jacobians), evaluated through
the same entry, beside the library's answer on the same chunks.  A report: no thresholds are checked.

Timing: device-pointer entries on resident buffers, HIP events around `--inner` back-to-back calls, `--runs` such
windows per entry after `--warmup` untimed ones, the two entries alternating; the figure is the median window over
inner.  With --device -1 the tables come from the host backend and nothing is timed.

    python tools/plan_quality_report.py [--B 8192] [--slsqp 64] [--runs 20] [--inner 10] [--warmup 3] [--json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "safe-autonomous-driving-mpc_amd"), os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

COLS = ("max_defect", "l1_ineq", "min_row", "cost")


def class_table(status, summary):
    """{class name: dict(count, <column>: (median, worst))} of one evaluation (worst: min for MIN_ROW, else max)."""
    import mpcplan
    out = {}
    for code, name in mpcplan.STATUS_NAMES.items():
        q = summary[status == code]
        out[name] = dict(count=int(len(q)))
        for c in COLS if len(q) else ():
            v = q[:, mpcplan.EVQ[c]]
            out[name][c] = (float(np.median(v)), float(np.min(v) if c == "min_row" else np.max(v)))
    return out


def print_table(title, table):
    print(title)
    print(f"  {'class':<14}{'count':>7}  " + "  ".join(f"{c + ' med':>15} {c + ' worst':>16}" for c in COLS))
    for name, t in table.items():
        if not t["count"]:
            print(f"  {name:<14}{0:>7}")
            continue
        print(f"  {name:<14}{t['count']:>7}  " + "  ".join(f"{t[c][0]:>15.4g} {t[c][1]:>16.4g}" for c in COLS))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--slsqp", type=int, default=64, help="chunks of the SLSQP sample (0: none)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", action="store_true", help="also print one JSON line with every figure")
    a = ap.parse_args()

    if a.device >= 0:
        import torch                  # torch's HIP runtime first (bench.py does the same)
        if not torch.cuda.is_available():
            sys.exit("plan_quality_report: no GPU (--device -1 reports the host backend, untimed)")
    import mpcplan
    import workloads as W

    route = W.plan_route("traj3")
    wb = W.plan_batch_ref(route, a.B, seed=3)
    B, Nv = a.B, wb["N"]
    Nmax = int(Nv.max())
    pl = mpcplan.Planner(route, mpcplan.default_params(N=min(Nmax, mpcplan.PLAN_MAX_N)), device=a.device)
    sol = pl.solve_chunks(wb["x0"], wb["s_target"], wb["is_final"], N=Nv)
    ev = pl.evaluate_chunks(wb["x0"], wb["s_target"], wb["is_final"], sol["X"], sol["U"], sol["S"], N=Nv, want=("summary",))
    table = class_table(sol["status"], ev["summary"])
    chk = pl.check_verdicts(ev["summary"])

    # the reference's own solver on a sample, through the same entry
    sample = {}
    if a.slsqp > 0:
        import plan_ref as PR
        idx = np.linspace(0, B - 1, min(a.slsqp, B)).astype(int)
        Xs, Us, Ss = np.zeros((len(idx), Nmax + 1, 5)), np.zeros((len(idx), Nmax, 2)), np.zeros((len(idx), Nmax))
        ok = np.zeros(len(idx), bool)
        for j, b in enumerate(idx):
            n = int(Nv[b])
            ch = PR.Chunk(route, n, pl.params.dt, wb["x0"][b], float(wb["s_target"][b]), bool(wb["is_final"][b]))
            r, _ = ch.slsqp(jac=True)
            Xs[j, :n + 1], Us[j, :n], Ss[j, :n] = ch.unpack(r.x)
            ok[j] = bool(r.success)
        es = pl.evaluate_chunks(wb["x0"][idx], wb["s_target"][idx], wb["is_final"][idx], Xs, Us, Ss, N=Nv[idx],
                                want=("summary",))["summary"]
        sample = dict(n=int(len(idx)), slsqp_success=int(ok.sum()),
                      slsqp=class_table(np.zeros(len(idx), np.int32), es)["ok"],
                      library=class_table(np.zeros(len(idx), np.int32), ev["summary"][idx])["ok"],
                      library_status=np.bincount(sol["status"][idx], minlength=5).tolist())

    timing = {}
    if a.device >= 0:
        dev = torch.device("cuda", a.device)
        t = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=dev)
        e = lambda *s, dt=torch.float64: torch.empty(s, dtype=dt, device=dev)
        x0, st, fin, Nd = t(wb["x0"]), t(wb["s_target"]), t(wb["is_final"], torch.int32), t(Nv, torch.int32)
        X, U, S = e(B, Nmax + 1, 5), e(B, Nmax, 2), e(B, Nmax)
        o = [e(B, dt=torch.int32) for _ in range(3)]
        q = e(B, mpcplan.PLAN_EV_NQ)
        stream = torch.cuda.current_stream(dev).cuda_stream
        entries = {
            "solve": lambda: pl.solve_chunks_device(B, Nmax, Nd.data_ptr(), x0.data_ptr(), st.data_ptr(), fin.data_ptr(),
                                                    X.data_ptr(), U.data_ptr(), S.data_ptr(), *[z.data_ptr() for z in o],
                                                    stream=stream),
            "evaluate (summary)": lambda: pl.evaluate_chunks_device(B, Nmax, Nd.data_ptr(), x0.data_ptr(), st.data_ptr(),
                                                                    fin.data_ptr(), X.data_ptr(), U.data_ptr(), S.data_ptr(),
                                                                    q.data_ptr(), 0, 0, stream=stream)}
        ms = {k: [] for k in entries}
        for r in range(a.warmup + a.runs):
            for k, fn in entries.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.inner):
                    fn()
                t1.record()
                t1.synchronize()
                if r >= a.warmup:
                    ms[k].append(t0.elapsed_time(t1) / a.inner)
        timing = {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))
                  for k, v in ms.items()}
        same = bool(np.array_equal(q.cpu().numpy(), ev["summary"], equal_nan=True))
    pl.close()

    print(f"planner quality report: route traj3 ({route.s_total:.0f} m), B = {B} chunks of plan_batch_ref, horizons "
          f"{int(Nv.min())}..{Nmax}, device {a.device}")
    print_table("the library's chunk plans, by status:", table)
    print("reference_trajectory_check bits over all chunks (chunks are not whole plans: DESTINATION / FULL_STOP are "
          "expected to fail on intermediate ones): " + ", ".join(f"{n} {int(c)}" for n, c in zip(mpcplan.CHECK_NAMES, chk["counts"])))
    if sample:
        print(f"sample of {sample['n']} chunks: scipy SLSQP (maxiter 500, ftol 1e-4) reported success on "
              f"{sample['slsqp_success']}; the library's statuses there {sample['library_status']}")
        print_table("the same columns on the sample:", {"slsqp": sample["slsqp"], "library": sample["library"]})
    if timing:
        print(f"device time per call, median of {a.runs} windows of {a.inner} calls (min .. max); the timed evaluation's "
              f"summary equals the reported one bit for bit: {same}")
        for k, v in timing.items():
            print(f"  {k:<20}{v['median_ms']:>10.4f} ms   ({v['min_ms']:.4f} .. {v['max_ms']:.4f})   "
                  f"{B / v['median_ms'] / 1e3:.3f} M chunks/s")
    if a.json:
        print(json.dumps(dict(B=B, Nmin=int(Nv.min()), Nmax=Nmax, table=table, checks=chk["counts"].tolist(), sample=sample,
                              timing_ms=timing)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
