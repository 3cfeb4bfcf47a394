"""bench.py's multi-rank launch: `python bench.py --gpus N` without torchrun starts N
rank processes itself, and a rank whose WORLD_SIZE disagrees with --gpus refuses to run.  The ranks use
the `--device cpu` stand-in (libmpcqp's host backend, gloo), the same sharded path as the GPU ranks.
The legs beyond the headline run only with `--full`; a plain run prints the headline line alone and, with
`--dump-outputs DIR`, writes the last timed step's outputs, the same from run to run."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env=None):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=e, timeout=600)


def test_self_launch_two_ranks():
    r = _run(["--gpus", "2", "--device", "cpu", "--steps", "2", "--warmup", "1", "--batch", "48", "--full",
              "--no-cpu", "--closed-loop", "6"])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout            # rank 0 alone prints the result line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2
    assert d["solver"]["ranks"] == 2 and d["solver"]["egos"] == 96
    assert d["config"]["global_batch"] == 96
    assert d["closed_loop"]["ranks"] == 2 and d["closed_loop"]["egos"] == 12
    assert d["device"] == "cpu-standin"


def test_plain_run_prints_the_headline_alone_and_dumps_its_outputs(tmp_path):
    import numpy as np
    runs = []
    for d in ("a", "b"):
        r = _run(["--gpus", "1", "--device", "cpu", "--steps", "3", "--warmup", "1", "--batch", "40",
                  "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        runs.append(json.loads(lines[0]))
    d = runs[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "solves/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 40 / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    for leg in ("solver", "roofline", "p50_batch_latency_ms", "nlp_sqp", "inflight", "closed_loop", "plan",
                "cpu_backend", "cpu_reference", "cpu_baseline"):
        assert leg not in d, leg
    shapes = {"u0": (40, 2), "U": (40, 20, 2), "Xpred": (40, 21, 5), "status": (40,), "iters": (40,)}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(k + ".npy" for k in shapes)
    for k, shp in shapes.items():
        a, b = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert a.dtype == np.float64 and a.shape == shp, (k, a.dtype, a.shape)
        assert np.isfinite(a).all() and np.array_equal(a, b), k
    # what a caller of the timed path receives: the first input of the plan is the step's control
    assert np.array_equal(np.load(tmp_path / "a" / "u0.npy"), np.load(tmp_path / "a" / "U.npy")[:, 0])


def test_world_size_mismatch_refused():
    r = _run(["--gpus", "2", "--device", "cpu", "--steps", "1", "--warmup", "0", "--batch", "8", "--no-cpu",
              "--closed-loop", "0"], env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr
