"""Build tools/evaluate_host_check.cpp with AddressSanitizer + UBSan (host code only, a stand-alone program) and run
it on trajectory2: the host backend's evaluator (mpc_evaluate_batch with device = -1) must run clean over every
argument variant (horizons at both lane-group boundaries, partial batches, slabs of 0, 1 and 64 with every n_obs form,
every subset of NULL outputs, NaN inputs) and keep its outputs consistent.  Same sanitizer and FP flags as
tools/noise_host_check.py.

    python tools/evaluate_host_check.py          # exit status of the program (0 = clean and equal)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "evaluate_host_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
FP = ["-ffp-contract=off", "-fno-fast-math"]


def main():
    with np.load(os.path.join(ROOT, "safe-autonomous-driving-mpc_amd", "data", "trajectory2.npz")) as z:
        X, U = np.ascontiguousarray(z["X"], np.float64), np.ascontiguousarray(z["U"], np.float64)
    with tempfile.TemporaryDirectory() as tmp:
        exe, data = os.path.join(tmp, "evaluate_host_check"), os.path.join(tmp, "traj.bin")
        subprocess.run(["g++", "-std=c++17"] + SAN + FP + ["-pthread", "-Wall", "-Wextra", "-o", exe, SRC], check=True)
        with open(data, "wb") as fh:
            fh.write(np.array([X.shape[0], U.shape[0]], np.int32).tobytes() + X.tobytes() + U.tobytes())
        return subprocess.run([exe, data]).returncode


if __name__ == "__main__":
    sys.exit(main())
