"""The planner's chunk kernel against its recorded outputs: tests/golden/plan_chunks_device.npz
(tools/record_plan_chunks.py documents the batch: 8 chunks on synth1, N = 13, 16, 20, 26 in turn, two of them final).
X, U, S, status, iterations and QP counts bit for bit, dtype and shape too: what "the kernel computes what it
computed" means across commits (the other planner tests hold the device to the oracle within a tolerance)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_plan_chunks as REC  # noqa: E402

pytestmark = pytest.mark.gpu


def test_chunks_equal_the_recorded_outputs():
    import __graft_entry__ as g
    g.build()
    recorded = REC.load()
    assert sorted(recorded["N"].tolist()) == sorted(2 * list(REC.HORIZONS)) and int(recorded["is_final"].sum()) == 2
    solved = np.isin(recorded["status"], (0, 4))                    # the record holds solved chunks of both kinds
    assert (solved & (recorded["is_final"] == 1)).any() and (solved & (recorded["is_final"] == 0)).any()
    got = REC.solve(0)
    for k in ("x0", "s_target", "is_final", "N") + REC.OUTPUTS:
        assert np.array_equal(got[k], recorded[k]), k
    assert REC.differences(got, recorded) == []
