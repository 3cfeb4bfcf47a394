"""The tracker's evaluator, lookup and pose kernels against their recorded outputs:
tests/golden/tracker_model_device.npz (tools/record_tracker_model.py documents the batches: trajectory 1, N = 5, 15,
16, 31, 32 with 5 instances each, max_obs = 0 and 3, one call with n_obs = NULL, a NaN control, a rollout past s_max;
lookup and global_pose at 40 abscissae).  Every output bit for bit, dtype and shape too: what "the kernels compute
what they computed" means across commits (the other tests of these kernels hold the device to the reference's
goldens, to numpy and to the host backend)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_tracker_model as REC  # noqa: E402

pytestmark = pytest.mark.gpu


def test_outputs_equal_the_recorded_outputs():
    import __graft_entry__ as g
    g.build()
    recorded = REC.load()
    # the record holds what its docstring says: every horizon with and without obstacles, the NULL call, the NaN
    # instance, the instance past s_max, NaN-padded rows, and abscissae outside the table
    for N in REC.HORIZONS:
        for tag in ("mo0", f"mo{REC.MAX_OBS}"):
            for k in REC.OUTPUTS:
                assert f"N{N}_{tag}_{k}" in recorded
        assert recorded[f"N{N}_mo{REC.MAX_OBS}_rows"].shape == (REC.B, N, 7 + REC.MAX_OBS)
        assert np.isnan(recorded[f"N{N}_mo0_summary"][3, 0]) and np.isfinite(recorded[f"N{N}_mo0_summary"][4, 0])
        assert np.isnan(recorded[f"N{N}_mo{REC.MAX_OBS}_rows"][0, :, 7:]).all()          # n_obs = 0
    assert f"N{REC.N_NULL}_mo{REC.MAX_OBS}_null_rows" in recorded
    assert np.isfinite(recorded[f"N{REC.N_NULL}_mo{REC.MAX_OBS}_null_rows"][0]).all()    # NULL: all max_obs rows
    s = recorded["lk_s"]
    assert s.shape == (40,) and np.isnan(s).sum() == 1 and (s < 0).any()
    assert (recorded["lk_control"] == 0.0).all(axis=1).sum() >= 4                        # at and past s_max
    got = REC.run(0)
    for k in recorded:
        assert k in got and got[k].dtype == recorded[k].dtype and got[k].shape == recorded[k].shape, k
        assert got[k].tobytes() == recorded[k].tobytes(), k
    assert REC.differences(got, recorded) == []
