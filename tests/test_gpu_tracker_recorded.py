"""The tracker's evaluator, lookup and pose kernels against their recorded outputs:
tests/golden/tracker_model_device.npz (tools/record_tracker_model.py documents the batches: trajectory 1, N = 5, 15,
16, 31, 32 with 5 instances each, max_obs = 0 and 3, one call with n_obs = NULL, a NaN control, a rollout past s_max;
lookup and global_pose at 40 abscissae).  Every output bit for bit, dtype and shape too: what "the kernels compute
what they computed" means across commits (the other tests of these kernels hold the device to the reference's
goldens, to numpy and to the host backend).

The evaluator's siblings (gradient_batch, multipliers_batch, hessvec_batch) are held the same way to
tests/golden/tracker_derivatives_device.npz: N = 15, 16, 32 with the same five instances, max_obs = 0 and 3, with and
without lam, default and steered active_tol, both Hessian modes, given and unit directions, and N = 57 (the 32-wide
pass)."""
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


def test_derivatives_equal_the_recorded_outputs():
    import __graft_entry__ as g
    g.build()
    recorded = REC.load(REC.DERIV_GOLDEN)
    mo = f"mo{REC.MAX_OBS}"
    # the record holds what the tool's docstring says: every horizon with and without obstacles, the three entries with
    # each of their outputs, the NaN instance, and lists that are empty, kept whole, cut by the drop rule and overflowing
    kinds = set()
    for N in REC.DERIV_HORIZONS:
        for tag in ("mo0", mo):
            rw = 7 + (REC.MAX_OBS if tag == mo else 0)
            for k in ("grad", "gx0", "summary", "jtl", "costate"):
                assert f"N{N}_{tag}_gr_{k}" in recorded
            assert f"N{N}_{tag}_gr_nolam_grad" in recorded and f"N{N}_{tag}_gr_nolam_jtl" not in recorded
            assert np.isnan(recorded[f"N{N}_{tag}_gr_summary"][3, 0]) and np.isfinite(recorded[f"N{N}_{tag}_gr_summary"][4]).all()
            for i in range(1 + len(REC.DERIV_STEER)):
                assert recorded[f"N{N}_{tag}_mu{i}_lam"].shape == (REC.B, N, rw)
                assert recorded[f"N{N}_{tag}_mu{i}_active"].dtype == np.int32
                st, na, _, nu = recorded[f"N{N}_{tag}_mu{i}_summary"][:, :4].astype(int).T
                kinds |= {"empty"} if ((st == 0) & (na == 0)).any() else set()
                kinds |= {"whole"} if ((st == 0) & (na > 0) & (nu == na)).any() else set()
                kinds |= {"dropped"} if ((st == 0) & (nu < na)).any() else set()
                kinds |= {"overflow"} if (st == 1).any() else set()
            for run, M in [(m, REC.DERIV_M) for m in REC.DERIV_MODES] + [("unit", REC.DERIV_UNIT_M)]:
                assert recorded[f"N{N}_{tag}_hv_{run}_HV"].shape == (REC.B, M, N, 2)
                assert recorded[f"N{N}_{tag}_hv_{run}_JV"].shape == (REC.B, M, N, rw)
                assert recorded[f"N{N}_{tag}_hv_{run}_curv"].shape == (REC.B, M, 2)
            assert np.isnan(recorded[f"N{N}_{mo}_hv_exact_JV"][0, :, :, 7:]).all()           # n_obs = 0
    assert kinds == {"empty", "whole", "dropped", "overflow"}, kinds
    N = REC.DERIV_N32PASS
    assert recorded[f"N{N}_{mo}_hv_exact_HV"].shape == (REC.DERIV_B32PASS, REC.DERIV_M, N, 2)
    got = REC.run_derivatives(0)
    for k in recorded:
        assert k in got and got[k].dtype == recorded[k].dtype and got[k].shape == recorded[k].shape, k
        assert got[k].tobytes() == recorded[k].tobytes(), k
    assert REC.differences(got, recorded) == []
