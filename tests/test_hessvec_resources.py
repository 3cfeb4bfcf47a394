"""Static resources of the Hessian-vector kernels (CPU test: reads the gfx950 code object's metadata from libmpcqp.so
with the ROCm LLVM tools, tools/kernel_resources.py).  mpc_hessvec_kernel<W, OBS> (csrc/hessvec_kernel.h) exists for the
pass widths W = 64 and 32 with and without obstacles and uses no scratch; its LDS is all dynamic, and static plus
dynamic at each pass width's longest horizon equals the header's formula (include/mpcqp.h, MPC_HV_N64_MAX) and stays
within the 160 KiB of a CU.  The VGPR count is printed."""
import os
import sys

import pytest

from conftest import PKG, ROOT

LIB = os.path.join(PKG, "libmpcqp.so")
KEYS = [(w, obs) for w in (32, 64) for obs in (0, 1)]
HV_MAX_DIRS, N64_MAX, MAX_N = 128, 56, 63
# the longest horizon of each pass width and the bytes include/mpcqp.h and DESIGN.md section 5g state for it
LONGEST = {64: N64_MAX, 32: MAX_N}
LDS_STATED = {64: 161168, 32: 100408}


def lds_bytes(N, W):
    """The header's formula: 30 N + 10 + 2 MPC_HV_MAX_DIRS doubles for the instance, 5 N (W + 1) for a pass."""
    return 8 * (30 * N + 10 + 2 * HV_MAX_DIRS + 5 * N * (W + 1))


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("ROCm LLVM tools not available")
    import __graft_entry__ as g
    g.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import hessvec_kernel_key, kernel_resources
    return {hessvec_kernel_key(k["name"]): k for k in kernel_resources(LIB) if hessvec_kernel_key(k["name"])}


def test_the_four_kernels_are_present(kernels):
    assert sorted(kernels) == KEYS


@pytest.mark.parametrize("w,obs", KEYS)
def test_no_scratch_and_the_stated_lds(kernels, w, obs):
    k = kernels[(w, obs)]
    assert k["scratch"] == 0, k
    static, dynamic = k["lds"], lds_bytes(LONGEST[w], w)
    assert static == 0, k                                    # every double is sized by the actual N at the launch
    assert static + dynamic == LDS_STATED[w] <= 160 * 1024, (static, dynamic)
    assert lds_bytes(N64_MAX + 1, 64) > 160 * 1024           # the table's threshold is the last N that fits W = 64
    assert 2 * lds_bytes(20, 64) <= 160 * 1024               # two workgroups per CU at N = 20
    assert k["vgpr"] > 0 and k["sgpr"] > 0, k                # the record was parsed
    print(f"mpc_hessvec_kernel<{w}, {obs}>: {k['vgpr']} VGPRs, {k['sgpr']} SGPRs, dynamic LDS {dynamic} B at N = "
          f"{LONGEST[w]}, scratch {k['scratch']}")


def test_the_launch_uses_the_formula():
    """The library's pass width and the bytes it asks for are the header's: read from the sources the launch uses."""
    src = open(os.path.join(PKG, "csrc", "hessvec_kernel.h")).read()
    assert "return 30 * N + 10 + 2 * MPC_HV_MAX_DIRS;" in src and "hv_inst_doubles(N) + 5 * N * (W + 1)" in src
    hdr = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    assert "#define MPC_HV_N64_MAX 56" in hdr and "#define MPC_HV_MAX_DIRS 128" in hdr
