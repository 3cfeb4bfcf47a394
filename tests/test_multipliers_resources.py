"""Static resources of the multiplier kernels (CPU test: reads the gfx950 code object's metadata from libmpcqp.so with
the ROCm LLVM tools, tools/kernel_resources.py).  mpc_multipliers_kernel<GL, OBS> (csrc/multiplier_kernel.h) exists
for GL = 16, 32, 64 with and without obstacles, uses no scratch, and its static LDS per workgroup (one wavefront, one
instance) is the header's mu_lds_doubles at the longest horizon of the lane group: the figures DESIGN.md section 5f
states.  The VGPR count is printed."""
import os
import re

import pytest

from conftest import PKG, ROOT

LIB = os.path.join(PKG, "libmpcqp.so")
KEYS = [(gl, obs) for gl in (16, 32, 64) for obs in (0, 1)]
# bytes of LDS per workgroup
LDS_STATED = {16: 52232, 32: 71304, 64: 109448}


def _key(name):
    m = re.search(r"mpc_multipliers_kernelILi(\d+)ELb([01])E", name)
    return tuple(int(x) for x in m.groups()) if m else None


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("ROCm LLVM tools not available")
    import __graft_entry__ as g
    g.build()
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    return {_key(k["name"]): k for k in kernel_resources(LIB) if _key(k["name"])}


def test_the_six_kernels_are_present(kernels):
    assert sorted(kernels) == KEYS


@pytest.mark.parametrize("gl,obs", KEYS)
def test_no_scratch_and_the_stated_lds(kernels, gl, obs):
    k = kernels[(gl, obs)]
    assert k["scratch"] == 0, k
    n = gl - 1
    doubles = 6 * (n + 1) + 12 * n + 64 + (n + 64) + 2 * n * 65 + 64 * 65
    assert k["lds"] == 8 * doubles and k["lds"] <= LDS_STATED[gl] <= 160 * 1024, k
    assert k["vgpr"] > 0 and k["sgpr"] > 0, k                # the record was parsed
    print(f"mpc_multipliers_kernel<{gl}, {obs}>: {k['vgpr']} VGPRs, {k['sgpr']} SGPRs, {k['lds']} B LDS, scratch {k['scratch']}")
