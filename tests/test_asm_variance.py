"""Build-time resource check of the pick-freeze kernel (mc_fid_pickfreeze_philox_kernel<N, MODE>, N = 2 .. 13, both eigenvalue-only
weight modes) from the per-kernel metadata of the listing `make asm` leaves behind for the sixth translation unit
(robchar_vidx.gfx950.s) and nothing else: every instantiation is there, none spills a VGPR, none uses scratch, and registers and
LDS allow the residency the launch bounds declare.  `min_waves` below restates `pickfreeze_min_waves` of
k_fidelity_pickfreeze.inc.h and moves with it.  (tests/test_asm_sobol.py holds the older units' listings to their golden file.)
CPU test: hipcc cross-compiles without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from test_asm_sobol import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "code-robchar_amd", "csrc")


@pytest.fixture(scope="module")
def listing():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    subprocess.run(["make", "-j4", "-C", CSRC, "asm"], check=True, capture_output=True)
    return kernel_resources(os.path.join(CSRC, "robchar_vidx.gfx950.s"))


def min_waves(n):
    """pickfreeze_min_waves of k_fidelity_pickfreeze.inc.h"""
    return 3 if n <= 3 else (2 if n <= 7 else 1)


def test_every_pickfreeze_kernel_without_spill_or_scratch(listing):
    found = {}
    for name, (res,) in listing.items():
        print(name, res)
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (name, res)
        m = re.search(r"mc_fid_pickfreeze_philox_kernelILi(\d+)ELi(\d+)E", name)
        if m:
            n = int(m.group(1))
            found[(n, int(m.group(2)))] = res
            assert res["vgpr_count"] + res["agpr_count"] <= 512 // min_waves(n), (name, res)
            # one wave per workgroup, four SIMDs per compute unit, 160 KiB of LDS
            assert 4 * min_waves(n) * res["group_segment_fixed_size"] <= 160 * 1024, (name, res)
            assert res["max_flat_workgroup_size"] == 64
    assert sorted({n for n, _ in found}) == list(range(2, 14)) and len(found) == 24, sorted(found)
    assert sorted({mode for _, mode in found}) == [1, 2]                  # rc::kWeightsAdjugate, rc::kWeightsEnds
    assert sum("mc_fid_pickfreeze_mean_kernel" in k for k in listing) == 1


def test_the_unit_has_a_listing_of_its_own(listing):
    main = kernel_resources(os.path.join(CSRC, "robchar_hip.gfx950.s"))
    qmc = kernel_resources(os.path.join(CSRC, "robchar_qmc.gfx950.s"))
    assert not any("pickfreeze" in k for k in main) and not any("pickfreeze" in k for k in qmc)
