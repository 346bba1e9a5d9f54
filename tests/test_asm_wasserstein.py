"""Build-time resource check of wasserstein_tile_kernel<1>, <2> and wasserstein_finish_kernel<1>, <2>, from the kernel metadata of
the listing `make asm` leaves behind and nothing else (register counts, spill counts, scratch size, LDS bytes): no scratch, no VGPR
spill, and LDS and registers consistent with the occupancy the launch bounds claim - two workgroups of 256 threads per CU, i.e.
two waves per SIMD.  CPU test: hipcc cross-compiles without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "code-robchar_amd", "csrc")
KEYS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "max_flat_workgroup_size")
TILE, STEP, LDS_STRIDE, THREADS = 64, 32, 66, 256            # rcwd::kTile, kStep, kLdsStride, kThreads
WAVES_PER_SIMD = 2                                           # __launch_bounds__(kThreads, 2)
VGPR_FILE, LDS_PER_CU = 512, 163840                          # registers per lane of a SIMD, bytes of LDS of a CU (gfx950)


@pytest.fixture(scope="module")
def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    subprocess.run(["make", "-j4", "-C", CSRC, "asm"], check=True, capture_output=True)
    text = open(os.path.join(CSRC, "robchar_hip.gfx950.s")).read()
    out = {}
    for chunk in text.split("amdhsa.kernels:")[1:]:                      # one metadata document per translation unit
        for block in chunk.split("  - .agpr_count:")[1:]:
            block = ".agpr_count:" + block
            get = lambda key: re.search(r"\.%s:\s+(\S+)" % key, block).group(1)
            m = re.search(r"wasserstein_(tile|finish)_kernelILi(\d)E", get("name"))
            if m:
                out[(m.group(1), int(m.group(2)))] = {k: int(get(k)) for k in KEYS}
    return out


def test_every_instantiation_without_spill_or_scratch(resources):
    assert sorted(resources) == [("finish", 1), ("finish", 2), ("tile", 1), ("tile", 2)], sorted(resources)
    for inst, res in sorted(resources.items()):
        print(f"wasserstein kernel {inst}: {res}")
        assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0, (inst, res)
        assert res["private_segment_fixed_size"] == 0, (inst, res)


def test_lds_and_registers_allow_the_claimed_occupancy(resources):
    """the tile kernel: two LDS images of kStep x kLdsStride doubles; two workgroups per CU need at most half the LDS and, at two
    waves per SIMD, at most 256 of the 512 registers per lane"""
    for p in (1, 2):
        res = resources[("tile", p)]
        assert res["max_flat_workgroup_size"] == THREADS, res
        assert res["group_segment_fixed_size"] == 2 * STEP * LDS_STRIDE * 8, res
        assert WAVES_PER_SIMD * res["group_segment_fixed_size"] <= LDS_PER_CU, res
        assert res["vgpr_count"] + res["agpr_count"] <= VGPR_FILE // WAVES_PER_SIMD, res
        # the four levels of 4 x 4 sums alone are 128 registers: fewer would mean they are not all kept in registers
        assert res["vgpr_count"] >= 4 * 16 * 2, res
        fin = resources[("finish", p)]
        assert fin["group_segment_fixed_size"] == 0 and fin["vgpr_count"] + fin["agpr_count"] <= 64, fin
