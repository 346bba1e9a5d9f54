"""Build-time resource check of tail_select_kernel and tail_select_rows_wave_kernel (the tail selection behind
rc_tail_select_f64_async): their four + three instantiations are in the listing, none spills a VGPR, none uses scratch memory, and
each stays inside the workgroup size and the LDS it declares, with registers that let one workgroup run.  Reads the per-kernel resource metadata of the listing `make asm` leaves
behind, nothing else.  CPU test: hipcc cross-compiles without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "code-robchar_amd", "csrc")
KEYS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "max_flat_workgroup_size")
# (threads, values per thread and tile, cached): the dispatch of rc_tail_select_f64_async
INSTANCES = ((128, 32, 1), (256, 32, 1), (512, 32, 1), (512, 8, 0))
WAVE_INSTANCES = (2, 8, 32)                                  # values per lane of the wave-per-row route (K <= 128 / 512 / 2048)


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
            m = re.search(r"tail_select_kernelILi(\d+)ELi(\d+)ELb(\d)E", get("name"))
            if m:
                out[tuple(int(v) for v in m.groups())] = {k: int(get(k)) for k in KEYS}
            m = re.search(r"tail_select_rows_wave_kernelILi(\d+)E", get("name"))
            if m:
                out[int(m.group(1))] = {k: int(get(k)) for k in KEYS}
    return out


def test_every_instantiation_without_spill_or_scratch(resources):
    assert sorted(map(str, resources)) == sorted(map(str, INSTANCES + WAVE_INSTANCES)), sorted(map(str, resources))
    for inst, res in sorted(resources.items(), key=str):
        print(f"tail_select_kernel<{inst}>: {res}")
        assert res["vgpr_spill_count"] == 0, (inst, res)
        assert res["private_segment_fixed_size"] == 0, (inst, res)


def test_declared_workgroup_lds_and_registers(resources):
    """LDS: the 256-bin histogram, one packed 64-bit count per (value slot, wave) segment of a tile plus the tile total, three
    control words.  Registers: the waves of one workgroup share a CU's four SIMDs of 512 registers per lane"""
    for slots in WAVE_INSTANCES:                             # four rows per workgroup of 256, no LDS, one wave per SIMD
        res = resources[slots]
        assert res["max_flat_workgroup_size"] == 256 and res["group_segment_fixed_size"] == 0, (slots, res)
        assert res["vgpr_count"] + res["agpr_count"] <= 512, (slots, res)
    for (threads, u, cached), res in sorted((k, v) for k, v in resources.items() if isinstance(k, tuple)):
        assert res["max_flat_workgroup_size"] == threads, (threads, u, res)
        lds = 256 * 4 + (u * (threads // 64) + 1) * 8 + 3 * 4
        assert res["group_segment_fixed_size"] <= lds + 16, (threads, u, res, lds)             # (+ alignment padding)
        waves_per_simd = max(1, threads // 256)
        assert res["vgpr_count"] + res["agpr_count"] <= 512 // waves_per_simd, (threads, u, res)
