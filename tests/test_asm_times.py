"""Build-time resource check of the readout-time kernels (mc_fid_times_kernel, mc_fid_times_philox_kernel): the 15 + 15
instantiations N = 2 .. 16 are in the listing of their own translation unit, none spills a VGPR, none uses scratch memory, and
registers and LDS allow the residency the kernels declare.  Reads the per-kernel resource metadata of the listing `make asm`
leaves behind, nothing else.  CPU test: hipcc cross-compiles without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "code-robchar_amd", "csrc")
KEYS = ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


@pytest.fixture(scope="module")
def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    subprocess.run(["make", "-j4", "-C", CSRC, "asm"], check=True, capture_output=True)
    text = open(os.path.join(CSRC, "robchar_hip.gfx950.s")).read()
    units = []
    for chunk in text.split("amdhsa.kernels:")[1:]:                      # one metadata document per translation unit
        found = {"mc_fid_times_kernel": {}, "mc_fid_times_philox_kernel": {}, "other": 0}
        for block in chunk.split("  - .agpr_count:")[1:]:
            get = lambda key: re.search(r"\.%s:\s+(\S+)" % key, block).group(1)
            m = re.search(r"\d+(mc_fid_times(?:_philox)?_kernel)ILi(\d+)E", get("name"))
            if m:
                found[m.group(1)][int(m.group(2))] = {k: int(get(k)) for k in KEYS}
            else:
                found["other"] += 1
        units.append(found)
    return units


def waves(kernel, n):
    """the launch bounds of k_fidelity_times.inc.h"""
    w = 5 if n <= 8 else (3 if n <= 12 else 2)
    if kernel == "mc_fid_times_philox_kernel":
        w = 1 if n >= 14 else min(w, 3)
    return w


def test_both_kernels_live_in_a_unit_of_their_own(resources):
    mine = [u for u in resources if u["mc_fid_times_kernel"] or u["mc_fid_times_philox_kernel"]]
    assert len(resources) == 4 and len(mine) == 1, [({k: len(v) if isinstance(v, dict) else v for k, v in u.items()}) for u in resources]
    unit = mine[0]
    assert unit["other"] == 0                                            # nothing else compiles with them
    assert sorted(unit["mc_fid_times_kernel"]) == list(range(2, 17))
    assert sorted(unit["mc_fid_times_philox_kernel"]) == list(range(2, 17))


def test_no_spill_no_scratch_and_the_declared_residency(resources):
    unit = [u for u in resources if u["mc_fid_times_kernel"]][0]
    for kernel in ("mc_fid_times_kernel", "mc_fid_times_philox_kernel"):
        for n, res in sorted(unit[kernel].items()):
            print(f"{kernel}<{n}>: {res}, {waves(kernel, n)} waves")
            assert res["vgpr_spill_count"] == 0, (kernel, n, res)
            assert res["private_segment_fixed_size"] == 0, (kernel, n, res)
            assert res["vgpr_count"] <= 512 // waves(kernel, n), (kernel, n, res)
            # one wave per workgroup, four SIMDs per compute unit, 160 KiB of LDS
            assert 4 * waves(kernel, n) * res["group_segment_fixed_size"] <= 160 * 1024, (kernel, n, res)
