"""Build-time resource check of bootstrap_replicates_kernel (both routes, both threshold counts) and bootstrap_summary_kernel,
from the kernel metadata of the listing `make asm` leaves behind and nothing else: no scratch, no VGPR spill, and the LDS route's
static LDS inside the 160 KiB of a gfx950 CU.  CPU test: hipcc cross-compiles without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "code-robchar_amd", "csrc")
KEYS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "max_flat_workgroup_size")
INSTANCES = ((2, 1), (8, 1), (2, 0), (8, 0))                 # (thresholds, LDS route): the dispatch of rc_bootstrap_metrics_f64_async
LDS_MAX_K = 18432


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
            m = re.search(r"bootstrap_replicates_kernelILi(\d+)ELb(\d)E", get("name"))
            if m:
                out[tuple(int(v) for v in m.groups())] = {k: int(get(k)) for k in KEYS}
            if "bootstrap_summary_kernel" in get("name"):
                out["summary"] = {k: int(get(k)) for k in KEYS}
    return out


def test_every_instantiation_without_spill_or_scratch(resources):
    assert sorted(map(str, resources)) == sorted(map(str, INSTANCES + ("summary",))), sorted(map(str, resources))
    for inst, res in sorted(resources.items(), key=str):
        print(f"bootstrap kernel {inst}: {res}")
        assert res["vgpr_spill_count"] == 0, (inst, res)
        assert res["private_segment_fixed_size"] == 0, (inst, res)


def test_lds_and_registers(resources):
    """LDS route: the row (18 432 doubles) and the 16 wave sums, inside a CU's 160 KiB; global route: the wave sums alone.  1024
    threads are four waves per SIMD: at most 128 registers per lane."""
    import importlib
    assert importlib.import_module("code-robchar_amd.bootstrap").LDS_MAX_K == LDS_MAX_K
    for (nq, lds), res in ((k, v) for k, v in resources.items() if k != "summary"):
        assert res["max_flat_workgroup_size"] == 1024, (nq, lds, res)
        assert res["vgpr_count"] + res["agpr_count"] <= 128, (nq, lds, res)
        if lds:
            assert LDS_MAX_K * 8 <= res["group_segment_fixed_size"] <= 163840, (nq, res)
        else:
            assert res["group_segment_fixed_size"] <= 1024, (nq, res)
    assert resources["summary"]["group_segment_fixed_size"] == 0
