"""Build-time resource check of the Sobol kernels (sobol_draws_kernel and mc_fid_chain_sobol_kernel<N, MODE>, N = 2 .. 13, both
weight modes) from the per-kernel metadata of the listings `make asm` leaves behind and nothing else: every one is there, none
spills a VGPR, none uses scratch, and registers and LDS allow the residency the launch bounds declare.  The fifth translation unit
has a listing of its own (robchar_qmc.gfx950.s); robchar_hip.gfx950.s still holds the four units it held, and the resource
metadata of every kernel in it equals tests/golden/asm_resources_older_kernels.json, taken from the build before this unit existed
Maintenance: a pull request that changes an older kernel on purpose, or a compiler update, regenerates that file from its own
build - `make -C code-robchar_amd/csrc asm && python tests/test_asm_sobol.py --write-golden code-robchar_amd/csrc/robchar_hip.gfx950.s` -
and says so; the file carries the same note under "_about".  `min_waves` below restates `fid_sobol_min_waves` of
k_fidelity_sobol.inc.h (min(3, fid_min_waves) for the eigenvalue-only modes) and moves with it.
CPU test: hipcc cross-compiles without a GPU."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "code-robchar_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "asm_resources_older_kernels.json")
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "max_flat_workgroup_size")


def kernel_resources(path):
    out = {}
    for chunk in open(path).read().split("amdhsa.kernels:")[1:]:          # one metadata document per translation unit
        for block in chunk.split("  - .agpr_count:")[1:]:
            block = ".agpr_count:" + block
            get = lambda key: re.search(r"\.%s:\s+(\S+)" % key, block).group(1)
            out.setdefault(get("name"), []).append({k: int(get(k)) for k in KEYS})
    return out


@pytest.fixture(scope="module")
def listings():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    subprocess.run(["make", "-j4", "-C", CSRC, "asm"], check=True, capture_output=True)
    return (kernel_resources(os.path.join(CSRC, "robchar_hip.gfx950.s")), kernel_resources(os.path.join(CSRC, "robchar_qmc.gfx950.s")))


def min_waves(n):
    """fid_sobol_min_waves of k_fidelity_sobol.inc.h: min(3, fid_min_waves) - the eigenvalue-only modes"""
    return 3 if n <= 8 else 2


def test_every_sobol_kernel_without_spill_or_scratch(listings):
    _, qmc = listings
    fused = {}
    for name, (res,) in ((k, v) for k, v in qmc.items() if "sobol" in k):
        print(name, res)
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (name, res)
        m = re.search(r"mc_fid_chain_sobol_kernelILi(\d+)ELi(\d+)E", name)
        if m:
            n = int(m.group(1))
            fused[(n, int(m.group(2)))] = res
            assert res["vgpr_count"] + res["agpr_count"] <= 512 // min_waves(n), (name, res)
            # one wave per workgroup, four SIMDs per compute unit, 160 KiB of LDS
            assert 4 * min_waves(n) * res["group_segment_fixed_size"] <= 160 * 1024, (name, res)
            assert res["max_flat_workgroup_size"] == 64
    assert sorted({n for n, _ in fused}) == list(range(2, 14)) and len(fused) == 24, sorted(fused)
    assert sum("sobol_draws_kernel" in k for k in qmc) == 1


def test_older_kernels_keep_the_resources_of_the_build_before(listings):
    main, qmc = listings
    want = {k: v for k, v in json.load(open(GOLDEN)).items() if k != "_about"}
    assert not any("sobol" in k for k in main)                            # the new kernels live in their own unit and listing
    assert sorted(main) == sorted(want)
    for name in want:
        assert main[name] == want[name], (name, main[name], want[name])


if __name__ == "__main__" and "--write-golden" in sys.argv[1:]:
    about = json.load(open(GOLDEN))["_about"] if os.path.exists(GOLDEN) else ""
    table = {"_about": about, **kernel_resources(sys.argv[sys.argv.index("--write-golden") + 1])}
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
