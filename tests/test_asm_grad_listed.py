"""Build-time resource check of mc_fid_grad_listed_kernel (the listed-sample weighted fidelity-gradient kernel): the eleven
instantiations N = 2 .. 12 are in the listing, none spills a VGPR, none uses scratch memory, and registers and LDS allow the
residency the kernel declares.  Reads the per-kernel resource metadata of the listing `make asm` leaves behind, nothing else.
CPU test: hipcc cross-compiles without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "code-robchar_amd", "csrc")
KEYS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


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
            get = lambda key: re.search(r"\.%s:\s+(\S+)" % key, block).group(1)
            m = re.search(r"mc_fid_grad_listed_kernelILi(\d+)E", get("name"))
            if m:
                out[int(m.group(1))] = {k: int(get(k)) for k in KEYS}
    return out


def test_eleven_instantiations_without_spill_or_scratch(resources):
    assert sorted(resources) == list(range(2, 13)), sorted(resources)
    for n, res in sorted(resources.items()):
        print(f"mc_fid_grad_listed_kernel<{n}>: {res}")
        assert res["vgpr_spill_count"] == 0, (n, res)
        assert res["private_segment_fixed_size"] == 0, (n, res)


def test_registers_and_lds_allow_the_declared_residency(resources):
    """launch bounds per N (k_fidelity_grad_listed.inc.h: mc_fid_grad_philox_kernel's): four waves per SIMD up to N = 3, three up
    to N = 5, two up to N = 7, one above - the register count must fit 512 / waves, and the LDS of the waves of a CU (one wave
    per workgroup, four SIMDs) the 160 KiB"""
    for n, res in sorted(resources.items()):
        waves = 4 if n <= 3 else (3 if n <= 5 else (2 if n <= 7 else 1))
        assert res["vgpr_count"] <= 512 // waves, (n, res)
        assert 4 * waves * res["group_segment_fixed_size"] <= 160 * 1024, (n, res)
