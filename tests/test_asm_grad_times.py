"""Build-time resource check of mc_fid_grad_times_philox_kernel (the fidelity gradient on a grid of readout times): the eleven
instantiations N = 2 .. 12 are in the listing, in the GRADIENT translation unit (beside mc_fid_grad_philox_kernel, not in a unit
of their own and not in the readout-time unit), none spills a VGPR, none uses scratch memory, and registers and LDS allow the
residency the kernel declares.  Reads the per-kernel resource metadata of the listing `make asm` leaves behind, nothing else.
CPU test: hipcc cross-compiles without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "code-robchar_amd", "csrc")
KEYS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def waves_of(n):
    """the launch bounds of k_fidelity_grad_times_philox.inc.h (grad_times_min_waves: mc_fid_grad_philox_kernel's), restated"""
    return 4 if n <= 3 else (3 if n <= 5 else (2 if n <= 7 else 1))


@pytest.fixture(scope="module")
def units():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    subprocess.run(["make", "-j4", "-C", CSRC, "asm"], check=True, capture_output=True)
    text = open(os.path.join(CSRC, "robchar_hip.gfx950.s")).read()
    out = []
    for chunk in text.split("amdhsa.kernels:")[1:]:                      # one metadata document per translation unit
        found = {"times": {}, "names": set()}
        for block in chunk.split("  - .agpr_count:")[1:]:
            block = "  - .agpr_count:" + block
            get = lambda key: re.search(r"\.%s:\s+(\S+)" % key, block).group(1)
            name = get("name")
            found["names"].add(re.sub(r"ILi\d+E.*", "", name))
            m = re.search(r"mc_fid_grad_times_philox_kernelILi(\d+)E", name)
            if m:
                found["times"][int(m.group(1))] = {k: int(get(k)) for k in KEYS}
        out.append(found)
    return out


def test_eleven_instantiations_in_the_gradient_unit(units):
    assert len(units) == 4                                               # no fifth translation unit
    mine = [u for u in units if u["times"]]
    assert len(mine) == 1
    unit = mine[0]
    assert sorted(unit["times"]) == list(range(2, 13)), sorted(unit["times"])
    assert any("mc_fid_grad_philox_kernel" in n for n in unit["names"]) and any("mc_fid_grad_kernel" in n for n in unit["names"])
    assert not any("mc_fid_times_kernel" in n for n in unit["names"])


def test_no_spill_no_scratch_and_the_declared_residency(units):
    res_of = [u for u in units if u["times"]][0]["times"]
    for n, res in sorted(res_of.items()):
        print(f"mc_fid_grad_times_philox_kernel<{n}>: waves {waves_of(n)} {res}")
        assert res["vgpr_spill_count"] == 0, (n, res)
        assert res["private_segment_fixed_size"] == 0, (n, res)
        assert res["vgpr_count"] <= 512 // waves_of(n), (n, res)
        # one wave per workgroup, four SIMDs per compute unit, 160 KiB of LDS
        assert 4 * waves_of(n) * res["group_segment_fixed_size"] <= 160 * 1024, (n, res)
