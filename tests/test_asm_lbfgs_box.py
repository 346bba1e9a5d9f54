"""Build-time resource check of the BOXED batched L-BFGS kernels (lbfgs_advance_box_kernel<3 .. 13> and lbfgs_init_box_kernel
behind rc_lbfgs_advance_box_f64_async / rc_lbfgs_init_box_f64_async): the 11 + 1 instantiations are in the listing, none spills a
register, none uses scratch memory or LDS, and the workgroup is one wave.  Reads the per-kernel resource metadata of the listing
`make asm` leaves behind, nothing else.  CPU test: hipcc cross-compiles without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "code-robchar_amd", "csrc")
KEYS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "max_flat_workgroup_size")
NDIMS = tuple(range(3, 14))


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
            m = re.search(r"lbfgs_advance_box_kernelILi(\d+)E", get("name"))
            if m:
                out[int(m.group(1))] = {k: int(get(k)) for k in KEYS}
            m = re.search(r"\d+lbfgs_(init)_box_kernelE", get("name"))
            if m:
                out[m.group(1)] = {k: int(get(k)) for k in KEYS}
    return out


def test_every_instantiation_without_spill_scratch_or_lds(resources):
    assert sorted(map(str, resources)) == sorted(map(str, NDIMS + ("init",))), sorted(map(str, resources))
    for inst, res in sorted(resources.items(), key=str):
        print(f"boxed lbfgs kernel <{inst}>: {res}")
        assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0, (inst, res)
        assert res["private_segment_fixed_size"] == 0 and res["group_segment_fixed_size"] == 0, (inst, res)
        assert res["max_flat_workgroup_size"] == 64, (inst, res)
        assert res["vgpr_count"] + res["agpr_count"] <= 512, (inst, res)         # one wave per workgroup: a SIMD's whole file
