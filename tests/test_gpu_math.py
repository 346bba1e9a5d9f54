"""The device's fp64 primitives against mpmath (tests/math_checks.py), and large angles through the fidelity kernels.

tests/host/hip_math_probe.cpp is built ONCE per module with hipcc straight from csrc/ (it links nothing from the library) and run
ONCE, in a subprocess under its own time limit: one launch per primitive on the chosen inputs of math_checks, the tables in LDS as
in the product kernels.  The checks are the ones tests/test_math_checks.py runs on the host build and on the NumPy restatement -
the same inputs, the same references, the same bars -, now with the hardware's v_rsq_f64 / v_rcp_f64 seeds, the device's
ln_table and box_muller_pair, and the host compilation of the two sincos routines in the same binary as their bit-for-bit twin."""
import os
import shutil

import numpy as np
import pytest

import math_checks as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    d = tmp_path_factory.mktemp("mathprobe")
    fn = mc.ProbeFn(mc.build_probe(d, hipcc), d, timeout=120)
    fn.prefetch(mc.standard_requests())
    assert fn.runs == 1
    return fn


@pytest.mark.parametrize("check", mc.ALL_CHECKS, ids=lambda c: c.__name__)
def test_device_primitive(probe, check):
    check(probe)
    assert probe.runs == 1                         # everything came from the one run of the program


@pytest.mark.parametrize("scale", mc.SCALES)
def test_device_box_muller_pair(probe, scale):
    """every chosen (a, b) within 16 * 2^-53 * scale * radius of mpmath - and a = 2^53 - 1 (u1 == 1: NaN before the radicand got
    its nudge) finite and within 1e-15 of the definition's 0"""
    mc.check_box_muller(probe, scale)
    assert probe.runs == 1


def test_device_sincos_twin_is_there(probe):
    """the bit-for-bit comparison of the two sincos routines is against the HOST compilation of the same binary, not against nothing"""
    for name, x in (("sincos_table", mc.sincos_table_inputs()), ("sincos_reduced", mc.sincos_reduced_inputs())):
        out, twin = probe(name, x)
        assert twin is not None and twin is not out and twin.shape == out.shape


@pytest.mark.parametrize("N", mc.LA_NS)
def test_large_angles_closed_form(be, N):
    """The parity tests end at |T lam| ~ 1e4.  The spin-j chain (equally spaced levels, fidelity in closed form at any T), from both
    ends to every site, kernels auto / tridiag_ql / tridiag_adj, C = 3, K = 65, T such that the largest |T (lam_k - lam_0)| is 1e5,
    1e6, 1e7, 1e8 and 0.9 of sincos_table's domain (2^31 pi/32 = 2.1e8) - against the closed form in mpmath at the fp64 inputs,
    |dF| <= 1e-10 + 8 * 2^-53 * angle_max * (1 - 1/N) (math_checks.large_angle_bar)."""
    def fid(ctrl, draws, n, a, b, off, kern):
        return be.mc_fidelity(ctrl, draws, n, a, b, h0_offdiag=off, kernel=kern)
    for target in mc.LA_TARGETS:
        mc.check_large_angles(fid, N, target, kernels=("auto", "tridiag_ql", "tridiag_adj"))
