"""End-to-end fidelity without weights (rc::ends_amplitude in code-robchar_amd/csrc/tridiag_core.h): the host build of
chain_fidelity_fast<N, kWeightsEnds> against the oracle on DELOCALISED controllers - biases |B| <= 1 against the hopping
J = 1, T in [2, 30] - where most samples carry a fidelity the relative bound can bite on.  N = 3, 7, 8: all cofactor
products in one batch; N = 9, 13: two and three batches, each scaled by its own total; N = 2: the all-fp64 QL branch, one
reciprocal per eigenvalue; N = 14: the same branch, which keeps the weights at N >= 14 (registers) and has to meet the same
bounds.  Runs without a GPU (harness: tests/host/host_core.cpp, built as tests/test_host_core.py does)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import robchar_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.POINTER(ctypes.c_double)
ABS_TOL = 1e-10
REL_TOL = 1e-9
BIG = 1e-3                # the relative bound holds wherever the reference fidelity exceeds this
MIN_SHARE = 0.5           # ... and at least this share of the compared samples must (oracle alone: 0.76 ... 1.0 below)


@pytest.fixture(scope="module")
def host_ends(tmp_path_factory):
    out = tmp_path_factory.mktemp("hostamp") / "librc_hosttest.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                    os.path.join(ROOT, "tests", "host", "host_core.cpp")], check=True)
    lib = ctypes.CDLL(str(out))
    lib.rc_host_general_calls.restype = ctypes.c_longlong

    def fid(ctrl, draws, N):
        """chain_fidelity_fast<N, kWeightsEnds>, 0 -> N-1; returns (F, number of samples that left the fast path)."""
        lib.rc_host_set_variant(0)
        C, K = draws.shape[:2]
        ctrl = np.ascontiguousarray(ctrl, dtype=np.float64)
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        h0d, h0o = np.zeros(N), np.ones(max(N - 1, 1))
        res = np.empty((C, K))
        before = lib.rc_host_general_calls()
        rc = lib.rc_host_chain_fidelity(N, ctrl.ctypes.data_as(P), h0d.ctypes.data_as(P), h0o.ctypes.data_as(P),
                                        draws.ctypes.data_as(P), ctypes.c_longlong(C), ctypes.c_longlong(K),
                                        0, N - 1, res.ctypes.data_as(P))
        assert rc == 0
        return res, lib.rc_host_general_calls() - before
    return fid


def _deloc(N, C=12, K=40):
    rng = np.random.default_rng(7100 + N)
    ctrl = np.empty((C, N + 1))
    ctrl[:, :N] = rng.uniform(-1.0, 1.0, (C, N))
    ctrl[:, N] = rng.uniform(2.0, 30.0, C)
    draws = 0.05 * rng.standard_normal((C, K, N, 3))
    return ctrl, draws


@pytest.mark.parametrize("N", [2, 3, 7, 8, 9, 13, 14])
def test_ends_amplitude_vs_oracle_delocalised(host_ends, N):
    ctrl, draws = _deloc(N)
    want = orc.fidelity_eigh(ctrl, draws, N, 0, N - 1)
    big = want > BIG
    assert big.mean() >= MIN_SHARE, (N, float(big.mean()))
    got, general = host_ends(ctrl, draws, N)
    assert general == 0, (N, general)                 # the fast path itself is what is compared
    err = np.abs(got - want)
    rel = (err[big] / want[big]).max()
    print(f"N={N}: share F>1e-3 {big.mean():.3f}  max abs {err.max():.3e}  max rel {rel:.3e}")
    assert err.max() <= ABS_TOL, (N, float(err.max()))
    assert rel <= REL_TOL, (N, float(rel))


@pytest.fixture(scope="module")
def host_paths(tmp_path_factory):
    """tests/host/host_ends_weights.cpp: chain_fidelity_fast<N, kWeightsEnds, AMPLITUDE> with AMPLITUDE chosen at run time."""
    out = tmp_path_factory.mktemp("hostpaths") / "librc_hostpaths.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                    os.path.join(ROOT, "tests", "host", "host_ends_weights.cpp")], check=True)
    lib = ctypes.CDLL(str(out))
    lib.rc_host_ends_fidelity.restype = ctypes.c_longlong

    def fid(ctrl, draws, N, amplitude):
        C, K = draws.shape[:2]
        ctrl = np.ascontiguousarray(ctrl, dtype=np.float64)
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        h0d, h0o = np.zeros(N), np.ones(N - 1)
        res = np.empty((C, K))
        left = lib.rc_host_ends_fidelity(N, int(amplitude), ctrl.ctypes.data_as(P), h0d.ctypes.data_as(P), h0o.ctypes.data_as(P),
                                         draws.ctypes.data_as(P), ctypes.c_longlong(C), ctypes.c_longlong(K), res.ctypes.data_as(P))
        assert left >= 0
        return res, left
    return fid


@pytest.mark.parametrize("N", [3, 5, 7, 9, 10, 13])
def test_weights_path_keeps_its_host_coverage(host_paths, N):
    """The weights + phase loop (AMPLITUDE = false: the directional kernel's path at N <= 13) beside the weight-free path, on
    the same delocalised samples: each within the bounds of the oracle comparison, none leaving the fast path."""
    ctrl, draws = _deloc(N)
    want = orc.fidelity_eigh(ctrl, draws, N, 0, N - 1)
    big = want > BIG
    assert big.mean() >= MIN_SHARE, (N, float(big.mean()))
    got = {}
    for amplitude in (False, True):
        got[amplitude], left = host_paths(ctrl, draws, N, amplitude)
        assert left == 0, (N, amplitude, left)
        err = np.abs(got[amplitude] - want)
        rel = (err[big] / want[big]).max()
        print(f"N={N} amplitude={amplitude}: max abs {err.max():.3e}  max rel {rel:.3e}")
        assert err.max() <= ABS_TOL, (N, amplitude, float(err.max()))
        assert rel <= REL_TOL, (N, amplitude, float(rel))
    print(f"N={N}: max |F_amplitude - F_weights| {np.abs(got[True] - got[False]).max():.3e}")


def test_cut_bonds_give_zero_on_the_fast_path(host_ends):
    """One exactly cancelled coupling: the product of the squared couplings carries 1e-300 and F is zero at that level; two
    of them: the product underflows and F = 0 exactly.  Finite, and no sample leaves the fast path."""
    N = 7
    ctrl, draws = _deloc(N, C=2, K=8)
    draws[0, :, 3, 1] = -1.0
    draws[0, :, 3, 2] = 0.0
    draws[1, :, 2, 1] = -1.0
    draws[1, :, 2, 2] = 0.0
    draws[1, :, 5, 1] = -1.0
    draws[1, :, 5, 2] = 0.0
    got, general = host_ends(ctrl, draws, N)
    assert general == 0
    assert np.isfinite(got).all()
    assert (got[0] >= 0).all() and got[0].max() < 1e-290, got[0]
    assert (got[1] == 0.0).all(), got[1]


def test_large_spectral_scale_stays_in_range(host_ends):
    """Biases of 1e4: a cofactor product reaches (2e4)^36 ~ 1e155 at N = 7 - in range, but its square is not; the phase
    sum is scaled by the reciprocal total before it is squared.  Every sample stays on the fast path; 1e-8 = the phase
    error eps |T lam| of the oracle's own eigenvalues at this scale."""
    N = 7
    rng = np.random.default_rng(7207)
    ctrl = np.empty((4, N + 1))
    ctrl[:, :N] = rng.uniform(-1e4, 1e4, (4, N))
    ctrl[:, N] = rng.uniform(2.0, 30.0, 4)
    draws = 0.05 * rng.standard_normal((4, 16, N, 3))
    got, general = host_ends(ctrl, draws, N)
    want = orc.fidelity_eigh(ctrl, draws, N, 0, N - 1)
    assert general == 0
    assert np.isfinite(got).all() and np.abs(got - want).max() < 1e-8
