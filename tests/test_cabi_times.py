"""The C entries of the fidelity on a grid of readout times (ABI 16) exist and reject bad arguments before any HIP call, each
with its code and message; the Python layer validates before it touches the device - runs without a GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rc_mc_fidelity_times_f64_async", "rc_mc_fidelity_times_f64", "rc_mc_fidelity_times_philox_f64_async",
           "rc_stats_times_general_tiles")
EINVAL, ENOSUP = -1, -3


def header_text():
    return open(os.path.join(ROOT, "include", "robchar_hip.h")).read()


def test_header_and_exports():
    assert int(re.search(r"#define\s+RC_ABI_VERSION\s+(\d+)", header_text()).group(1)) >= 16
    assert int(re.search(r"#define\s+RC_MAX_TIMES\s+(\d+)", header_text()).group(1)) == 64
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    assert lib.rc_version() >= 16
    for symbol in SYMBOLS:
        assert symbol in libmod.EXPORTS and hasattr(lib, symbol)
        assert re.search(r"\b%s\s*\(" % symbol, header_text())
    text = " ".join(header_text().replace("\n *", "\n").split())
    comment = text[text.index("(ABI 16) Fidelity on a grid"):text.index("int rc_mc_fidelity_times_f64_async")]
    for phrase in ("| T_c tscale[j] + tshift[j] |", "product rounded first, sum second", "[M][C][K]", "fma(weights[j], F_j, acc)",
                   "min_j F_j", "|t_cj (lambda_k - lambda_0)| < 2.1e8", "rc_stats_times_general_tiles", "RC_ENOSUP"):
        assert phrase in comment, phrase


def entries(lib):
    z = ctypes.c_void_p(0)

    def tensor_async(N, a, b, ring, ctrl, draws, C, K, M, w, fid, wsum, fmin):
        return lib.rc_mc_fidelity_times_f64_async(0, z, N, a, b, z, z, ring, ctrl, draws, -1, C, K, M, z, z, w, fid, wsum, fmin)

    def tensor_blocking(N, a, b, ring, ctrl, draws, C, K, M, w, fid, wsum, fmin):
        return lib.rc_mc_fidelity_times_f64(0, N, a, b, z, z, ring, ctrl, draws, -1, C, K, M, z, z, w, fid, wsum, fmin)

    def philox(N, a, b, ring, ctrl, draws, C, K, M, w, fid, wsum, fmin):
        return lib.rc_mc_fidelity_times_philox_f64_async(0, z, N, a, b, z, z, ring, ctrl, 1, 0, 0.05, z, C, K, M, z, z, w, fid, wsum, fmin)

    return tensor_async, tensor_blocking, philox


@pytest.mark.parametrize("which", (0, 1, 2), ids=("async", "blocking", "philox"))
def test_argument_validation_without_gpu(which):
    lib = importlib.import_module("code-robchar_amd._lib").load()
    call = entries(lib)[which]
    one = np.ones(4096)
    p, z = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(0)
    err = lambda: lib.rc_last_error()
    for M in (0, 65, -1):
        assert call(5, 0, 4, 0, p, p, 1, 8, M, p, p, p, p) == EINVAL and b"M must be in [1, 64]" in err(), M
    assert call(5, 0, 4, 0, p, p, 1, 8, 4, p, z, z, z) == EINVAL and b"no output" in err()
    assert call(5, 0, 4, 0, p, p, 1, 8, 4, z, p, p, p) == EINVAL and b"wsum_out needs weights" in err()
    assert call(1, 0, 0, 0, p, p, 1, 8, 4, p, p, p, p) == EINVAL and b"N must be" in err()
    assert call(17, 0, 16, 0, p, p, 1, 8, 4, p, p, p, p) == ENOSUP and b"N <= 16" in err()
    assert call(33, 0, 16, 0, p, p, 1, 8, 4, p, p, p, p) == EINVAL and b"N must be" in err()
    assert call(5, 0, 4, 1, p, p, 1, 8, 4, p, p, p, p) == ENOSUP and b"chain topology only" in err()
    for (a, b) in ((-1, 4), (5, 0), (0, 5), (0, -1)):
        assert call(5, a, b, 0, p, p, 1, 8, 4, p, p, p, p) == EINVAL and b"out of range" in err(), (a, b)
    assert call(5, 0, 4, 0, z, p, 1, 8, 4, p, p, p, p) == EINVAL and b"NULL array pointer" in err()          # NULL controllers
    if which < 2:
        assert call(5, 0, 4, 0, p, z, 1, 8, 4, p, p, p, p) == EINVAL and b"NULL array pointer" in err()      # NULL draws
    assert call(5, 0, 4, 0, p, p, -1, 8, 4, p, p, p, p) == EINVAL and call(5, 0, 4, 0, p, p, 1, -8, 4, p, p, p, p) == EINVAL
    assert call(5, 0, 4, 0, p, p, 2 ** 31, 8, 4, p, p, p, p) == EINVAL and b"too many tiles" in err()
    # empty batches: nothing written, no device needed; bad arguments are still refused with C = 0
    assert call(5, 0, 4, 0, z, z, 0, 8, 4, z, p, z, z) == 0 and call(5, 0, 4, 0, z, z, 3, 0, 4, z, z, z, p) == 0
    assert call(5, 0, 4, 0, z, z, 0, 8, 0, z, p, z, z) == EINVAL and b"M must be" in err()


def test_philox_entry_checks_sigma_and_the_tensor_entry_its_stride():
    lib = importlib.import_module("code-robchar_amd._lib").load()
    one = np.ones(64)
    p, z = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(0)
    for sigma in (-0.1, float("inf"), float("nan")):
        rc = lib.rc_mc_fidelity_times_philox_f64_async(0, z, 5, 0, 4, z, z, 0, p, 1, 0, sigma, z, 1, 8, 4, z, z, z, p, z, z)
        assert rc == EINVAL and b"sigma must be finite" in lib.rc_last_error()
    rc = lib.rc_mc_fidelity_times_f64_async(0, z, 5, 0, 4, z, z, 0, p, p, 7, 2, 8, 4, z, z, z, p, z, z)
    assert rc == EINVAL and b"draws_ctrl_stride overlaps" in lib.rc_last_error()


def test_python_layer_validates_before_the_device():
    be = importlib.import_module("code-robchar_amd.backend")
    noise = importlib.import_module("code-robchar_amd.noise")
    assert be.TIMES_OUTPUTS == ("fid", "wsum", "min") and be.MAX_TIMES == 64
    ctrl, draws = np.ones((2, 6)), np.zeros((2, 8, 5, 3))
    with pytest.raises(ValueError, match="want"):
        be.mc_fidelity_times(ctrl, draws, 5, 0, 4, want=("fid", "mean"))
    with pytest.raises(ValueError, match="want"):
        be.mc_fidelity_times(ctrl, draws, 5, 0, 4, want=())
    with pytest.raises(ValueError, match="needs weights"):
        be.mc_fidelity_times(ctrl, draws, 5, 0, 4, tshift=np.zeros(3), want=("wsum",))
    with pytest.raises(ValueError, match="one length"):
        be.mc_fidelity_times(ctrl, draws, 5, 0, 4, tscale=np.ones(3), tshift=np.zeros(4))
    for M in (0, 65):
        with pytest.raises(ValueError, match="1 .. 64"):
            be.mc_fidelity_times(ctrl, draws, 5, 0, 4, tshift=np.zeros(M))
    with pytest.raises(ValueError, match="N <= 16"):
        be.mc_fidelity_times(np.ones((2, 18)), np.zeros((2, 8, 17, 3)), 17, 0, 16)
    with pytest.raises(ValueError, match="draws"):
        be.mc_fidelity_times(ctrl, np.zeros((2, 8, 4, 3)), 5, 0, 4)
    with pytest.raises(ValueError, match="controllers"):
        be.mc_fidelity_times_philox(np.ones((2, 5)), 8, 5, 0, 4, seed=1)
    with pytest.raises(ValueError, match="sigma"):
        be.mc_fidelity_times_philox(ctrl, 8, 5, 0, 4, seed=1, sigma=np.ones(3))
    # readout_times: NumPy's |T a + b|
    T = np.array([2.5, -1.0])
    assert np.array_equal(be.readout_times(T, [1.0, -2.0], [0.0, 0.5]), np.abs(T[:, None] * np.array([1.0, -2.0]) + np.array([0.0, 0.5])))
    assert np.array_equal(be.readout_times(T), np.abs(T)[:, None])
    # the Gauss-Hermite nodes of the jitter: weights sum to 1, second moment sigma_t^2, symmetric
    tshift, w = noise.readout_jitter_nodes(0.3, order=8)
    x, wx = np.polynomial.hermite.hermgauss(8)
    assert np.array_equal(tshift, np.sqrt(2.0) * 0.3 * x) and np.array_equal(w, wx / np.sqrt(np.pi))
    assert abs(w.sum() - 1.0) < 1e-14 and abs((w * tshift ** 2).sum() - 0.09) < 1e-15 and abs((w * tshift).sum()) < 1e-16
    with pytest.raises(ValueError, match="order"):
        noise.readout_jitter_nodes(0.3, order=65)
    with pytest.raises(ValueError, match="sigma_t"):
        noise.readout_jitter_nodes(-1.0)
    model = noise.structured_perturbation(Nspin=5, inspin=0, outspin=4, topo="ring")
    with pytest.raises(NotImplementedError, match="chain topology"):
        model.fidelity_over_times(ctrl, draws, tshift=tshift)
