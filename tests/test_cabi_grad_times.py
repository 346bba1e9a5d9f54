"""The C entry of the fidelity gradient on a grid of readout times (ABI 17) exists and rejects bad arguments before any HIP call;
the Python layer validates before it touches the library - runs without a GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "rc_mc_fidelity_grad_times_philox_f64_async"


def header_text():
    return open(os.path.join(ROOT, "include", "robchar_hip.h")).read()


def header_constant(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, header_text()).group(1))


def test_header_and_exports():
    assert header_constant("RC_ABI_VERSION") >= 17
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    assert lib.rc_version() >= 17
    assert SYMBOL in libmod.EXPORTS and hasattr(lib, SYMBOL)
    assert re.search(r"\b%s\s*\(" % SYMBOL, header_text())
    text = " ".join(header_text().replace("\n *", "\n").split())
    comment = text[text.index("(ABI 17)"):text.index("int " + SYMBOL)]
    assert "u_cj = T_c tscale_j + tshift_j" in comment
    assert "acc = w_0 v_0; acc = fma(w_j, v_j, acc)" in comment
    assert "(mean W^2, mean W dW/dx_0 .. mean W dW/dx_N)" in comment
    assert "BIT FOR BIT" in comment


def test_argument_validation_without_gpu():
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    nmax, mmax = header_constant("RC_MAX_NSPIN_GRAD"), header_constant("RC_MAX_TIMES")
    one = np.ones(4096)
    p, z = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(0)
    err = lambda: lib.rc_last_error()
    # (device, stream, N, in, out, h0d, h0o, ctrl, seed, offset, sigma, sigma_rows, shared, C, K, M, tscale, tshift, weights,
    #  wfid, wgrad, mean, moment)
    call = lambda N, a, b, ctrl, sigma, rows, C, K, M, wts, fid, grad, mean, moment, shared=0, sc=z, sh=z: getattr(lib, SYMBOL)(
        0, z, N, a, b, z, z, ctrl, 7, 0, sigma, rows, shared, C, K, M, sc, sh, wts, fid, grad, mean, moment)
    assert call(1, 0, 0, p, 0.05, z, 1, 1, 5, p, p, p, p, p) == -1 and b"N must be" in err()
    assert call(99, 0, 0, p, 0.05, z, 1, 1, 5, p, p, p, p, p) == -1 and b"N must be" in err()
    assert call(5, 0, 7, p, 0.05, z, 1, 1, 5, p, p, p, p, p) == -1 and b"out of range" in err()
    assert call(5, -1, 2, p, 0.05, z, 1, 1, 5, p, p, p, p, p) == -1 and b"out of range" in err()
    assert call(nmax + 1, 0, nmax, p, 0.05, z, 1, 1, 5, p, p, p, p, p) == -3 and b"N <= %d" % nmax in err()       # RC_ENOSUP
    assert nmax == 12 and b"N <= 12" in err()
    assert call(5, 0, 4, p, 0.05, z, -1, 1, 5, p, p, p, p, p) == -1 and b"non-negative" in err()
    assert call(5, 0, 4, p, 0.05, z, 1, -1, 5, p, p, p, p, p) == -1 and b"non-negative" in err()
    assert mmax == 64
    for M in (0, -1, mmax + 1):
        assert call(5, 0, 4, p, 0.05, z, 1, 1, M, p, p, p, p, p) == -1 and b"M must be" in err(), M
    assert call(5, 0, 4, p, 0.05, z, 1, 1, 5, z, p, p, p, p) == -1 and b"weights" in err()
    assert call(5, 0, 4, p, 0.05, z, 1, 1, 5, p, z, z, z, z) == -1 and b"no output" in err() and b"moment_out" in err()
    for shared in (0, 1):
        for bad in (-0.05, float("inf"), float("-inf"), float("nan")):
            assert call(5, 0, 4, p, bad, z, 1, 1, 5, p, p, p, p, p, shared) == -1 and b"sigma" in err(), bad
    assert call(5, 0, 4, z, 0.05, z, 1, 1, 5, p, p, p, p, p) == -1 and b"NULL" in err()
    # empty batches: RC_OK, nothing touched (NULL controllers pass), each output alone is enough, the grid arrays may be given
    assert call(5, 0, 4, z, 0.05, z, 0, 10, 1, p, p, z, z, z) == 0
    assert call(5, 0, 4, z, 0.0, z, 10, 0, mmax, p, z, z, z, p, 0, p, p) == 0
    assert call(5, 0, 4, z, -1.0, p, 10, 0, 5, p, z, z, p, z, 1) == 0                      # (sigma is not read beside sigma_rows)
    assert call(5, 0, 4, p, 0.05, z, 1 << 40, 1 << 20, 5, p, p, p, p, p) == -1 and b"too many tiles" in err()


def test_python_layer_validates_before_the_library():
    be = importlib.import_module("code-robchar_amd.backend")
    w = np.ones(3) / 3
    with pytest.raises(ValueError):
        be.mc_fidelity_grad_times_philox(np.zeros((1, 6)), 4, 5, 0, 9, seed=1, weights=w)                # geometry
    with pytest.raises(ValueError, match="weights"):
        be.mc_fidelity_grad_times_philox(np.zeros((1, 6)), 4, 5, 0, 4, seed=1)
    with pytest.raises(ValueError, match="one length"):
        be.mc_fidelity_grad_times_philox(np.zeros((1, 6)), 4, 5, 0, 4, seed=1, weights=w, tscale=np.ones(4))
    with pytest.raises(ValueError, match="1 .. 64"):
        be.mc_fidelity_grad_times_philox(np.zeros((1, 6)), 4, 5, 0, 4, seed=1, weights=np.ones(65))
    with pytest.raises(ValueError, match="want"):
        be.mc_fidelity_grad_times_philox(np.zeros((1, 6)), 4, 5, 0, 4, seed=1, weights=w, want=("wsum",))
    with pytest.raises(ValueError, match="controllers"):
        be.mc_fidelity_grad_times_philox(np.zeros((1, 7)), 4, 5, 0, 4, seed=1, weights=w)
    with pytest.raises(ValueError, match="n_draws"):
        be.mc_fidelity_grad_times_philox(np.zeros((1, 6)), -1, 5, 0, 4, seed=1, weights=w)
