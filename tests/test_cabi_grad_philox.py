"""The C entry of the fidelity gradient with the draws generated inside the kernel (ABI 10) exists and rejects bad arguments
before any HIP call; the Python layer validates before it touches the library - runs without a GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "rc_mc_fidelity_grad_philox_f64_async"


def header_text():
    return open(os.path.join(ROOT, "include", "robchar_hip.h")).read()


def header_constant(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, header_text()).group(1))


def test_header_and_exports():
    assert header_constant("RC_ABI_VERSION") >= 10
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    assert lib.rc_version() >= 10
    assert SYMBOL in libmod.EXPORTS and hasattr(lib, SYMBOL)
    assert re.search(r"\b%s\s*\(" % SYMBOL, header_text())
    # the header states both stream conventions, the bit identity, what moment_out holds and what a sigma = 0 row gives
    text = " ".join(header_text().replace("\n *", "\n").split())
    comment = text[text.index("(ABI 10)"):text.index("int " + SYMBOL)]
    assert "offset + ((c K + k) N + i) 3 + s" in comment
    assert "offset + (k N + i) 3 + s" in comment
    assert "BIT-IDENTICAL to the two-kernel route" in comment
    assert "(mean F^2, mean F dF/dx_0 .. mean F dF/dx_N)" in comment
    assert "sigma = 0 gives K identical samples" in comment


def test_argument_validation_without_gpu():
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    nmax = header_constant("RC_MAX_NSPIN_GRAD")
    one = np.ones(4096)
    p, z = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(0)
    err = lambda: lib.rc_last_error()
    # (device, stream, N, in, out, h0d, h0o, ctrl, seed, offset, sigma, sigma_rows, shared, C, K, fid, grad, mean, moment)
    call = lambda N, a, b, ctrl, sigma, rows, C, K, fid, grad, mean, moment, shared=0: lib.rc_mc_fidelity_grad_philox_f64_async(
        0, z, N, a, b, z, z, ctrl, 7, 0, sigma, rows, shared, C, K, fid, grad, mean, moment)
    assert call(1, 0, 0, p, 0.05, z, 1, 1, p, p, p, p) == -1 and b"N must be" in err()
    assert call(99, 0, 0, p, 0.05, z, 1, 1, p, p, p, p) == -1 and b"N must be" in err()
    assert call(5, 0, 7, p, 0.05, z, 1, 1, p, p, p, p) == -1 and b"out of range" in err()
    assert call(5, -1, 2, p, 0.05, z, 1, 1, p, p, p, p) == -1 and b"out of range" in err()
    assert call(nmax + 1, 0, nmax, p, 0.05, z, 1, 1, p, p, p, p) == -3 and b"N <= %d" % nmax in err()              # RC_ENOSUP
    assert nmax == 12 and b"N <= 12" in err() and b"gradient" in err()
    assert call(5, 0, 4, p, 0.05, z, 1, 1, z, z, z, z) == -1 and b"no output" in err() and b"moment_out" in err()
    assert call(5, 0, 4, p, 0.05, z, -1, 1, p, p, p, p) == -1 and b"non-negative" in err()
    assert call(5, 0, 4, p, 0.05, z, 1, -1, p, p, p, p) == -1 and b"non-negative" in err()
    for shared in (0, 1):
        for bad in (-0.05, float("inf"), float("-inf"), float("nan")):
            assert call(5, 0, 4, p, bad, z, 1, 1, p, p, p, p, shared) == -1 and b"sigma" in err(), bad
    assert call(5, 0, 4, z, 0.05, z, 1, 1, p, p, p, p) == -1 and b"NULL" in err()
    assert call(5, 0, 4, z, 0.05, z, 0, 10, p, z, z, z) == 0                                                      # empty batches
    assert call(5, 0, 4, z, 0.0, z, 10, 0, z, z, z, p) == 0
    assert call(5, 0, 4, z, -1.0, p, 10, 0, z, z, p, z, 1) == 0                          # (sigma is not read beside sigma_rows)
    assert call(5, 0, 4, p, 0.05, z, 1 << 40, 1 << 20, p, p, p, p) == -1 and b"too many tiles" in err()


def test_python_layer_validates_before_the_library():
    be = importlib.import_module("code-robchar_amd.backend")
    noise = importlib.import_module("code-robchar_amd.noise")
    assert be.GRAD_PHILOX_OUTPUTS == ("fid", "grad", "mean", "moment")
    with pytest.raises(ValueError):
        be.mc_fidelity_grad_philox(np.zeros((1, 6)), 4, 5, 0, 9, seed=1)                       # geometry
    with pytest.raises(ValueError, match="want"):
        be.mc_fidelity_grad_philox(np.zeros((1, 6)), 4, 5, 0, 4, seed=1, want=("sens",))
    with pytest.raises(ValueError, match="want"):
        be.mc_fidelity_grad_philox(np.zeros((1, 6)), 4, 5, 0, 4, seed=1, want=())
    with pytest.raises(ValueError, match="controllers"):
        be.mc_fidelity_grad_philox(np.zeros((1, 7)), 4, 5, 0, 4, seed=1)
    with pytest.raises(ValueError, match="n_draws"):
        be.mc_fidelity_grad_philox(np.zeros((1, 6)), -1, 5, 0, 4, seed=1)
    with pytest.raises(ValueError, match="sigma"):
        be.mc_fidelity_grad_philox(np.zeros((2, 6)), 4, 5, 0, 4, seed=1, sigma=np.array([0.1, 0.2, 0.3]))
    ring = noise.structured_perturbation(Nspin=5, inspin=0, outspin=4, noise=0.05, topo="ring")
    with pytest.raises(NotImplementedError):
        ring.fidelity_moments_philox(np.zeros((1, 6)), 4, seed=1)
    cplx = noise.structured_perturbation(Nspin=5, inspin=0, outspin=4, noise=0.05)
    cplx.HH[1, 0] += 0.3j
    cplx.HH[0, 1] -= 0.3j
    with pytest.raises(NotImplementedError, match="real static couplings"):
        cplx.fidelity_moments_philox(np.zeros((1, 6)), 4, seed=1)
