"""The C entries of the noise sensitivity (ABI 8) exist and reject bad arguments before any HIP call - runs without a GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rc_mc_fidelity_sens_f64_async", "rc_mc_fidelity_sens_f64", "rc_stats_sens_general_tiles")


def header_text():
    return open(os.path.join(ROOT, "include", "robchar_hip.h")).read()


def header_constant(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, header_text()).group(1))


def test_header_and_exports():
    assert header_constant("RC_ABI_VERSION") >= 8
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    assert lib.rc_version() >= 8
    for name in SYMBOLS:
        assert name in libmod.EXPORTS and hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header_text()), name


def test_argument_validation_without_gpu():
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    nmax = header_constant("RC_MAX_NSPIN_GRAD")
    one = np.ones(4096)
    p, z = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(0)
    err = lambda: lib.rc_last_error()
    # rc_mc_fidelity_sens_f64(device, N, in, out, h0d, h0o, ctrl, draws, stride, C, K, fid, sens, mean)
    for call in (lambda *a: lib.rc_mc_fidelity_sens_f64(0, *a), lambda *a: lib.rc_mc_fidelity_sens_f64_async(0, z, *a)):
        assert call(1, 0, 0, z, z, p, p, -1, 1, 1, p, p, p) == -1 and b"N must be" in err()
        assert call(99, 0, 0, z, z, p, p, -1, 1, 1, p, p, p) == -1 and b"N must be" in err()
        assert call(5, 0, 7, z, z, p, p, -1, 1, 1, p, p, p) == -1 and b"out of range" in err()
        assert call(5, -1, 2, z, z, p, p, -1, 1, 1, p, p, p) == -1 and b"out of range" in err()
        assert call(nmax + 1, 0, nmax, z, z, p, p, -1, 1, 1, p, p, p) == -3 and b"N <= %d" % nmax in err()      # RC_ENOSUP
        assert b"sensitivity" in err()
        assert call(5, 0, 4, z, z, p, p, -1, 1, 1, z, z, z) == -1 and b"no output" in err() and b"sens_out" in err()
        assert call(5, 0, 4, z, z, p, p, -1, -1, 1, p, p, p) == -1 and b"non-negative" in err()
        assert call(5, 0, 4, z, z, p, p, -1, 1, -1, p, p, p) == -1 and b"non-negative" in err()
        assert call(5, 0, 4, z, z, p, p, 3, 2, 4, p, p, p) == -1 and b"overlaps" in err()                        # stride < K N 3
        assert call(5, 0, 4, z, z, z, p, -1, 1, 1, p, p, p) == -1 and b"NULL" in err()
        assert call(5, 0, 4, z, z, p, z, -1, 1, 1, p, p, p) == -1 and b"NULL" in err()
        assert call(5, 0, 4, z, z, z, z, -1, 0, 10, p, z, z) == 0                                                # empty batch
        assert call(5, 0, 4, z, z, z, z, -1, 10, 0, z, z, p) == 0


def test_python_layer_validates_before_the_library():
    be = importlib.import_module("code-robchar_amd.backend")
    noise = importlib.import_module("code-robchar_amd.noise")
    with pytest.raises(ValueError):
        be.mc_fidelity_sens(np.zeros((1, 6)), np.zeros((1, 4, 5, 3)), 5, 0, 9)
    with pytest.raises(ValueError, match="want"):
        be.mc_fidelity_sens(np.zeros((1, 6)), np.zeros((1, 4, 5, 3)), 5, 0, 4, want=("grad",))
    with pytest.raises(ValueError, match="want"):
        be.mc_fidelity_sens(np.zeros((1, 6)), np.zeros((1, 4, 5, 3)), 5, 0, 4, want=())
    nm = noise.structured_perturbation(Nspin=5, inspin=0, outspin=4, noise=0.05, topo="ring")
    for call in (lambda: nm.fidelity_sens_from_draws(np.zeros((1, 6)), np.zeros((1, 4, 5, 3))),
                 lambda: nm.noise_sensitivity(np.zeros((1, 6)), np.zeros((4, 5, 3))), lambda: nm.nominal_sensitivity(np.zeros((1, 6)))):
        with pytest.raises(NotImplementedError):
            call()
