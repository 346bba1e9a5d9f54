"""The C entries of the fidelity gradient (ABI 7) reject bad arguments before any HIP call - runs without a GPU."""
import ctypes
import importlib
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    text = open(os.path.join(ROOT, "include", "robchar_hip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


def test_header_constants():
    assert header_constant("RC_MAX_NSPIN_GRAD") >= 12
    assert header_constant("RC_ABI_VERSION") >= 7
    be = importlib.import_module("code-robchar_amd.backend")
    assert be.max_nspin_grad() == header_constant("RC_MAX_NSPIN_GRAD")


def test_argument_validation_without_gpu():
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    nmax = header_constant("RC_MAX_NSPIN_GRAD")
    one = np.ones(4096)
    p, z = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(0)
    err = lambda: lib.rc_last_error()
    # rc_mc_fidelity_grad_f64(device, N, in, out, h0d, h0o, ctrl, draws, stride, C, K, fid, grad, mean)
    for call in (lambda *a: lib.rc_mc_fidelity_grad_f64(0, *a), lambda *a: lib.rc_mc_fidelity_grad_f64_async(0, z, *a)):
        assert call(1, 0, 0, z, z, p, p, -1, 1, 1, p, p, p) == -1 and b"N must be" in err()
        assert call(99, 0, 0, z, z, p, p, -1, 1, 1, p, p, p) == -1 and b"N must be" in err()
        assert call(5, 0, 7, z, z, p, p, -1, 1, 1, p, p, p) == -1 and b"out of range" in err()
        assert call(5, -1, 2, z, z, p, p, -1, 1, 1, p, p, p) == -1 and b"out of range" in err()
        assert call(nmax + 1, 0, nmax, z, z, p, p, -1, 1, 1, p, p, p) == -3 and b"N <= %d" % nmax in err()      # RC_ENOSUP
        assert call(5, 0, 4, z, z, p, p, -1, 1, 1, z, z, z) == -1 and b"no output" in err()
        assert call(5, 0, 4, z, z, p, p, -1, -1, 1, p, p, p) == -1 and b"non-negative" in err()
        assert call(5, 0, 4, z, z, p, p, 3, 2, 4, p, p, p) == -1 and b"overlaps" in err()                        # stride < K N 3
        assert call(5, 0, 4, z, z, z, p, -1, 1, 1, p, p, p) == -1 and b"NULL" in err()
        assert call(5, 0, 4, z, z, p, z, -1, 1, 1, p, p, p) == -1 and b"NULL" in err()
        assert call(5, 0, 4, z, z, z, z, -1, 0, 10, p, z, z) == 0                                                # empty batch
        assert call(5, 0, 4, z, z, z, z, -1, 10, 0, z, z, p) == 0
    assert "rc_mc_fidelity_grad_f64" in libmod.EXPORTS and "rc_mc_fidelity_grad_f64_async" in libmod.EXPORTS


def test_python_layer_validates_before_the_library():
    import pytest
    be = importlib.import_module("code-robchar_amd.backend")
    with pytest.raises(ValueError):
        be.mc_fidelity_grad(np.zeros((1, 6)), np.zeros((1, 4, 5, 3)), 5, 0, 9)
    with pytest.raises(ValueError, match="want"):
        be.mc_fidelity_grad(np.zeros((1, 6)), np.zeros((1, 4, 5, 3)), 5, 0, 4, want=("hessian",))
    with pytest.raises(ValueError, match="want"):
        be.mc_fidelity_grad(np.zeros((1, 6)), np.zeros((1, 4, 5, 3)), 5, 0, 4, want=())
