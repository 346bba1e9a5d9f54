"""The C entries of the pairwise Wasserstein matrix (ABI 18) exist and reject bad arguments before any HIP call, each with its
code and message; the Python layers validate before they touch the device - runs without a GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rc_wasserstein_matrix_f64_async", "rc_wasserstein_matrix_f64")


def header_text():
    return open(os.path.join(ROOT, "include", "robchar_hip.h")).read()


def test_header_and_exports():
    assert int(re.search(r"#define\s+RC_ABI_VERSION\s+(\d+)", header_text()).group(1)) >= 18
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    assert lib.rc_version() >= 18
    for symbol in SYMBOLS:
        assert symbol in libmod.EXPORTS and hasattr(lib, symbol)
        assert re.search(r"\b%s\s*\(" % symbol, header_text())
    text = " ".join(header_text().replace("\n *", "\n").split())
    comment = text[text.index("(ABI 18)"):text.index("int rc_wasserstein_matrix_f64_async")]
    for phrase in ("wasserstein.py", "W_1 = (1/K) sum_k |a_(k) - b_(k)|", "W_2 = sqrt((1/K) sum_k (a_(k) - b_(k))^2)", "sorted ascending",
                   "b = NULL", "CB is then ignored", "equals its transpose bit for bit", "exactly 0", "fma(d, d, acc)",
                   "A row holding any NaN gives NaN in its whole row and column", "No atomics", "RC_OK, nothing written",
                   "presorted = 0", "[CA][CB]", "[CA][CA]"):
        assert phrase in comment, phrase


def entries(lib):
    z = ctypes.c_void_p(0)

    def asynchronous(p, a, CA, b, CB, K, out):
        return lib.rc_wasserstein_matrix_f64_async(0, z, p, a, CA, b, CB, K, out)

    def blocking(p, a, CA, b, CB, K, out):
        return lib.rc_wasserstein_matrix_f64(0, p, a, CA, b, CB, K, 1, out)

    def blocking_sorting(p, a, CA, b, CB, K, out):
        return lib.rc_wasserstein_matrix_f64(0, p, a, CA, b, CB, K, 0, out)

    return asynchronous, blocking, blocking_sorting


@pytest.mark.parametrize("which", (0, 1, 2), ids=("async", "blocking", "blocking-sorting"))
def test_argument_validation_without_gpu(which):
    lib = importlib.import_module("code-robchar_amd._lib").load()
    call = entries(lib)[which]
    one = np.ones(64)
    out = np.full(64, 7.0)
    a, o, z = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(0)
    err = lambda: lib.rc_last_error()
    EINVAL, OK = -1, 0
    for p in (0, 3, -1):
        assert call(p, a, 2, a, 2, 8, o) == EINVAL and b"p must be 1 or 2" in err()
        assert call(p, z, 0, z, 0, 0, z) == EINVAL and b"p must be 1 or 2" in err()       # refused with an empty batch too
    for CA, CB, K in ((-1, 2, 8), (2, -1, 8), (2, 2, -8)):
        assert call(1, a, CA, a, CB, K, o) == EINVAL and b"CA, CB and K must be non-negative" in err()
    assert call(2, a, -1, z, 0, 8, o) == EINVAL and b"non-negative" in err()
    # empty batches: RC_OK, nothing written, no device needed - pointers are not looked at
    for CA, b, CB, K in ((0, a, 2, 8), (2, a, 0, 8), (2, a, 2, 0), (0, z, 0, 8), (2, z, 0, 0)):
        assert call(1, z, CA, b, CB, K, z) == OK and call(2, a, CA, b, CB, K, o) == OK
    assert np.all(out == 7.0)
    # NULL a or out
    assert call(1, z, 2, a, 2, 8, o) == EINVAL and b"NULL array pointer" in err()
    assert call(1, a, 2, a, 2, 8, z) == EINVAL and b"NULL array pointer" in err()
    # b = NULL: CB is ignored, whatever it holds - the call gets as far as the NULL check of `out`
    for CB in (0, 5, -3):
        assert call(1, a, 2, z, CB, 8, z) == EINVAL and b"NULL array pointer" in err()
    assert call(1, a, 2 ** 31, a, 2, 8, o) == EINVAL and b"too many rows" in err()
    assert call(1, a, 2, a, 2 ** 31, 8, o) == EINVAL and b"too many rows" in err()


def test_python_layer_validates_before_the_device():
    be = importlib.import_module("code-robchar_amd.backend")
    rm = importlib.import_module("code-robchar_amd.rim_metrics")
    a = np.zeros((2, 8))
    for p in (0, 3):
        with pytest.raises(ValueError, match="p must be 1 or 2"):
            be.wasserstein_matrix(a, p=p)
    with pytest.raises(ValueError, match="expected"):
        be.wasserstein_matrix(np.zeros(8))
    with pytest.raises(ValueError, match="same K"):
        be.wasserstein_matrix(a, np.zeros((2, 7)))
    with pytest.raises(ValueError, match="same K"):
        be.wasserstein_matrix(a, np.zeros(8))
    with pytest.raises(ValueError, match="p must be 1 or 2"):
        rm.wasserstein_matrix(a, p=4)
    mcmod = importlib.import_module("code-robchar_amd.mc_data_sim")
    assert hasattr(mcmod.MCDataSim, "get_wasserstein_dict") and not hasattr(mcmod.MCDataSim, "get_wd_data_c")
