"""The C entries of the boxed batched L-BFGS (ABI 14) exist and reject bad arguments before any HIP call; the Python layer validates
the bounds before it touches the device - runs without a GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rc_lbfgs_init_box_f64_async", "rc_lbfgs_advance_box_f64_async")


def header_text():
    return open(os.path.join(ROOT, "include", "robchar_hip.h")).read()


def test_header_and_exports():
    assert int(re.search(r"#define\s+RC_ABI_VERSION\s+(\d+)", header_text()).group(1)) >= 14
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    assert lib.rc_version() >= 14
    for symbol in SYMBOLS:
        assert symbol in libmod.EXPORTS and hasattr(lib, symbol)
        assert re.search(r"\b%s\s*\(" % symbol, header_text())
    text = " ".join(header_text().replace("\n *", "\n").split())
    comment = text[text.index("(ABI 14)"):text.index("int rc_lbfgs_init_box_f64_async")]
    for phrase in ("lbfgs.py", "nothing new is stored", "both required", "-inf / +inf", "x0 <- P(x0)", "gs < 0", "f_trial <= f + c1 gs",
                   "|x_i - P(x - g)_i| <= gtol", "x_i <= lo_i and g_i > 0", "x_i >= hi_i and g_i < 0", "P(x + t d)", "status 5",
                   "rc_lbfgs_result_f64_async"):
        assert phrase in comment, phrase


def test_argument_validation_without_gpu():
    lib = importlib.import_module("code-robchar_amd._lib").load()
    one = np.ones(4096)
    p, z = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(0)
    err = lambda: lib.rc_last_error()
    init = lambda n=8, m=5, C=4, x0=p, mask=z, lo=p, hi=p, state=p, trial=p: \
        lib.rc_lbfgs_init_box_f64_async(0, z, n, m, C, x0, mask, lo, hi, state, trial)
    adv = lambda n=8, m=5, C=4, kind=1, a=p, b=z, lo=p, hi=p, c1=1e-4, gtol=1e-6, ftol=0.0, maxiter=100, maxback=20, state=p, trial=p: \
        lib.rc_lbfgs_advance_box_f64_async(0, z, n, m, C, kind, 0.0, a, b, lo, hi, c1, gtol, ftol, maxiter, maxback, state, trial)
    for call in (init, adv):
        for n in (2, 14, -1):
            assert call(n, 5, 4) == -1 and b"ndim must be 3 .. 13" in err(), n
        for m in (0, 9):
            assert call(8, m, 4) == -1 and b"m must be 1 .. 8" in err(), m
        assert call(8, 5, -1) == -1 and b"non-negative" in err()
        assert call(8, 5, 0) == 0                                              # nothing to do
        assert call(lo=z) == -1 and b"NULL array pointer (lo, hi" in err()
        assert call(hi=z) == -1 and b"NULL array pointer (lo, hi" in err()
        assert call(C=0, lo=z) == -1 and b"lo, hi" in err()                     # (both required, whatever C)
        assert call(state=z) == -1 and b"NULL array pointer (state)" in err()
        assert call(trial=z) == -1 and b"NULL" in err()
    assert init(x0=z) == -1 and b"NULL" in err()
    assert adv(a=z) == -1 and b"NULL" in err()
    assert adv(kind=2) == -1 and b"row_b" in err()
    for kind in (-1, 3):
        assert adv(kind=kind) == -1 and b"kind" in err()
    for c1 in (0.0, 1.0, float("nan")):
        assert adv(c1=c1) == -1 and b"c1" in err()
    assert adv(gtol=-1.0) == -1 and adv(ftol=float("nan")) == -1 and b"gtol and ftol" in err()
    assert adv(maxiter=0) == -1 and adv(maxback=-1) == -1 and b"maxiter" in err()


def test_python_layer_validates_first():
    torch = pytest.importorskip("torch")
    be = importlib.import_module("code-robchar_amd.backend")
    x = torch.zeros((4, 8), dtype=torch.float64)
    with pytest.raises(ValueError, match="bounds: a pair"):
        be._lbfgs_bounds((x,), x)
    with pytest.raises(ValueError, match="bounds: a pair"):
        be._lbfgs_bounds((np.zeros(8), np.ones(8)), x)
    with pytest.raises(ValueError, match="does not broadcast"):
        be._lbfgs_bounds((torch.zeros(7, dtype=torch.float64), x), x)
    lo, hi = be._lbfgs_bounds((torch.tensor(-1.0), torch.arange(8.0)), x)
    assert tuple(lo.shape) == tuple(hi.shape) == (4, 8) and lo.is_contiguous() and hi.is_contiguous() and lo.dtype == torch.float64
    assert (lo == -1.0).all() and (hi[3] == torch.arange(8.0, dtype=torch.float64)).all()
    full = torch.ones((4, 8), dtype=torch.float64)
    assert be._lbfgs_bounds((full, full), x)[0].data_ptr() == full.data_ptr()   # an expanded tensor is passed through
    nm = importlib.import_module("code-robchar_amd.noise").structured_perturbation(Nspin=5, inspin=0, outspin=4)
    for bad in (1, (1.0,), (0.0, 1.0, 2.0)):
        with pytest.raises(ValueError, match="bounds"):
            nm.optimize_controllers(np.zeros((2, 6)), 8, 1, bounds=bad)
