"""The C entries of the batched L-BFGS (ABI 13) exist, size the state as lbfgs.py lays it out and reject bad arguments before any
HIP call; the Python layer validates before it touches the device - runs without a GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rc_lbfgs_state_len", "rc_lbfgs_init_f64_async", "rc_lbfgs_advance_f64_async", "rc_lbfgs_result_f64_async")


def header_text():
    return open(os.path.join(ROOT, "include", "robchar_hip.h")).read()


def test_header_and_exports():
    assert int(re.search(r"#define\s+RC_ABI_VERSION\s+(\d+)", header_text()).group(1)) >= 13
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    assert lib.rc_version() >= 13
    for symbol in SYMBOLS:
        assert symbol in libmod.EXPORTS and hasattr(lib, symbol)
        assert re.search(r"\b%s\s*\(" % symbol, header_text())
    text = " ".join(header_text().replace("\n *", "\n").split())
    comment = text[text.index("(ABI 13)"):text.index("long long rc_lbfgs_state_len")]
    for phrase in ("lbfgs.py", "accumulated sequentially over the variable index", "[field][C]", "all NaN", "Bounds on the variables are not supported",
                   "noise.moments_from_sums", "5 first value or gradient not finite", "no synchronisation"):
        assert phrase in comment, phrase


def test_state_len_is_the_layout_of_the_definition():
    lib = importlib.import_module("code-robchar_amd._lib").load()
    lbfgs = importlib.import_module("code-robchar_amd.lbfgs")
    for n in range(3, 14):
        for m in range(1, 9):
            assert lib.rc_lbfgs_state_len(7, n, m) == 7 * lbfgs.state_fields(n, m) == 7 * lbfgs.field_offsets(n, m)["len"]
    assert lib.rc_lbfgs_state_len(0, 8, 5) == 0
    for C, n, m in ((4, 2, 5), (4, 14, 5), (4, 8, 0), (4, 8, 9), (-1, 8, 5)):
        assert lib.rc_lbfgs_state_len(C, n, m) < 0, (C, n, m)


def test_argument_validation_without_gpu():
    lib = importlib.import_module("code-robchar_amd._lib").load()
    one = np.ones(4096)
    p, z = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(0)
    err = lambda: lib.rc_last_error()
    init = lambda n, m, C, x0=p, mask=z, state=p, trial=p: lib.rc_lbfgs_init_f64_async(0, z, n, m, C, x0, mask, state, trial)
    adv = lambda n=8, m=5, C=4, kind=1, a=p, b=z, c1=1e-4, gtol=1e-6, ftol=0.0, maxiter=100, maxback=20, state=p, trial=p: \
        lib.rc_lbfgs_advance_f64_async(0, z, n, m, C, kind, 0.0, a, b, c1, gtol, ftol, maxiter, maxback, state, trial)
    res = lambda n=8, m=5, C=4, state=p, outs=(p, z, z, z, z, z): lib.rc_lbfgs_result_f64_async(0, z, n, m, C, state, *outs)
    for call in (init, lambda n, m, C: adv(n, m, C), lambda n, m, C: res(n, m, C)):
        for n in (2, 14, -1):
            assert call(n, 5, 4) == -1 and b"ndim must be 3 .. 13" in err(), n
        for m in (0, 9):
            assert call(8, m, 4) == -1 and b"m must be 1 .. 8" in err(), m
        assert call(8, 5, -1) == -1 and b"non-negative" in err()
        assert call(8, 5, 0) == 0                                              # nothing to do
    assert init(8, 5, 4, state=z) == -1 and b"NULL array pointer (state)" in err()
    assert init(8, 5, 4, x0=z) == -1 and init(8, 5, 4, trial=z) == -1 and b"NULL" in err()
    assert adv(state=z) == -1 and b"NULL array pointer (state)" in err()
    assert adv(a=z) == -1 and adv(trial=z) == -1 and b"NULL" in err()
    assert adv(kind=2) == -1 and b"row_b" in err()
    for kind in (-1, 3):
        assert adv(kind=kind) == -1 and b"kind" in err()
    for c1 in (0.0, 1.0, float("nan")):
        assert adv(c1=c1) == -1 and b"c1" in err()
    assert adv(gtol=-1.0) == -1 and adv(ftol=float("nan")) == -1 and b"gtol and ftol" in err()
    assert adv(maxiter=0) == -1 and adv(maxback=-1) == -1 and b"maxiter" in err()
    assert res(state=z) == -1 and b"NULL array pointer (state)" in err()
    assert res(outs=(z,) * 6) == -1 and b"no output" in err()
    assert res(C=0, outs=(z,) * 6) == -1 and b"no output" in err()              # (checked before the empty batch)


def test_python_layer_validates_first():
    be = importlib.import_module("code-robchar_amd.backend")
    with pytest.raises(ValueError, match="ndim must be"):
        be.lbfgs_state_len(4, 2, 5)
    with pytest.raises(ValueError, match="m must be"):
        be.lbfgs_state_len(4, 8, 9)
    assert be.lbfgs_state_len(4, 8, 5) == 4 * (4 * 8 + 2 * 5 * 8 + 5 + 11)
    with pytest.raises(ValueError, match="x0"):
        be.lbfgs_init(np.zeros((4, 8)))                                        # torch CUDA tensors only
    with pytest.raises(ValueError, match="kind"):
        be.lbfgs_advance(None, None, None, kind="nope")
    with pytest.raises(ValueError, match="trial"):
        be.lbfgs_advance(None, np.zeros((4, 8)), None)
    with pytest.raises(ValueError, match="want"):
        be.lbfgs_result(None, None, want=("y",))
    nm = importlib.import_module("code-robchar_amd.noise").structured_perturbation(Nspin=5, inspin=0, outspin=4)
    with pytest.raises(ValueError, match="objective"):
        nm.optimize_controllers(np.zeros((2, 6)), 8, 1, objective="median")
    with pytest.raises(ValueError, match="alpha"):
        nm.optimize_controllers(np.zeros((2, 6)), 8, 1, objective=("cvar", 0.0))
    with pytest.raises(ValueError, match="unknown L-BFGS parameters"):
        nm.optimize_controllers(np.zeros((2, 6)), 8, 1, bounds=1)
    ring = importlib.import_module("code-robchar_amd.noise").structured_perturbation(Nspin=5, inspin=0, outspin=2, topo="ring")
    with pytest.raises(NotImplementedError):
        ring.optimize_controllers(np.zeros((2, 6)), 8, 1)
