"""The C entries of the bootstrap (ABI 15) exist and reject bad arguments before any HIP call, each with its message; the Python
layers validate before they touch the device - runs without a GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rc_bootstrap_metrics_f64_async", "rc_bootstrap_metrics_f64")


def header_text():
    return open(os.path.join(ROOT, "include", "robchar_hip.h")).read()


def test_header_and_exports():
    assert int(re.search(r"#define\s+RC_ABI_VERSION\s+(\d+)", header_text()).group(1)) >= 15
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    assert lib.rc_version() >= 15
    for symbol in SYMBOLS:
        assert symbol in libmod.EXPORTS and hasattr(lib, symbol)
        assert re.search(r"\b%s\s*\(" % symbol, header_text())
    text = " ".join(header_text().replace("\n *", "\n").split())
    comment = text[text.index("(ABI 15)"):text.index("int rc_bootstrap_metrics_f64_async")]
    for phrase in ("bootstrap.py", "offset + (c B + b) Q + (t >> 2)", "idx = (word * K) >> 32", "No rejection step",
                   "rim1 = 1 - (m + S1 / K)", "A row holding any NaN gives NaN", "rank_lo = floor(a (B - 1))", "[M][C][B]", "[M][4][C]"):
        assert phrase in comment, phrase


def entries(lib):
    z = ctypes.c_void_p(0)

    def asynchronous(fid, C, K, B, offset, thr, nq, lo, hi, route, rep, summ):
        return lib.rc_bootstrap_metrics_f64_async(0, z, fid, C, K, B, 1, offset, thr, nq, lo, hi, route, rep, summ)

    def blocking(fid, C, K, B, offset, thr, nq, lo, hi, route, rep, summ):
        return lib.rc_bootstrap_metrics_f64(0, fid, C, K, B, 1, offset, thr, nq, lo, hi, route, rep, summ)

    return asynchronous, blocking


@pytest.mark.parametrize("which", (0, 1), ids=("async", "blocking"))
def test_argument_validation_without_gpu(which):
    lib = importlib.import_module("code-robchar_amd._lib").load()
    call = entries(lib)[which]
    one = np.ones(64)
    p, z = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(0)
    err = lambda: lib.rc_last_error()
    assert call(p, -1, 8, 4, 0, p, 2, 0, 3, 0, p, p) == -1 and b"C must be non-negative" in err()
    for K in (0, -3):
        assert call(p, 1, K, 4, 0, p, 2, 0, 3, 0, p, p) == -1 and b"K must be positive" in err()
    assert call(p, 1, 2 ** 31, 4, 0, p, 2, 0, 3, 0, p, p) == -1 and b"2^31 - 1" in err()
    for B in (0, -1):
        assert call(p, 1, 8, B, 0, p, 2, 0, 0, 0, p, p) == -1 and b"B must be positive" in err()
    assert call(p, 1, 8, 16385, 0, p, 2, 0, 3, 0, p, p) == -1 and b"B must be at most 16384" in err() and b"row sort" in err()
    for nq in (-1, 9):
        assert call(p, 1, 8, 4, 0, p, nq, 0, 3, 0, p, p) == -1 and b"nq must be in [0, 8]" in err()
    assert call(p, 1, 8, 4, 0, z, 2, 0, 3, 0, p, p) == -1 and b"q_thresholds is NULL" in err()
    for lo, hi in ((-1, 3), (0, 4), (3, 2), (4, 4)):
        assert call(p, 1, 8, 4, 0, p, 2, lo, hi, 0, p, p) == -1 and b"0 <= rank_lo <= rank_hi < B" in err(), (lo, hi)
    for route in (-1, 3):
        assert call(p, 1, 8, 4, 0, p, 2, 0, 3, route, p, p) == -1 and b"route must be 0 (auto), 1 (LDS) or 2 (global)" in err()
    assert call(p, 1, 18433, 4, 0, p, 2, 0, 3, 1, p, p) == -1 and b"route 1 (LDS)" in err() and b"18432" in err()
    assert call(p, 2 ** 31, 8, 4, 0, p, 2, 0, 3, 0, p, p) == -1 and b"too many rows" in err()
    # C B Q = 3 * 4 * 2 = 24 counters: the last offset that fits, and the first that wraps
    assert call(p, 3, 8, 4, 2 ** 64 - 23, p, 2, 0, 3, 0, p, p) == -1 and b"wraps 2^64" in err()
    assert call(z, 3, 8, 4, 2 ** 64 - 24, p, 2, 0, 3, 0, p, p) == -1 and b"NULL fid pointer" in err()      # (the wrap check passed)
    assert call(z, 1, 8, 4, 0, p, 2, 0, 3, 0, p, p) == -1 and b"NULL fid pointer" in err()
    # empty batches: nothing written, no device needed; bad arguments are still refused with C = 0
    assert call(z, 0, 8, 4, 0, p, 2, 0, 3, 0, z, z) == 0 and call(z, 0, 8, 4, 0, z, 0, 0, 3, 2, p, p) == 0
    assert call(z, 0, 0, 4, 0, p, 2, 0, 3, 0, z, z) == -1 and b"K must be positive" in err()
    assert call(p, 1, 8, 4, 0, p, 2, 0, 3, 0, z, z) == 0                                                 # neither output wanted


def test_python_layer_validates_before_the_device():
    be = importlib.import_module("code-robchar_amd.backend")
    boot = importlib.import_module("code-robchar_amd.bootstrap")
    assert be.BOOTSTRAP_OUTPUTS == ("summary", "replicates") and be.BOOTSTRAP_ROUTES == {"auto": 0, "lds": 1, "global": 2}
    fid = np.zeros((2, 8))
    with pytest.raises(ValueError, match="want"):
        be.bootstrap_metrics(fid, 10, 1, want=("summary", "mean"))
    with pytest.raises(ValueError, match="want"):
        be.bootstrap_metrics(fid, 10, 1, want=())
    with pytest.raises(ValueError, match="route"):
        be.bootstrap_metrics(fid, 10, 1, route="fast")
    with pytest.raises(ValueError, match="fid"):
        be.bootstrap_metrics(np.zeros(8), 10, 1)
    with pytest.raises(ValueError, match="K must be positive"):
        be.bootstrap_metrics(np.zeros((2, 0)), 10, 1)
    for n_boot in (0, -1, 16385):
        with pytest.raises(ValueError, match="n_boot"):
            be.bootstrap_metrics(fid, n_boot, 1)
    with pytest.raises(ValueError, match="seed"):
        be.bootstrap_metrics(fid, 10, -1)
    with pytest.raises(ValueError, match="offset"):
        be.bootstrap_metrics(fid, 10, 1, offset=2 ** 64)
    for conf in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="conf"):
            be.bootstrap_metrics(fid, 10, 1, conf=conf)
    assert boot.ranks(400, 0.95) == (9, 390) and boot.ranks(1000, 0.95) == (24, 975) and boot.ranks(1, 0.95) == (0, 0)
    assert boot.ranks(2, 0.5) == (0, 1) and boot.metric_names(2) == ("rim1", "std", "min", "q0", "q1")


def test_ranks_are_numpys_lower_and_higher():
    boot = importlib.import_module("code-robchar_amd.bootstrap")
    rng = np.random.default_rng(2)
    for B in (2, 3, 10, 67, 400, 1000, 1001):
        x = rng.random(B)
        for conf in (0.5, 0.8, 0.9, 0.95, 0.99):
            lo, hi = boot.ranks(B, conf)
            a = (1.0 - conf) / 2.0
            assert np.sort(x)[lo] == np.quantile(x, a, method="lower") and np.sort(x)[hi] == np.quantile(x, 1.0 - a, method="higher"), (B, conf)
