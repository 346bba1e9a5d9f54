"""The C entries of the tail selection (ABI 12) exist, reject bad arguments before any HIP call and compute the tail length with the
bits of `noise.tail_weights`; the Python layer validates before it touches the device; the CVaR client without Python compiles and
links - runs without a GPU."""
import ctypes
import importlib
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rc_tail_select_len", "rc_tail_select_f64_async")


def header_text():
    return open(os.path.join(ROOT, "include", "robchar_hip.h")).read()


def header_constant(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, header_text()).group(1))


def test_header_and_exports():
    assert header_constant("RC_ABI_VERSION") >= 12
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    assert lib.rc_version() >= 12
    for symbol in SYMBOLS:
        assert symbol in libmod.EXPORTS and hasattr(lib, symbol)
        assert re.search(r"\b%s\s*\(" % symbol, header_text())
    # the header states the order, the tie rule, the -0.0 rule and the NaN rule, and cites the definition
    text = " ".join(header_text().replace("\n *", "\n").split())
    comment = text[text.index("(ABI 12)"):text.index("long long rc_tail_select_len")]
    assert "noise.tail_weights" in comment
    assert "the indices of the m smallest values of the row under the order (value, index)" in comment
    assert "ties go to the lower index, as in NumPy's stable sort" in comment and "ascending index order" in comment
    assert "w_last on the slot that holds the m-th smallest element in that order" in comment
    assert "the selected tied element with the highest index" in comment
    assert "-0.0 and +0.0 are equal" in comment and "the index breaks the tie" in comment
    assert "A row containing any NaN gives list = -1, weight = 0.0, var = NaN" in comment
    assert "ak = alpha * K" in comment and "w_last = (ak - (m - 1)) / ak" in comment
    listed = text[text.index("(ABI 11)"):text.index("int rc_mc_fidelity_grad_listed_f64_async")]
    assert "rc_tail_select_f64_async" in listed and "noise.tail_weights" in listed


def test_argument_validation_without_gpu():
    lib = importlib.import_module("code-robchar_amd._lib").load()
    one = np.ones(64)
    p, z = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(0)
    err = lambda: lib.rc_last_error()
    call = lambda fid, C, K, alpha, lst, w, var: lib.rc_tail_select_f64_async(0, z, fid, C, K, alpha, lst, w, var)
    for alpha in (0.0, -0.1, 1.0000001, float("nan"), float("inf"), float("-inf")):
        assert call(p, 1, 8, alpha, p, p, p) == -1 and b"alpha must be in (0, 1]" in err(), alpha
        assert call(z, 0, 0, alpha, z, z, z) == -1 and b"alpha" in err(), alpha               # (checked before the empty batch)
        assert lib.rc_tail_select_len(8, alpha) == -1
    assert call(p, -1, 8, 0.5, p, p, p) == -1 and b"non-negative" in err()
    assert call(p, 1, -8, 0.5, p, p, p) == -1 and b"non-negative" in err()
    assert call(p, 1, 2 ** 31, 0.5, p, p, p) == -1 and b"2^31 - 1" in err()
    assert call(z, 1, 8, 0.5, p, p, p) == -1 and b"NULL" in err() and b"fid" in err()
    assert call(p, 1, 8, 0.5, z, p, p) == -1 and b"NULL" in err() and b"list" in err()
    assert call(p, 2 ** 31, 8, 0.5, p, p, p) == -1 and b"too many rows" in err()
    assert call(z, 0, 8, 0.5, z, z, z) == 0 and call(z, 8, 0, 1.0, z, z, z) == 0             # empty batches: nothing written
    assert call(p, 0, 8, 0.5, p, z, z) == 0
    assert lib.rc_tail_select_len(-1, 0.5) == -1 and lib.rc_tail_select_len(2 ** 31, 0.5) == -1
    assert lib.rc_tail_select_len(0, 0.5) == 0 and lib.rc_tail_select_len(2 ** 31 - 1, 1.0) == 2 ** 31 - 1


def test_tail_length_has_the_bits_of_the_definition():
    lib = importlib.import_module("code-robchar_amd._lib").load()
    rng = np.random.default_rng(12)
    pairs = [(int(K), float(a)) for K, a in zip(rng.integers(1, 200_000, 200), rng.uniform(1e-6, 1.0, 200))]
    for K in (1, 7, 100, 256, 1000, 10_000, 100_003, 2 ** 31 - 1):
        for j in sorted({v for v in (1, 2, K // 10, K // 3, K - 1, K) if 1 <= v <= K}):
            a = j / K                                                # alpha K within an ulp of the integer j, on either side
            pairs += [(K, a), (K, float(np.nextafter(a, 0.0))), (K, min(1.0, float(np.nextafter(a, 2.0))))]
        pairs += [(K, 0.03), (K, 0.1), (K, 0.95), (K, 1.0), (K, 0.5 / K)]
    near = 0
    for K, alpha in pairs:
        want = min(K, int(math.ceil(alpha * K)))
        near += alpha * K != round(alpha * K) and abs(alpha * K - round(alpha * K)) <= 2 * np.spacing(alpha * K)
        assert lib.rc_tail_select_len(K, alpha) == want, (K, alpha)
    assert len(pairs) >= 300 and near >= 10


def test_python_layer_validates_before_the_device():
    be = importlib.import_module("code-robchar_amd.backend")
    assert be.TAIL_SELECT_OUTPUTS == ("list", "weight", "var")
    fid = np.zeros((2, 8))
    for alpha in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            be.tail_select(fid, alpha)
    with pytest.raises(ValueError, match="want"):
        be.tail_select(fid, 0.5, want=("list", "mean"))
    with pytest.raises(ValueError, match="fid"):
        be.tail_select(np.zeros(8), 0.5)
    with pytest.raises(ValueError, match="K must be positive"):
        be.tail_select(np.zeros((2, 0)), 0.5)
    torch = pytest.importorskip("torch")
    noise = importlib.import_module("code-robchar_amd.noise")
    F = np.random.default_rng(3).random((3, 50))
    F[1, 4] = np.nan
    want = noise.tail_weights(F, 0.1)                                # a CPU tensor keeps torch's sort: same arrays
    for got in (noise.tail_weights(torch.from_numpy(F), 0.1), noise._tail_weights_torch(torch.from_numpy(F), 0.1)):
        assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])


def test_cvar_client_compiles_and_links(tmp_path):
    """`tests/host/hip_client_cvar.cpp` (fidelities -> selection -> listed gradient on its own stream, no Python) builds with hipcc
    against the header and the library; it is RUN by tests/test_gpu_tail_select.py on the GPU."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    libdir = os.path.join(ROOT, "code-robchar_amd", "csrc")
    r = subprocess.run([hipcc, "-O1", "--offload-arch=gfx950", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o",
                        str(tmp_path / "hip_client_cvar"), os.path.join(ROOT, "tests", "host", "hip_client_cvar.cpp"), "-L", libdir,
                        "-lrobchar_hip", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
