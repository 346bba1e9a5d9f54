"""The C entry of the variance indices (ABI 20) exists with its constants, every rule of its contract is refused before any HIP call
with its code and message, and the Python layer validates before it touches the device - runs without a GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "rc_mc_fidelity_pickfreeze_philox_f64_async"
EINVAL, ENOSUP, OK = -1, -3, 0


def header_text():
    return open(os.path.join(ROOT, "include", "robchar_hip.h")).read()


def test_header_and_exports():
    version = int(re.search(r"#define\s+RC_ABI_VERSION\s+(\d+)", header_text()).group(1))
    assert version >= 20
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    assert lib.rc_version() == version
    assert SYMBOL in libmod.EXPORTS and hasattr(lib, SYMBOL) and re.search(r"\b%s\s*\(" % SYMBOL, header_text())
    assert re.search(r"#define\s+RC_MAX_NSPIN_PICKFREEZE\s+13\b", header_text())
    assert re.search(r"#define\s+RC_PICKFREEZE_MAX_GROUPS\s+64\b", header_text())
    be = importlib.import_module("code-robchar_amd.backend")
    vi = importlib.import_module("code-robchar_amd.variance_indices")
    assert be.MAX_NSPIN_PICKFREEZE == vi.MAX_NSPIN == 13 and vi.MAX_GROUPS == 64


def test_contract_is_refused_without_gpu():
    lib = importlib.import_module("code-robchar_amd._lib").load()
    one = np.ones(4096)
    groups = np.array([0b001001, 0b010000, 0b100000], dtype=np.uint64)
    a, z, gp = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(0), ctypes.c_void_p(groups.ctypes.data)
    err = lambda: lib.rc_last_error()

    def call(N=2, kernel=0, i=0, o=1, ctrl=a, off_a=0, off_b=2 * 128 * 6, sigma=0.05, rows=z, g=gp, G=3, C=2, K=128, fid=a, mean=a):
        return lib.rc_mc_fidelity_pickfreeze_philox_f64_async(0, z, kernel, N, i, o, z, z, ctrl, 7, off_a, off_b, sigma, rows, g, G, C, K,
                                                              fid, mean)

    assert call(N=1) == EINVAL and b"N must be" in err()
    assert call(N=33) == EINVAL and b"N must be" in err()
    assert call(o=2) == EINVAL and b"out of range" in err()
    for N in (14, 16, 32):
        assert call(N=N, o=N - 1) == ENOSUP and b"pick-freeze kernel: N <= 13" in err()
    for kernel in (1, 2, 4, 5):
        assert call(kernel=kernel) == ENOSUP and b"eigenvalue-only chain kernels only" in err()
    for G in (-1, 65):
        assert call(G=G) == EINVAL and b"G must be in [0, 64]" in err()
    assert call(g=z) == EINVAL and b"groups" in err()
    groups[1] = 1 << 6                                   # N = 2: coordinates 0 .. 5
    assert call() == EINVAL and b"group 1: a mask bit at or above 3 N = 6" in err()
    groups[1] = 0b110                                   # the dropped coordinates are allowed
    assert call(sigma=-1.0) == EINVAL and b"sigma must be finite and non-negative" in err()
    assert call(sigma=float("nan")) == EINVAL and b"sigma" in err()
    n = 2 * 128 * 6
    for off_a, off_b in ((0, n - 1), (n - 1, 0), (5, 5), (2 ** 64 - 10, n - 11), (n - 11, 2 ** 64 - 10)):
        assert call(off_a=off_a, off_b=off_b) == EINVAL and b"overlap" in err(), (off_a, off_b)
    assert call(off_a=5, off_b=5, C=0) == OK             # empty ranges do not overlap
    assert call(fid=z, mean=z) == EINVAL and b"no output requested" in err()
    assert call(ctrl=z) == EINVAL and b"NULL array pointer (controllers)" in err()
    assert call(C=2 ** 31, K=64, off_b=2 ** 31 * 64 * 6) == EINVAL and b"too many tiles" in err()
    assert call(C=-1) == EINVAL and call(K=-1) == EINVAL and b"non-negative" in err()
    # empty batches: RC_OK behind the contract, nothing written, pointers not looked at
    assert call(C=0, ctrl=z) == OK and call(K=0, ctrl=z) == OK and call(G=0, g=z, C=0) == OK
    assert call(C=0, G=65) == EINVAL and call(K=0, fid=z, mean=z) == EINVAL
    assert np.all(one == 1.0)


def test_python_layer_validates_before_the_device():
    be = importlib.import_module("code-robchar_amd.backend")
    ctrl = np.zeros((2, 4))
    with pytest.raises(ValueError, match="at or above 3 N"):
        be.mc_fidelity_pickfreeze_philox(ctrl, 64, 3, 0, 2, 1, [1 << 9])
    with pytest.raises(ValueError, match="at most 64"):
        be.mc_fidelity_pickfreeze_philox(ctrl, 64, 3, 0, 2, 1, [1] * 65)
    with pytest.raises(ValueError, match="overlap"):
        be.mc_fidelity_pickfreeze_philox(ctrl, 64, 3, 0, 2, 1, [1], offset=0, offset_b=2 * 64 * 9 - 1)
    with pytest.raises(ValueError, match="want"):
        be.mc_fidelity_pickfreeze_philox(ctrl, 64, 3, 0, 2, 1, [1], want=("sens",))
    with pytest.raises(ValueError, match="expected"):
        be.mc_fidelity_pickfreeze_philox(np.zeros((2, 5)), 64, 3, 0, 2, 1, [1])
    with pytest.raises(NotImplementedError):
        be.mc_fidelity_pickfreeze_philox(np.zeros((2, 15)), 64, 14, 0, 13, 1, [1])
    with pytest.raises(NotImplementedError):
        be.mc_fidelity_pickfreeze_philox(ctrl, 64, 3, 0, 2, 1, [1], kernel="jacobi")
    assert be.pickfreeze_supported(13) and not be.pickfreeze_supported(14) and not be.pickfreeze_supported(5, ring=True)
    assert not be.pickfreeze_supported(5, kernel="jacobi")
    nm = importlib.import_module("code-robchar_amd.noise")
    model = nm.structured_perturbation(Nspin=4, inspin=0, outspin=3, topo="ring")
    with pytest.raises(NotImplementedError):
        model.noise_variance_indices_philox(np.zeros((1, 5)), 64, 1)
    with pytest.raises(NotImplementedError):
        nm.structured_perturbation(Nspin=14, inspin=0, outspin=13).noise_variance_indices_philox(np.zeros((1, 15)), 64, 1)
    with pytest.raises(ValueError, match="groups"):
        nm.structured_perturbation(Nspin=4, inspin=0, outspin=3).noise_variance_indices_philox(np.zeros((1, 5)), 64, 1, groups="sobol")
