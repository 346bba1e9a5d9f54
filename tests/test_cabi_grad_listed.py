"""The C entry of the listed-sample weighted fidelity gradient (ABI 11) exists and rejects bad arguments before any HIP call; the
Python layer validates before it touches the library - runs without a GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "rc_mc_fidelity_grad_listed_f64_async"


def header_text():
    return open(os.path.join(ROOT, "include", "robchar_hip.h")).read()


def header_constant(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, header_text()).group(1))


def test_header_and_exports():
    assert header_constant("RC_ABI_VERSION") >= 11
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    assert lib.rc_version() >= 11
    assert SYMBOL in libmod.EXPORTS and hasattr(lib, SYMBOL)
    assert re.search(r"\b%s\s*\(" % SYMBOL, header_text())
    # the header states the stream conventions, what an empty slot is, the independence of a sample's bits from its list, and that
    # the full launch is matched to rounding only - with the reason
    text = " ".join(header_text().replace("\n *", "\n").split())
    comment = text[text.index("(ABI 11)"):text.index("int " + SYMBOL)]
    assert "offset + ((c K + k) N + i) 3 + s'" in comment
    assert "offset + (k N + i) 3 + s'" in comment
    assert "outside 0 .. K - 1 is an EMPTY slot" in comment
    assert "not on L, not on the slot, not on what else is listed" in comment
    assert "AGREES TO ROUNDING, NOT BIT FOR BIT" in comment and "votes the sweep count" in comment
    assert "weight_dev [C][L], or NULL" in comment and "no atomics" in comment
    assert "rc_stats_grad_general_tiles" in comment


def test_argument_validation_without_gpu():
    libmod = importlib.import_module("code-robchar_amd._lib")
    lib = libmod.load()
    nmax = header_constant("RC_MAX_NSPIN_GRAD")
    one = np.ones(4096)
    p, z = ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(0)
    err = lambda: lib.rc_last_error()
    # (device, stream, N, in, out, h0d, h0o, ctrl, seed, offset, sigma, sigma_rows, shared, C, K, list, weight, L, fid, grad, sum)
    call = lambda N, a, b, ctrl, sigma, rows, C, K, lst, w, L, fid, grad, tot, shared=0: lib.rc_mc_fidelity_grad_listed_f64_async(
        0, z, N, a, b, z, z, ctrl, 7, 0, sigma, rows, shared, C, K, lst, w, L, fid, grad, tot)
    assert call(1, 0, 0, p, 0.05, z, 1, 1, p, z, 1, p, p, p) == -1 and b"N must be" in err()
    assert call(99, 0, 0, p, 0.05, z, 1, 1, p, z, 1, p, p, p) == -1 and b"N must be" in err()
    assert call(5, 0, 7, p, 0.05, z, 1, 1, p, z, 1, p, p, p) == -1 and b"out of range" in err()
    assert call(5, -1, 2, p, 0.05, z, 1, 1, p, z, 1, p, p, p) == -1 and b"out of range" in err()
    assert call(nmax + 1, 0, nmax, p, 0.05, z, 1, 1, p, z, 1, p, p, p) == -3 and b"N <= %d" % nmax in err()      # RC_ENOSUP
    assert nmax == 12 and b"N <= 12" in err() and b"gradient" in err()
    assert call(5, 0, 4, p, 0.05, z, 1, 1, p, p, 1, z, z, z) == -1 and b"no output" in err() and b"sum_out" in err()
    assert call(5, 0, 4, p, 0.05, z, -1, 1, p, z, 1, p, p, p) == -1 and b"non-negative" in err()
    assert call(5, 0, 4, p, 0.05, z, 1, -1, p, z, 1, p, p, p) == -1 and b"non-negative" in err()
    assert call(5, 0, 4, p, 0.05, z, 1, 1, p, z, -1, p, p, p) == -1 and b"L must be non-negative" in err()
    for shared in (0, 1):
        for bad in (-0.05, float("inf"), float("-inf"), float("nan")):
            assert call(5, 0, 4, p, bad, z, 1, 1, p, z, 1, p, p, p, shared) == -1 and b"sigma" in err(), bad
    assert call(5, 0, 4, z, 0.05, z, 1, 1, p, z, 1, p, p, p) == -1 and b"NULL" in err()                      # controllers
    assert call(5, 0, 4, p, 0.05, z, 1, 1, z, z, 1, p, p, p) == -1 and b"NULL" in err() and b"list" in err()
    assert call(5, 0, 4, p, 0.05, z, 1, 1, z, p, 1, z, z, p) == -1 and b"list" in err()
    assert call(5, 0, 4, z, 0.05, z, 0, 10, z, z, 10, p, z, z) == 0                                          # empty batches
    assert call(5, 0, 4, z, 0.0, z, 10, 0, z, z, 10, z, z, p) == 0
    assert call(5, 0, 4, p, 0.05, z, 10, 10, z, z, 0, z, p, z) == 0                                          # (L = 0: no list needed)
    assert call(5, 0, 4, z, -1.0, p, 10, 0, z, z, 3, z, z, p, 1) == 0                        # (sigma is not read beside sigma_rows)
    assert call(5, 0, 4, p, 0.05, z, 1 << 20, 64, p, z, 1 << 40, p, p, p) == -1 and b"too many tiles" in err()


def test_python_layer_validates_before_the_library():
    be = importlib.import_module("code-robchar_amd.backend")
    noise = importlib.import_module("code-robchar_amd.noise")
    assert be.GRAD_LISTED_OUTPUTS == ("fid", "grad", "sum")
    geo = dict(nspin=5, inspin=0, outspin=4, seed=1)
    ctrl, lst = np.zeros((2, 6)), np.zeros((2, 3), dtype=np.int32)
    with pytest.raises(ValueError):
        be.mc_fidelity_grad_listed(ctrl, 4, lst, nspin=5, inspin=0, outspin=9, seed=1)          # geometry
    with pytest.raises(ValueError, match="want"):
        be.mc_fidelity_grad_listed(ctrl, 4, lst, want=("mean",), **geo)
    with pytest.raises(ValueError, match="want"):
        be.mc_fidelity_grad_listed(ctrl, 4, lst, want=(), **geo)
    with pytest.raises(ValueError, match="controllers"):
        be.mc_fidelity_grad_listed(np.zeros((2, 7)), 4, lst, **geo)
    with pytest.raises(ValueError, match="n_draws"):
        be.mc_fidelity_grad_listed(ctrl, -1, lst, **geo)
    with pytest.raises(ValueError, match="sigma"):
        be.mc_fidelity_grad_listed(ctrl, 4, lst, sigma=np.array([0.1, 0.2, 0.3]), **geo)
    with pytest.raises(ValueError, match="listed"):
        be.mc_fidelity_grad_listed(ctrl, 4, np.zeros((3, 3), dtype=np.int32), **geo)           # rows
    with pytest.raises(ValueError, match="listed"):
        be.mc_fidelity_grad_listed(ctrl, 4, np.zeros(3, dtype=np.int32), **geo)                # one-dimensional
    with pytest.raises(ValueError, match="listed"):
        be.mc_fidelity_grad_listed(ctrl, 4, np.zeros((2, 3)), **geo)                            # a float list
    with pytest.raises(ValueError, match="weights"):
        be.mc_fidelity_grad_listed(ctrl, 4, lst, np.ones((2, 4)), **geo)
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="listed"):
        be.mc_fidelity_grad_listed(ctrl, 4, torch.zeros((2, 3), dtype=torch.int64), **geo)
    with pytest.raises(ValueError, match="weights"):
        be.mc_fidelity_grad_listed(ctrl, 4, lst, torch.ones((2, 3), dtype=torch.float32), **geo)
    ring = noise.structured_perturbation(Nspin=5, inspin=0, outspin=4, noise=0.05, topo="ring")
    with pytest.raises(NotImplementedError, match="chain topology"):
        ring.fidelity_cvar_philox(np.zeros((1, 6)), 4, seed=1, alpha=0.5)
    cplx = noise.structured_perturbation(Nspin=5, inspin=0, outspin=4, noise=0.05)
    cplx.HH[1, 0] += 0.3j
    cplx.HH[0, 1] -= 0.3j
    with pytest.raises(NotImplementedError, match="real static couplings"):
        cplx.fidelity_cvar_philox(np.zeros((1, 6)), 4, seed=1, alpha=0.5)
    chain = noise.structured_perturbation(Nspin=5, inspin=0, outspin=4, noise=0.05)
    for alpha in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            chain.fidelity_cvar_philox(np.zeros((1, 6)), 4, seed=1, alpha=alpha)


def test_example_script_takes_one_objective():
    import sys
    scripts = os.path.join(ROOT, "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    robust_lbfgs = importlib.import_module("robust_lbfgs")
    pytest.importorskip("scipy")
    with pytest.raises(ValueError, match="one of them"):
        robust_lbfgs.run(draws="philox", risk=0.5, cvar=0.1, verbose=False)
    with pytest.raises(ValueError, match="philox"):
        robust_lbfgs.run(draws="set", cvar=0.1, verbose=False)
    with pytest.raises(ValueError, match="alpha"):
        robust_lbfgs.run(draws="philox", cvar=1.5, verbose=False)
