"""`backend.tail_select` (tail_select_kernel behind rc_tail_select_f64_async) on the device: every check of tail_select_checks.py,
`noise.tail_weights` on a GPU tensor against the torch sort it replaces, `fidelity_cvar_philox` against the same call with that
torch route patched in, and the CVaR client without Python.  Every comparison is exact."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import grad_checks as gc
import tail_select_checks as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_select(be):
    def select(F, alpha):
        res = be.tail_select(F, alpha)                       # NumPy in: uploaded, NumPy out
        return res["list"], res["weight"], res["var"]
    return select


@pytest.mark.parametrize("K", tc.RANDOM_K)
@pytest.mark.parametrize("which", range(6), ids=("m=1", "0.03", "0.1", "0.5", "0.95", "1.0"))
def test_random_rows(be, K, which):
    tc.check_random(device_select(be), ks=(K,), which=(which,))


@pytest.mark.parametrize("check", [c for c in tc.ALL_CHECKS if c is not tc.check_random], ids=lambda c: c.__name__)
def test_checks(be, check):
    check(device_select(be))


def test_optional_outputs_and_torch_in_torch_out(be):
    import torch
    F, exp = tc.case(("random", 1000), tc.random_rows(1000), 0.1)
    dev = be.compute_device()
    Ft = torch.from_numpy(F.copy()).to(dev)
    res = be.tail_select(Ft, 0.1, want=("list",))
    assert set(res) == {"list"} and res["list"].device == Ft.device and res["list"].dtype == torch.int32
    assert np.array_equal(res["list"].cpu().numpy(), exp[0])
    res = be.tail_select(Ft, 0.1, want=("var",))
    assert set(res) == {"list", "var"} and np.array_equal(res["var"].cpu().numpy(), exp[2], equal_nan=True)
    res = be.tail_select(Ft.t().contiguous().t(), 0.1)       # a non-contiguous view is made contiguous
    assert all(np.array_equal(res[k].cpu().numpy(), e, equal_nan=True) for k, e in zip(("list", "weight", "var"), exp))


def test_side_stream_behind_an_unwaited_fidelity_launch(be):
    """the selection enqueued on a non-default stream directly behind the fidelity launch that writes its input, nothing waited
    for in between: the result of selecting from the finished table"""
    import torch
    N, K, C = 5, 10_000, 8
    ctrl = torch.from_numpy(gc.philox_ctrl(N, C=C, nan_row=None)).to(be.compute_device())
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fid = be.mc_fidelity_philox(ctrl, K, N, 0, N - 1, seed=11, sigma=0.1)
        res = be.tail_select(fid, 0.1)
    side.synchronize()
    F = fid.cpu().numpy()
    exp = tc.expected(F, 0.1)
    for k, e in zip(("list", "weight", "var"), exp):
        assert np.array_equal(res[k].cpu().numpy(), e, equal_nan=True), k
    again = be.tail_select(fid, 0.1)
    assert all(torch.equal(again[k], res[k]) for k in ("list", "weight")) and again["var"].cpu().numpy().tobytes() == res["var"].cpu().numpy().tobytes()


@pytest.mark.parametrize("K, alpha", [(100, 0.1), (1000, 0.03), (10_000, 0.1), (16_385, 0.5), (257, 1.0)])
def test_tail_weights_on_a_gpu_tensor_equals_the_torch_route(be, K, alpha):
    import torch
    noise = importlib.import_module("code-robchar_amd.noise")
    F = np.floor(64.0 * np.random.default_rng(K).random((6, K))) / 64.0          # ties across the threshold too
    F[4, K // 3] = np.nan
    Ft = torch.from_numpy(F).to(be.compute_device())
    new, old, ref = noise.tail_weights(Ft, alpha), noise._tail_weights_torch(Ft, alpha), noise.tail_weights(F, alpha)
    for a, b, c in zip(new, old, ref):
        assert a.device == b.device and a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()) and np.array_equal(a.cpu().numpy(), c)


@pytest.mark.parametrize("N", [5, 7])
@pytest.mark.parametrize("alpha", [0.1, 1.0])
def test_cvar_keeps_its_bits(be, N, alpha, monkeypatch):
    """fidelity_cvar_philox through the selection kernel against the same call through the torch sort + gather + max: per-controller
    draws, shared draws, and one sigma per row including a sigma = 0 row (K identical fidelities: the tie group is the whole row)"""
    noise = importlib.import_module("code-robchar_amd.noise")
    K = 256
    ctrl = gc.philox_ctrl(N, C=3)
    model = noise.structured_perturbation(Nspin=N, inspin=0, outspin=N - 1, noise=0.1)
    modes = (dict(), dict(shared=True), dict(sigma=np.array([0.1, 0.2, 0.0])), dict(sigma=np.array([0.0, 0.05, 0.2]), shared=True))
    new = [model.fidelity_cvar_philox(ctrl, K, 77, alpha, offset=5, **mode) for mode in modes]
    monkeypatch.setattr(noise, "_tail_select_routed", lambda K: False)
    old = [model.fidelity_cvar_philox(ctrl, K, 77, alpha, offset=5, **mode) for mode in modes]
    for a, b, mode in zip(new, old, modes):
        assert np.isfinite(a["cvar"]).sum() >= 2, mode
        for k in ("cvar", "grad_cvar", "var"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (mode, k)


def test_cvar_client_without_python(be, tmp_path):
    """tests/host/hip_client_cvar.cpp: fidelities -> selection -> listed gradient through the three enqueue-only C entries on the
    program's own stream; CVaR, gradient and value at risk equal fidelity_cvar_philox's doubles"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    noise = importlib.import_module("code-robchar_amd.noise")
    libdir = os.path.join(ROOT, "code-robchar_amd", "csrc")
    exe = str(tmp_path / "hip_client_cvar")
    subprocess.run([hipcc, "-O1", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "hip_client_cvar.cpp"), "-L", libdir, "-lrobchar_hip", f"-Wl,-rpath,{libdir}"], check=True)
    N, C, K, seed, sigma, alpha = 5, 2, 256, 123, 0.1, 0.1
    ctrl = gc.philox_ctrl(N, C=C, nan_row=None, neg_row=None)
    r = subprocess.run([exe, str(N), "0", str(N - 1), str(C), str(K), str(seed), repr(sigma), repr(alpha)],
                       input=" ".join(repr(float(v)) for v in ctrl.ravel()) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-1000:])
    rows = np.array([float(v) for v in r.stdout.split()]).reshape(C, N + 3)
    want = noise.structured_perturbation(Nspin=N, inspin=0, outspin=N - 1, noise=sigma).fidelity_cvar_philox(ctrl, K, seed, alpha)
    assert np.array_equal(rows[:, 0], want["cvar"]) and np.array_equal(rows[:, 1:N + 2], want["grad_cvar"])
    assert np.array_equal(rows[:, N + 2], want["var"])
