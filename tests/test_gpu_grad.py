"""`backend.mc_fidelity_grad` / `noise_model_base.fidelity_ss_av_grad` on the device against the references and bars of
grad_checks.py.  The worst errors per workload are printed (run with -s)."""
import importlib
import os
import sys

import numpy as np
import pytest

import chain_checks as cc
import grad_checks as gc
from conftest import highfid_workload
from oracle import robchar_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NMAX = 12            # RC_MAX_NSPIN_GRAD (asserted below)
EPS = 2.0 ** -52


def fid_route_bound(ctrl, draws, N, h0_diag=None):
    """`fid_out` is computed from the gradient kernel's own eigensystem (all-fp64 QL with eigenvector rows), not by the
    RC_KERNEL_AUTO route (mixed-precision eigenvalues + adjugate weights): the two are not bit-identical.  What separates
    them is rounding: eigenvalues to a few N eps ||H|| each, multiplied by T in the phase, weights to a few N eps:
    |dF| <= 2 |dphi| <= 64 N eps max(1, T ||H||), ||H|| <= max|d| + 2 max e (64: the 'few' of both routes together)."""
    bars = gc.grad_bars(ctrl, draws, N, h0_diag)
    norm = bars[..., N] / gc.TOL
    T = np.abs(np.nan_to_num(np.asarray(ctrl)[:, N]))[:, None]
    return 64.0 * N * EPS * np.maximum(1.0, T * norm)


def test_header_constant(be):
    assert be.max_nspin_grad() == NMAX >= 12
    text = open(os.path.join(ROOT, "include", "robchar_hip.h")).read()
    assert f"#define RC_MAX_NSPIN_GRAD {NMAX}" in text


@pytest.mark.parametrize("N", range(2, NMAX + 1))
def test_parity_deloc(be, N):
    worst = gc.Worst()
    gc.check_deloc_grad(be, N, worst)
    print("gradient kernel:", worst)


@pytest.mark.parametrize("N", [2, 5, 9, 10, 12])
def test_hard_inputs(be, N):
    forced = os.environ.get("ROBCHAR_GRAD_FORCED_GENERAL") == "1"
    be.grad_general_tiles(reset=True)
    worst = gc.Worst()
    gc.check_hard_inputs(be, N, worst)
    # "never observed" as a tested statement: no tile of the hard inputs needs the sweep-cap fallback (a -DRC_GRAD_FORCE_GENERAL=1
    # variant build, announced with ROBCHAR_GRAD_FORCED_GENERAL=1, sends every tile through it instead)
    tiles = be.grad_general_tiles(reset=True)
    assert (tiles > 0) if forced else (tiles == 0), tiles
    print("gradient kernel:", worst)


@pytest.mark.parametrize("N", [3, 7, 12])
def test_closed_form(be, N):
    worst = gc.Worst()
    gc.check_closed_form_grad(be, N, worst)
    print("gradient kernel:", worst)


@pytest.mark.parametrize("cid", [2, 3, 4, 5])
def test_fullsize(be, cid):
    """Every BASELINE shape at 100 x 10 000, sigma = 0.05.  ALL of fid_out against `mc_fidelity` (bound: fid_route_bound) and
    all of grad_out finite; the gradient itself against the eigh formulas on every controller row, every 5th sample of it
    plus its whole last tile (2.0e5 samples per shape: the reference costs N^3 complex products per sample in NumPy)."""
    import torch
    N, a, b, ctrl, h0 = highfid_workload(cid, C=100)
    C, K = 100, 10000
    dev = be.compute_device()
    gen = torch.Generator(device=dev).manual_seed(100 + cid)
    draws_t = 0.05 * torch.randn((C, K, N, 3), dtype=torch.float64, device=dev, generator=gen)
    res = be.mc_fidelity_grad(torch.from_numpy(ctrl).to(dev), draws_t, N, a, b, h0_diag=h0)
    fid_auto = be.mc_fidelity(torch.from_numpy(ctrl).to(dev), draws_t, N, a, b, h0_diag=h0).cpu().numpy()
    F, G, M = res["fid"].cpu().numpy(), res["grad"].cpu().numpy(), res["mean"].cpu().numpy()
    draws = draws_t.cpu().numpy()
    assert np.isfinite(G).all() and np.isfinite(F).all()
    dfid = np.abs(F - fid_auto)
    bound = fid_route_bound(ctrl, draws, N, h0)
    print(f"config {cid}: fid_out vs mc_fidelity(auto): max |dF| = {dfid.max():.2e} (bound at that sample {bound.flat[dfid.argmax()]:.2e})")
    assert (dfid <= bound).all(), float((dfid / bound).max())
    sel = np.unique(np.concatenate([np.arange(0, K, 5), np.arange((K // 64) * 64 if K % 64 else K - 64, K)]))
    assert C * sel.size >= 2e5
    sub = np.ascontiguousarray(draws[:, sel])
    Fw, Gw = gc.grad_eigh(ctrl, sub, N, a, b, h0)
    med, share = gc.assert_grad_teeth(Gw, ("fullsize", cid))
    cc.compare(F[:, sel], Fw, ("fullsize", cid, "fid"))
    out = gc.compare_grad(G[:, sel], Gw, gc.grad_bars(ctrl, sub, N, h0), ("fullsize", cid))
    rows = np.concatenate([F.mean(axis=1)[:, None], G.mean(axis=1)], axis=1)
    assert np.abs(M - rows).max() <= K * EPS * max(1.0, np.abs(G).max())
    print(f"config {cid} (N = {N}, {a} -> {b}): teeth median {med:.3f} share {share:.3f}; gradient abs {out[0]:.2e}, of the bar {out[1]:.2e}, "
          f"per unit of T {out[2]:.2e}; max |entry| {np.abs(Gw).max():.2f}")


def test_fid_against_auto_kernel_small(be):
    """fid_out against mc_fidelity(kernel="auto") on the parity workloads: inside fid_route_bound (not bit-identical: stated in
    the header and in `backend.mc_fidelity_grad`)."""
    for N in (2, 5, 7, 10, 12):
        rng = np.random.default_rng(800 + N)
        ctrl = cc.deloc_ctrl(rng, 4, N, 0.5)
        draws = 0.05 * rng.standard_normal((4, 192, N, 3))
        for (a, b) in gc.grad_pairs(N):
            got = be.mc_fidelity_grad(ctrl, draws, N, a, b, want=("fid",))["fid"]
            ref = be.mc_fidelity(ctrl, draws, N, a, b, kernel="auto")
            d = np.abs(got - ref)
            assert (d <= fid_route_bound(ctrl, draws, N)).all(), (N, a, b, float(d.max()))


def test_mean_and_shared_set(be):
    gc.check_mean_and_shared(be, 7)
    gc.check_mean_and_shared(be, 11)        # (several QL passes per sample)


def test_torch_entry_on_a_side_stream(be):
    import torch
    rng = np.random.default_rng(5)
    N, C, K = 7, 3, 200
    ctrl = cc.deloc_ctrl(rng, C, N, 0.5)
    ctrl[1] = np.nan
    draws = 0.05 * rng.standard_normal((C, K, N, 3))
    want = be.mc_fidelity_grad(ctrl, draws, N, 0, N - 1)
    dev = be.compute_device()
    side = torch.cuda.Stream(device=dev)
    ct, dt = torch.from_numpy(ctrl).to(dev), torch.from_numpy(draws).to(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        got = be.mc_fidelity_grad(ct, dt, N, 0, N - 1)
    side.synchronize()
    for k in ("fid", "grad", "mean"):
        assert np.array_equal(got[k].cpu().numpy(), want[k], equal_nan=True), k
    assert np.isnan(want["mean"][1]).all() and np.isnan(want["grad"][1]).all() and np.isnan(want["fid"][1]).all()


def test_unsupported_requests(be):
    lib = importlib.import_module("code-robchar_amd._lib")
    noise = importlib.import_module("code-robchar_amd.noise")
    N = NMAX + 1
    with pytest.raises(lib.RobCharHipError, match="N <= 12"):
        be.mc_fidelity_grad(np.zeros((1, N + 1)), np.zeros((1, 4, N, 3)), N, 0, N - 1)
    nm = noise.structured_perturbation(Nspin=5, inspin=0, outspin=4, noise=0.05, topo="ring")
    with pytest.raises(NotImplementedError):
        nm.fidelity_ss_av_grad(np.zeros((1, 6)), np.zeros((4, 5, 3)))
    assert be.grad_general_tiles(reset=True) >= 0


def test_ss_av_grad_against_central_differences_of_ss_av(be, lbfgs_n7):
    """API consistency on the existing path as anchor: central differences (h = 1e-5) of `fidelity_ss_av` itself against
    `fidelity_ss_av_grad` on the shipped N = 7 controllers.  Bound 1.1e-5 = TOL / h for the two fidelities of each difference
    + the truncation floor measured on the reference (4.2e-8, h^2 T^3 scale)."""
    noise = importlib.import_module("code-robchar_amd.noise")
    h = 1e-5
    worst = 0.0
    for pair, (a, b) in (("0-6", (0, 6)), ("0-3", (0, 3))):
        ctrl = np.ascontiguousarray(lbfgs_n7["ctrl_" + pair][:12])
        nm = noise.structured_perturbation(Nspin=7, inspin=a, outspin=b, noise=0.05)
        train, _ = nm.randHset_constructor(train_size=300, test_size=10)
        fav, grad = nm.fidelity_ss_av_grad(ctrl, train)
        assert np.abs(fav - nm.fidelity_ss_av(ctrl, train)).max() < gc.TOL
        fav10, _ = nm.fidelity_ss_av_grad(ctrl, train, reps=10)
        assert np.abs(fav10 - nm.fidelity_ss_av(ctrl, train, reps=10)).max() < gc.TOL
        fd = np.empty_like(grad)
        for l in range(8):
            p, m = ctrl.copy(), ctrl.copy()
            p[:, l] += h
            m[:, l] -= h
            fd[:, l] = (nm.fidelity_ss_av(p, train) - nm.fidelity_ss_av(m, train)) / (2 * h)
        assert np.abs(grad).max() > 1e-2
        worst = max(worst, float(np.abs(fd - grad).max()))
    print(f"fidelity_ss_av_grad vs central differences of fidelity_ss_av: max |diff| = {worst:.2e}")
    assert worst < 1.1e-5


def test_robust_lbfgs_example(be):
    """scripts/robust_lbfgs.py, at most 30 iterations from a shipped 0 -> 6 controller at sigma = 0.05: the objective never
    increases between accepted iterates and ends strictly below the start; the gradient at the final point agrees with central
    differences of `fidelity_ss_av` inside the bound of the test above."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        robust_lbfgs = importlib.import_module("robust_lbfgs")
    finally:
        sys.path.pop(0)
    out = robust_lbfgs.run(row=0, sigma=0.05, maxiter=30, verbose=False)
    vals = [out["start"]] + [t[0] for t in out["trace"]]
    assert len(out["trace"]) >= 1 and len(out["trace"]) <= 30
    assert all(b <= a for a, b in zip(vals, vals[1:])), vals
    assert out["final"] < out["start"]
    nm, train, x = out["model"], out["train_set"], out["x"]
    h = 1e-5
    fd = np.empty(8)
    for l in range(8):
        p, m = x.copy(), x.copy()
        p[l] += h
        m[l] -= h
        fd[l] = -(nm.fidelity_ss_av(p[None], train)[0] - nm.fidelity_ss_av(m[None], train)[0]) / (2 * h)
    print(f"robust_lbfgs: 1 - F {out['start']:.6f} -> {out['final']:.6f} in {len(out['trace'])} iterations, {out['launches']} launches; "
          f"final gradient vs central differences {np.abs(fd - out['final_grad']).max():.2e}")
    assert np.abs(fd - out["final_grad"]).max() < 1.1e-5
