"""`backend.mc_fidelity_sens` and the `noise_model_base` methods built on it, on the device, against the references and bars
of sens_checks.py.  The worst errors per workload are printed (run with -s)."""
import importlib
import os

import numpy as np
import pytest

import chain_checks as cc
import grad_checks as gc
import sens_checks as sc

pytestmark = pytest.mark.gpu
NMAX = 12            # RC_MAX_NSPIN_GRAD
ALL_N = range(2, NMAX + 1)
FORCED = os.environ.get("ROBCHAR_GRAD_FORCED_GENERAL") == "1"      # a -DRC_GRAD_FORCE_GENERAL=1 variant build


@pytest.mark.parametrize("N", ALL_N)
def test_parity_deloc(be, N):
    worst = gc.Worst()
    sc.check_deloc_sens(be, N, worst)
    print("sensitivity kernel:", worst)


@pytest.mark.parametrize("N", ALL_N)
def test_hard_inputs(be, N):
    be.sens_general_tiles(reset=True)
    worst = gc.Worst()
    sc.check_hard_sens(be, N, worst)
    # no tile of the hard inputs needs the sweep-cap fallback (a forced variant build sends every tile through it instead)
    tiles = be.sens_general_tiles(reset=True)
    assert (tiles > 0) if FORCED else (tiles == 0), tiles
    print("sensitivity kernel:", worst)


@pytest.mark.parametrize("N", ALL_N)
def test_closed_form(be, N):
    worst = gc.Worst()
    sc.check_closed_form_sens(be, N, worst)
    print("sensitivity kernel:", worst)


@pytest.mark.parametrize("N", ALL_N)
def test_consistency(be, N):
    d = sc.check_consistency(be, N)
    print(f"sensitivity kernel, N = {N}: mean_out vs row means of sens_out: {d:.2e}")


def test_radial_derivative_against_central_differences(be, lbfgs_n7):
    """`noise_sensitivity` on the shipped N = 7 controllers, K = 1000 fixed z at sigma = 0.05: d fav / d ln(sigma) against a
    central difference (h = 1e-5) of `mc_fidelity`'s row mean with the draws (1 +- h) g.  Bound 1.1e-5 = TOL / h for the two
    fidelities of the difference + the truncation floor, as in test_ss_av_grad_against_central_differences_of_ss_av."""
    noise = importlib.import_module("code-robchar_amd.noise")
    h, sigma, K, N = 1e-5, 0.05, 1000, 7
    worst = big = 0.0
    for pair, (a, b) in (("0-6", (0, 6)), ("0-3", (0, 3))):
        ctrl = np.ascontiguousarray(lbfgs_n7["ctrl_" + pair][:12])
        g = sigma * np.random.default_rng(17).standard_normal((1, K, N, 3))
        nm = noise.structured_perturbation(Nspin=N, inspin=a, outspin=b, noise=sigma)
        res = nm.noise_sensitivity(ctrl, g)
        assert res["fav"].shape == (12,) and res["dfav_dlogsigma"].shape == (12,) and res["direction"].shape == (12, N, 3)
        fp = be.mc_fidelity(ctrl, (1 + h) * g, N, a, b).mean(axis=1)
        fm = be.mc_fidelity(ctrl, (1 - h) * g, N, a, b).mean(axis=1)
        assert np.abs(res["fav"] - be.mc_fidelity(ctrl, g, N, a, b).mean(axis=1)).max() < gc.TOL
        worst = max(worst, float(np.abs((fp - fm) / (2 * h) - res["dfav_dlogsigma"]).max()))
        big = max(big, float(np.abs(res["dfav_dlogsigma"]).max()))
    print(f"noise_sensitivity: d fav / d ln sigma vs central differences: max |diff| = {worst:.2e} (largest slope {big:.2e})")
    assert big > 1e-3
    assert worst < 1.1e-5


def test_model_methods(be, lbfgs_n7):
    """nominal_sensitivity: one zero draw, imaginary column exactly 0, equal to the bias gradient in the site column;
    static imaginary couplings: the radial derivative is taken over the draws alone."""
    noise = importlib.import_module("code-robchar_amd.noise")
    N, a, b = 7, 0, 6
    ctrl = np.ascontiguousarray(lbfgs_n7["ctrl_0-6"][:6])
    nm = noise.structured_perturbation(Nspin=N, inspin=a, outspin=b, noise=0.05)
    nom = nm.nominal_sensitivity(ctrl)
    assert nom.shape == (6, N, 3) and (nom[..., 2] == 0.0).all() and (nom[:, 0, 1] == 0.0).all()
    zero = np.zeros((1, 1, N, 3))
    _, Sw = sc.sens_eigh(ctrl, zero, N, a, b)
    sc.compare_sens(nom, Sw[:, 0], sc.sens_bars(ctrl, zero, N)[0][:, 0], "nominal")
    assert np.abs(nom[..., 1]).max() > 1e-2
    # a static imaginary part on the couplings
    imag = 0.3 * np.cos(np.arange(1, N))
    hop = np.arange(1, N)
    nm.HH[hop, hop - 1] += 1j * imag
    nm.HH[hop - 1, hop] -= 1j * imag
    g = 0.05 * np.random.default_rng(3).standard_normal((1, 200, N, 3))
    res = nm.fidelity_sens_from_draws(ctrl, g)
    shifted = g.copy()
    shifted[..., 1:, 2] += imag
    Fw, Sw = sc.sens_eigh(ctrl, shifted, N, a, b)
    bars, rbars = sc.sens_bars(ctrl, shifted, N)
    sc.compare_sens(res["sens"], Sw, bars, "static imaginary couplings")
    want = sc.mean_of(Fw, g, Sw)                       # rho over the draws, not over draws + static part
    sc.compare_sens(res["mean"], want, sc.mean_bars(bars, rbars), "static imaginary couplings, mean")
    assert np.abs(want[:, 1] - sc.mean_of(Fw, shifted, Sw)[:, 1]).max() > 1e-3      # the correction matters


def test_torch_entry_on_a_side_stream(be):
    import torch
    rng = np.random.default_rng(5)
    N, C, K = 11, 3, 200
    ctrl = cc.deloc_ctrl(rng, C, N, 0.5)
    ctrl[1] = np.nan
    draws = 0.05 * rng.standard_normal((C, K, N, 3))
    want = be.mc_fidelity_sens(ctrl, draws, N, 0, N - 1)
    dev = be.compute_device()
    side = torch.cuda.Stream(device=dev)
    ct, dt = torch.from_numpy(ctrl).to(dev), torch.from_numpy(draws).to(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        got = be.mc_fidelity_sens(ct, dt, N, 0, N - 1)
    side.synchronize()
    for k in ("fid", "sens", "mean"):
        assert got[k].device == dt.device
        assert np.array_equal(got[k].cpu().numpy(), want[k], equal_nan=True), k
    assert np.isnan(want["mean"][1]).all() and np.isnan(want["sens"][1]).all() and np.isnan(want["fid"][1]).all()


def test_unsupported_requests(be):
    lib = importlib.import_module("code-robchar_amd._lib")
    N = NMAX + 1
    with pytest.raises(lib.RobCharHipError, match="N <= 12"):
        be.mc_fidelity_sens(np.zeros((1, N + 1)), np.zeros((1, 4, N, 3)), N, 0, N - 1)
    assert be.sens_general_tiles(reset=True) >= 0
