"""`backend.mc_fidelity_sens_philox` - the noise sensitivity with the counter-based draws generated inside the kernel - on the
device: BIT-IDENTICAL to the two-kernel route (`philox_normal` + `mc_fidelity_sens`) in all three outputs, at every pass
schedule (one pass: N <= 9; 3 / 4 / 6 passes: N = 10 / 11 / 12), both pair parities of the first element, tile boundaries
and per-row sigma; against an independent reference (host-regenerated draws, eigh); and through the product surface
`MCDataSim.get_sensitivity_dict`.  Shapes are the smallest that reach those paths: C = 3 rows (one NaN), K = 130 = tiles of
64, 64 and 2 samples.  ROBCHAR_GRAD_FORCED_GENERAL=1 announces a -DRC_GRAD_FORCE_GENERAL=1 variant build (scripts/build_variant.sh),
in which every tile takes the sweep-cap fallback: run the bit-identity test for N = 7 and 10 on it."""
import importlib
import json
import os

import numpy as np
import pytest

import chain_checks as cc
import grad_checks as gc
import sens_checks as sc
from conftest import load_json
from oracle import philox_host

pytestmark = pytest.mark.gpu
FORCED = os.environ.get("ROBCHAR_GRAD_FORCED_GENERAL") == "1"      # a -DRC_GRAD_FORCE_GENERAL=1 variant build
SIGMA = 0.05
SEED = 0x5EED0009
IDENTITY_N = (2, 3, 7, 9, 10, 11, 12)
KEYS = ("fid", "sens", "mean")


def ctrl_rows(N, C=3, nan_row=1):
    """delocalised rows (the sensitivities have teeth there), one of them NaN"""
    ctrl = cc.deloc_ctrl(np.random.default_rng(9100 + N), C, N, 0.5)
    if nan_row is not None:
        ctrl[nan_row, N // 2] = np.nan
    return ctrl


def fused(be, ctrl, K, N, a, b, offset=0, sigma=SIGMA, seed=SEED, want=KEYS):
    import torch
    dev = be.compute_device()
    if not isinstance(sigma, float):
        sigma = torch.from_numpy(np.asarray(sigma, dtype=np.float64)).to(dev)
    res = be.mc_fidelity_sens_philox(torch.from_numpy(ctrl).to(dev), K, N, a, b, seed, offset=offset, sigma=sigma, want=want)
    return {k: v.cpu().numpy() for k, v in res.items()}


def two_kernels(be, ctrl, K, N, a, b, offset=0, sigma=SIGMA, seed=SEED):
    draws = be.philox_normal((ctrl.shape[0], K, N, 3), seed, scale=sigma, offset=offset)
    return be.mc_fidelity_sens(ctrl, draws, N, a, b)


def assert_same_bits(got, want, what):
    for k in want:
        assert got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k], equal_nan=True), (
            what, k, "differs in", int((~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k])))).sum()), "entries, max |diff|",
            float(np.nanmax(np.abs(got[k] - want[k]))))


def check_identity(be, N, K=130, offsets=(0, 7)):
    ctrl = ctrl_rows(N)
    for (a, b) in gc.grad_pairs(N):
        for offset in offsets:
            want = two_kernels(be, ctrl, K, N, a, b, offset)
            sc.assert_sens_teeth(want["sens"], ("two-kernel route", N, a, b, offset))
            assert np.isnan(want["fid"][1]).all() and np.isnan(want["sens"][1]).all() and np.isnan(want["mean"][1]).all()
            assert_same_bits(fused(be, ctrl, K, N, a, b, offset), want, (N, a, b, offset, K))


@pytest.mark.parametrize("N", IDENTITY_N)
def test_bit_identity_with_the_two_kernel_route(be, N):
    """(a forced variant build: both routes send every tile through the sweep-cap fallback - here the draws element by element
    from philox_element, the textbook QL in LDS - and must still agree bit for bit; the counter counts instead of staying 0)"""
    be.sens_general_tiles(reset=True)
    check_identity(be, N)
    tiles = be.sens_general_tiles(reset=True)
    assert (tiles > 0) if FORCED else (tiles == 0), tiles


@pytest.mark.parametrize("K", (1, 64, 65))
def test_tile_boundaries(be, K):
    check_identity(be, 7, K=K)


@pytest.mark.parametrize("N", (7, 10))
def test_per_row_sigma(be, N):
    """sigma_rows = (0, 0.02, 0.1): every row equals a scalar-sigma call of the two-kernel route at that row's offset; in the
    sigma = 0 row rho is exactly 0.0 and all K samples are the same nominal sensitivity."""
    K, a, b = 130, 0, N - 1
    rows = np.array([0.0, 0.02, 0.1])
    ctrl = ctrl_rows(N, nan_row=None)
    for offset in (0, 7):
        got = fused(be, ctrl, K, N, a, b, offset, sigma=rows)
        for c, sigma in enumerate(rows):
            want = two_kernels(be, ctrl[c:c + 1], K, N, a, b, offset + c * K * N * 3, sigma=float(sigma))
            assert_same_bits({k: got[k][c:c + 1] for k in KEYS}, want, (N, offset, "row", c))
        sc.assert_sens_teeth(got["sens"], ("per-row sigma", N))
        assert got["mean"][0, 1] == 0.0 and not np.signbit(got["mean"][0, 1])
        assert (got["sens"][0] == got["sens"][0, :1]).all() and (got["fid"][0] == got["fid"][0, 0]).all()
        assert np.abs(got["mean"][1:, 1]).min() > 0.0


@pytest.mark.parametrize("N", (5, 10))
def test_independent_reference(be, N):
    """draws regenerated on the host (oracle/philox_host.py), reference sens_checks.sens_eigh, bars of sens_checks"""
    C, K, offset = 3, 130, 7
    ctrl = ctrl_rows(N)
    draws = philox_host.philox_normal(SEED, offset, C * K * N * 3, SIGMA).reshape(C, K, N, 3)
    for (a, b) in ((0, N - 1), (min(1, N - 1), N // 2)):
        Fw, Sw = sc.sens_eigh(ctrl, draws, N, a, b)
        sc.assert_sens_teeth(Sw, ("independent reference", N, a, b))
        got = fused(be, ctrl, K, N, a, b, offset)
        bars, rbars = sc.sens_bars(ctrl, draws, N)
        cc.compare(got["fid"], Fw, ("fused", N, a, b, "fid"))
        e = sc.compare_sens(got["sens"], Sw, bars, ("fused", N, a, b, "sens"))
        m = sc.compare_sens(got["mean"], sc.mean_of(Fw, draws, Sw), sc.mean_bars(bars, rbars), ("fused", N, a, b, "mean"))
        print(f"fused sensitivity kernel, N = {N}, {a} -> {b}: worst |sens error| {e[0]:.2e} ({e[1]:.2e} of its bar), "
              f"mean {m[0]:.2e} ({m[1]:.2e})")


def test_output_subsets_and_side_stream(be):
    import torch
    N, K, a, b = 11, 130, 0, 10
    ctrl = ctrl_rows(N)
    full = fused(be, ctrl, K, N, a, b, 7)
    for sub in (("mean",), ("sens",), ("fid",), ("fid", "mean")):
        only = fused(be, ctrl, K, N, a, b, 7, want=sub)
        assert set(only) == set(sub)
        assert_same_bits(only, {k: full[k] for k in sub}, sub)
    dev = be.compute_device()
    side = torch.cuda.Stream(device=dev)
    ct = torch.from_numpy(ctrl).to(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        got = be.mc_fidelity_sens_philox(ct, K, N, a, b, SEED, offset=7, sigma=SIGMA)
    side.synchronize()
    assert all(got[k].device == ct.device for k in KEYS)
    assert_same_bits({k: v.cpu().numpy() for k, v in got.items()}, full, "side stream")


def test_unsupported_and_rejected(be):
    import torch
    lib = importlib.import_module("code-robchar_amd._lib")
    dev = be.compute_device()
    with pytest.raises(lib.RobCharHipError, match="N <= 12"):
        be.mc_fidelity_sens_philox(torch.zeros((1, 14), dtype=torch.float64, device=dev), 4, 13, 0, 12, seed=1)
    with pytest.raises(lib.RobCharHipError, match="sigma"):
        be.mc_fidelity_sens_philox(torch.zeros((1, 6), dtype=torch.float64, device=dev), 4, 5, 0, 4, seed=1, sigma=-0.1)


def _write_le(g, name):
    os.makedirs(f"experiments/{name}", exist_ok=True)
    base = f"experiments/{name}/ppo_spin_{g['Nspin']}_{g['inspin']}-{g['outspin']}_c_{g['numcontrollers']}"
    json.dump(g["le"], open(base + ".le", "w"))


def test_product_path(be, workdir):
    """`MCDataSim.get_sensitivity_dict` on the shipped N = 5 controllers, three levels, samples = 128: bit for bit the level-by-
    level `noise_sensitivity` on `philox_normal` draws; d fav / d ln sigma against a central difference in ln sigma of fav on
    the same unit normals (step h = 1e-5 and bound 1.1e-5 = TOL / h + truncation floor, as the radial-derivative test of
    tests/test_gpu_sens.py)."""
    mcmod = importlib.import_module("code-robchar_amd.mc_data_sim")
    noise = importlib.import_module("code-robchar_amd.noise")
    g = load_json("mcsim_run.json")
    _write_le(g, "sens")
    N, a, b, C, K, seed, tn = g["Nspin"], g["inspin"], g["outspin"], g["numcontrollers"], 128, 11, 0.05
    noises = np.array([0.0, 0.05, 0.1])
    sim = mcmod.MCDataSim(experiment_name="sens", Nspin=N, inspin=a, outspin=b, noises=noises, bootreps=5, training_noise=tn,
                          numcontrollers=C, filemarker=".le", verbose=False, rng_mode="philox", seed=seed)
    state, off0 = np.random.get_state(), sim._philox_offset
    table = sim.get_sensitivity_dict(samples=K)
    assert sim._philox_offset == off0 and all(np.array_equal(x, y) for x, y in zip(state, np.random.get_state()))
    assert list(table) == sim.algos
    nm = noise.structured_perturbation(Nspin=N, inspin=a, outspin=b, noise=0.05)
    h, worst, big = 1e-5, 0.0, 0.0
    for algo in sim.algos:
        rows = sim._controller_rows(algo, tn)
        nvalid = min(len(rows), C)
        ctrl = np.asarray(rows[:nvalid], dtype=np.float64)
        t = {k: np.array(v, dtype=np.float64) for k, v in table[algo].items()}
        assert t["fav"].shape == (3, C) and t["dfav_dlogsigma"].shape == (3, C) and t["direction"].shape == (3, C, N, 3)
        assert np.array_equal(t["noises"], noises)
        assert np.isnan(t["fav"][:, nvalid:]).all() and np.isnan(t["direction"][:, nvalid:]).all()
        for j, sigma in enumerate(noises):
            offset = j * nvalid * K * N * 3
            want = nm.noise_sensitivity(ctrl, be.philox_normal((nvalid, K, N, 3), seed, scale=float(sigma), offset=offset))
            for k in ("fav", "dfav_dlogsigma", "direction"):
                assert np.array_equal(t[k][j, :nvalid], want[k]), (algo, j, k)
            if sigma > 0:
                z = be.philox_normal((nvalid, K, N, 3), seed, scale=1.0, offset=offset)
                fp = be.mc_fidelity(ctrl, sigma * (1 + h) * z, N, a, b).mean(axis=1)
                fm = be.mc_fidelity(ctrl, sigma * (1 - h) * z, N, a, b).mean(axis=1)
                worst = max(worst, float(np.abs((fp - fm) / (2 * h) - t["dfav_dlogsigma"][j, :nvalid]).max()))
                big = max(big, float(np.abs(t["dfav_dlogsigma"][j, :nvalid]).max()))
            else:
                assert (t["dfav_dlogsigma"][j, :nvalid] == 0.0).all()
    print(f"get_sensitivity_dict: d fav / d ln sigma vs central differences: max |diff| = {worst:.2e} (largest slope {big:.2e})")
    assert big > 1e-3
    assert worst < 1.1e-5
    again = sim.get_sensitivity_dict(samples=K)                    # from the cache file
    assert all(np.array_equal(np.array(again[al][k], dtype=float), np.array(table[al][k], dtype=float), equal_nan=True)
               for al in table for k in table[al])
