"""The chain-topology fidelity kernels through the C ABI against the oracle and the golden fixtures: every N, ragged K
and NaN rows, the rare paths (interior splits, degenerate pairs, sweep caps), the mixed-precision eigenvalue route
with its close-pair / stepping / tile-wide fallbacks, the a-posteriori sum-rule guard, long chains, kernel selection,
device-pointer and shared-draw-set entries."""
import ctypes
import importlib
import json
import os
import pickle

import numpy as np
import pytest

import chain_checks as cc
from conftest import highfid_workload, load_json
from gpu_common import rand_ctrl, _h0
from oracle import philox_host
from oracle import robchar_oracle as orc
from test_host_core import _close_pair_matrix

pytestmark = pytest.mark.gpu
TOL = 1e-10


def _inject(ctrl_row, draws_row, d, e):
    """Make one sample's matrix exactly tridiag(d, e): g0 = d - x, g1 = e - 1, g2 = 0 (h0 = 0, J = 1)."""
    N = len(d)
    draws_row[:, 0] = d - ctrl_row[:N]
    draws_row[1:, 1] = e - 1.0
    draws_row[:, 2] = 0.0


def _degenerate_sample(ctrl, draws, c, k, N):
    """Mirror-symmetric controller + draws, chain cut in the middle: the two halves have the SAME spectrum (exactly
    degenerate pairs) - the eigenvalue-only weight formulas cannot serve it."""
    cut = N // 2
    draws[c, k, :, 0] = 0.0
    draws[c, k, cut, 1] = -1.0
    draws[c, k, cut, 2] = 0.0
    if N % 2:                                            # odd N: the middle site is cut off on both sides
        draws[c, k, cut + 1, 1] = -1.0
        draws[c, k, cut + 1, 2] = 0.0
    for i in range(1, cut):
        draws[c, k, N - i, 1:] = draws[c, k, i, 1:]


def test_golden_kernel_cases(be, kernel_cases):
    """Outputs of the unmodified reference (tests/golden/make_golden.py), chain and XXZ."""
    worst = 0.0
    for case in kernel_cases:
        if case["mode"] == "ring":
            continue
        for s in range(case["draws"].shape[0]):
            got = be.mc_fidelity(case["ctrl"], case["draws"][s], case["N"], case["inspin"], case["outspin"],
                                 h0_diag=_h0(case))
            worst = max(worst, np.abs(got - case["fid"][s]).max())
    assert worst < TOL, worst


def test_golden_shipped_sigma0(be, shipped_sigma0):
    """Reference-authored: shipped .le controllers -> sigma_sim = 0 rows of the shipped .mc caches."""
    for sl in shipped_sigma0:
        C = sl["ctrl"].shape[0]
        got = be.mc_fidelity(sl["ctrl"], np.zeros((C, 1, sl["N"], 3)), sl["N"], sl["inspin"], sl["outspin"])[:, 0]
        ok = ~np.isnan(sl["fid"])
        assert np.abs(got[ok] - sl["fid"][ok]).max() < TOL, sl["name"]


def test_golden_lbfgs_n7_and_envtest(be, lbfgs_n7):
    for tag, out in (("0-3", 3), ("0-6", 6)):
        ctrl = lbfgs_n7[f"ctrl_{tag}"]
        got = be.mc_fidelity(ctrl, np.zeros((len(ctrl), 1, 7, 3)), 7, 0, out)[:, 0]
        assert np.abs(got - lbfgs_n7[f"best_fid_{tag}"]).max() < TOL
    for c in load_json("envtest.json"):
        n = c["Nspin"]
        f = be.mc_fidelity(np.array([c["controller"]]), np.zeros((1, 1, n, 3)), n, c["inspin"], c["outspin"])[0, 0]
        assert abs(f - c["fid_reference_noise_model"]) < TOL


@pytest.mark.parametrize("N", list(range(2, 17)))
def test_random_vs_oracle_all_N(be, N):
    rng = np.random.default_rng(100 + N)
    C, K = 7, 193          # ragged: 3 full tiles + 1 lane
    ctrl = rand_ctrl(rng, C, N)
    ctrl[0, :N] = rng.uniform(-1e-6, 1e-6, N)      # near-degenerate diagonal
    ctrl[1, N] *= -1                               # abs(T)
    draws = 0.1 * rng.standard_normal((C, K, N, 3))
    draws[:, :5] = 0.0
    a, b = 0, N - 1
    got = be.mc_fidelity(ctrl, draws, N, a, b)
    want = orc.fidelity_eigh(ctrl, draws, N, a, b)
    assert np.abs(got - want).max() < TOL
    a, b = N // 2, max(0, N // 2 - 1)
    got = be.mc_fidelity(ctrl, draws, N, a, b, h0_diag=orc.xxz_delta(N))
    want = orc.fidelity_eigh(ctrl, draws, N, a, b, h0_diag=orc.xxz_delta(N))
    assert np.abs(got - want).max() < TOL
    # rand_ctrl's rows are localised (for N >= 9 the end-to-end comparison above leans on row 0 alone): delocalised rows too
    cc.check_deloc_vs_oracle(be, N)


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 128, 1000])
def test_ragged_K_and_nan_rows(be, K):
    rng = np.random.default_rng(K)
    N, C = 5, 5
    ctrl = rand_ctrl(rng, C, N)
    ctrl[2] = np.nan                                  # padded controller (mcsim.py:442-443)
    ctrl[4, 1] = np.nan
    draws = 0.05 * rng.standard_normal((C, K, N, 3))
    draws[2] = np.nan                                 # must not be consumed
    got = be.mc_fidelity(ctrl, draws, N, 0, 2)
    want = orc.fidelity_eigh(ctrl, np.nan_to_num(draws), N, 0, 2)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[2]).all() and np.isnan(got[4]).all()
    assert np.nanmax(np.abs(got - want)) < TOL


def test_interior_split_general_path(be):
    """Cut chains (a coupling draw cancels J exactly -> e_i = 0) and strongly graded diagonals; ragged K so that
    several tiles and both staging phases are involved.  (The fast path survives an exactly-zero interior coupling:
    see tridiag_ql2_fast; the general path is pinned by test_general_path_is_exercised.)"""
    rng = np.random.default_rng(77)
    for N in (4, 5, 7, 10, 16):
        C, K = 3, 150
        ctrl = rand_ctrl(rng, C, N)
        ctrl[1, :N] = np.linspace(-1e3, 1e3, N)              # graded
        draws = 0.05 * rng.standard_normal((C, K, N, 3))
        cut = N // 2
        draws[0, 5::7, cut, 1] = -1.0                         # some samples of a tile: chain cut at `cut`
        draws[0, 5::7, cut, 2] = 0.0
        draws[2, :, 1, 1] = -1.0                              # every sample: site 0 isolated
        draws[2, :, 1, 2] = 0.0
        for (a, b) in ((0, N - 1), (N - 1, 0), (cut, cut)):
            got = be.mc_fidelity(ctrl, draws, N, a, b)
            want = orc.fidelity_eigh(ctrl, draws, N, a, b)
            assert np.isfinite(got).all()
            assert np.abs(got - want).max() < TOL, (N, a, b)


def test_general_path_is_exercised(be):
    """The rare general path (per-sample QL window, LDS work vectors) really runs on the GPU and agrees with the
    oracle - counted by rc_stats_general_tiles.  Two triggers: (1) exactly degenerate spectra (mirror-symmetric
    controller, chain cut in the middle, mirror-symmetric draws) make the adjugate weight formulas bail out.  A chain
    cut on every sample, in contrast, stays on the fast path (the cancelled coupling enters as 1e-150)."""
    rng = np.random.default_rng(4242)
    for N in (4, 10, 16):
        C, K, cut = 3, 128, N // 2
        ctrl = rand_ctrl(rng, C, N)
        ctrl[:, N - cut:N] = ctrl[:, :cut][:, ::-1]
        draws = 0.05 * rng.standard_normal((C, K, N, 3))
        draws[:, ::5, :, 0] = 0.0
        draws[:, ::5, cut, 1] = -1.0
        draws[:, ::5, cut, 2] = 0.0
        for i in range(1, cut):
            draws[:, ::5, N - i, 1:] = draws[:, ::5, i, 1:]
        for (a, b, kern) in ((0, N - 1, "auto"), (1, N - 2, "tridiag_adj")):
            be.general_path_tiles(reset=True)
            got = be.mc_fidelity(ctrl, draws, N, a, b, kernel=kern)
            assert be.general_path_tiles() == C * K // 64, (N, a, b)
            assert np.abs(got - orc.fidelity_eigh(ctrl, draws, N, a, b)).max() < TOL, (N, a, b)
    N, C, K = 7, 3, 6400
    ctrl = rand_ctrl(rng, C, N)
    draws = 0.05 * rng.standard_normal((C, K, N, 3))
    draws[:, :, 3, 1] = -1.0
    draws[:, :, 3, 2] = 0.0
    for (a, b) in ((3, 3), (0, 6)):
        be.general_path_tiles(reset=True)
        got = be.mc_fidelity(ctrl, draws, N, a, b)
        assert be.general_path_tiles() == 0                # an exactly cancelled coupling enters as 1e-150: fast path
        sel = slice(0, 400)
        assert np.abs(got[:, sel] - orc.fidelity_eigh(ctrl, draws[:, sel], N, a, b)).max() < TOL
    # (3) pairs INSIDE one half of the cut chain, where the degenerate samples' answer is not 0, on delocalised rows; odd N
    # cut on both sides of the middle site.  N >= 17: no in-register repair - bad lanes go straight to the LDS routine
    for N in (4, 10, 16, 17, 20, 24):
        C, K, cut = 3, 128, N // 2
        ctrl = cc.deloc_ctrl(rng, C, N, 0.5)
        ctrl[:, N] = rng.uniform(0.3 * N, 0.5 * N, C)
        ctrl[:, N - cut:N] = ctrl[:, :cut][:, ::-1]
        draws = 0.05 * rng.standard_normal((C, K, N, 3))
        draws[:, ::5, :, 0] = 0.0
        for c in range(cut, N - cut + 1):
            draws[:, ::5, c, 1] = -1.0
            draws[:, ::5, c, 2] = 0.0
        for i in range(1, cut):
            draws[:, ::5, N - i, 1:] = draws[:, ::5, i, 1:]
        for (a, b, kern) in ((0, cut - 1, "auto"), (1, 1, "tridiag_adj"), (N - 1, N - cut, "auto")):
            be.general_path_tiles(reset=True)
            got = be.mc_fidelity(ctrl, draws, N, a, b, kernel=kern)
            tiles = be.general_path_tiles()
            print(f"general path, N = {N}, ({a}, {b}) {kern}: {tiles} tiles of {C * K // 64}")
            assert tiles == C * K // 64, (N, a, b, tiles)
            want = orc.fidelity_eigh(ctrl, draws, N, a, b)
            cc.assert_has_teeth(want[:, ::5], what=(N, a, b, "degenerate samples"))
            cc.compare(got, want, (N, a, b, kern))


@pytest.mark.parametrize("N", [4, 5, 7, 10])
def test_near_degenerate_spectra_eigenvalue_only_modes(be, N):
    """The eigenvalue-only weight modes deflate at a 1e-10 split tolerance (the eigenvalue error is second order in
    the dropped coupling) and divide by eigenvalue differences; both are most exposed on NEAR-degenerate spectra:
    strongly detuned mirror-symmetric controllers give pairs split by a weak effective coupling, weak noise of
    three magnitudes spreads the gaps over many decades.  Long transfer times amplify eigenvalue errors.  Measured
    worst case 1.3e-12; the rows mode (DBL_EPSILON tolerance, eigenvectors) is the on-device cross-check."""
    rng = np.random.default_rng(900 + N)
    C, K = 24, 512
    ctrl = rand_ctrl(rng, C, N)
    h = N // 2
    ctrl[:, N - h:N] = ctrl[:, :h][:, ::-1]
    ctrl[:, :N] *= 3.0
    ctrl[:, N] = rng.uniform(5.0, 70.0, C)
    worst = 0.0
    for scale in (1e-2, 1e-4, 1e-6):
        draws = scale * rng.standard_normal((C, K, N, 3))
        for (a, b, kern) in ((0, N - 1, "auto"), (1, N - 2, "auto"), (0, h, "tridiag_adj")):
            got = be.mc_fidelity(ctrl, draws, N, a, b, kernel=kern)
            want = orc.fidelity_eigh(ctrl, draws, N, a, b)
            worst = max(worst, np.abs(got - want).max())
            rows = be.mc_fidelity(ctrl, draws, N, a, b, kernel="tridiag_ql")
            assert np.abs(got - rows).max() < 1e-11, (N, scale, a, b)
    assert worst < 1e-11, worst


_LONG_WORST = {"17-24": cc.Worst(), "25-32": cc.Worst()}


@pytest.mark.parametrize("N", list(range(17, 33)))
def test_long_chains_general_kernel(be, N):
    """16 < N <= 32: the register-resident adjugate kernel (17 .. 24) and the LDS-resident general kernel (chain topology
    only); ragged K, a NaN row, XXZ offsets.  The rand_ctrl rows below are localised (end-to-end fidelities down to 1e-26):
    tests/chain_checks.py holds every route to delocalised rows as well."""
    rng = np.random.default_rng(7000 + N)
    C, K = 4, 150
    ctrl = rand_ctrl(rng, C, N)
    ctrl[2, 3] = np.nan
    draws = 0.05 * rng.standard_normal((C, K, N, 3))
    h0 = orc.xxz_delta(N)
    for (a, b, kern, h) in ((0, N - 1, "auto", None), (3, N // 2, "tridiag_ql", None), (0, N - 1, "tridiag_adj", h0)):
        got = be.mc_fidelity(ctrl, draws, N, a, b, h0_diag=h, kernel=kern)
        want = orc.fidelity_eigh(ctrl, draws, N, a, b, h0_diag=h)
        assert np.isnan(got[2]).all()
        ok = [0, 1, 3]
        assert np.abs(got[ok] - want[ok]).max() < TOL, (N, a, b)
    with pytest.raises(Exception):
        be.mc_fidelity(ctrl, draws, N, 0, N - 1, ring=True)
    with pytest.raises(Exception):
        be.mc_fidelity(ctrl, draws, N, 0, N - 1, kernel="expm")
    with pytest.raises(Exception):
        be.mc_fidelity(rand_ctrl(rng, 2, 33), np.zeros((2, 4, 33, 3)), 33, 0, 32)
    worst = _LONG_WORST["17-24" if N <= 24 else "25-32"]
    cc.check_long_chain(be, N, worst)
    print(f"long chains N = 17 ... {N}: " + " | ".join(f"{k}: {v}" for k, v in _LONG_WORST.items()))


@pytest.mark.parametrize("N", list(range(2, 33)))
def test_closed_form_chain_every_kernel(be, N):
    """The spin-j chain (H = lam Jx + g Jz: non-unit h0_offdiag, fidelities in closed form) from both ends to every site,
    every kernel that accepts N, T from 0 to the first full transfer."""
    worst = cc.Worst()
    cc.check_closed_form(be, N, worst)
    print(f"closed form N = {N}: {worst}")


@pytest.mark.parametrize("N", [2, 3, 5, 7, 10, 16])
def test_adjugate_variant(be, N):
    """Kernel variant RC_KERNEL_TRIDIAG_ADJ (eigenvalues by QL, eigenvector weights from the adjugate formula):
    random, near-degenerate, resonant-ends, mirror-symmetric and cut-chain inputs against the oracle."""
    rng = np.random.default_rng(N + 40)
    C, K = 12, 130
    ctrl = rand_ctrl(rng, C, N)
    ctrl[0:3, N - 1] = ctrl[0:3, 0] + np.array([1e-9, 1e-12, 0.0])
    ctrl[3:6, :N] = (ctrl[3:6, :N] + ctrl[3:6, N - 1::-1]) / 2
    ctrl[6, :N] = 0.0
    ctrl[7, :N] = rng.uniform(-1e-6, 1e-6, N)
    draws = 0.05 * rng.standard_normal((C, K, N, 3))
    draws[:, :5] = 0.0
    if N > 2:
        draws[8, ::3, N // 2, 1] = -1.0
        draws[8, ::3, N // 2, 2] = 0.0
    for (a, b) in ((0, N - 1), (0, N // 2), (N // 2, N // 2)):
        got = be.mc_fidelity(ctrl, draws, N, a, b, kernel="tridiag_adj")
        want = orc.fidelity_eigh(ctrl, draws, N, a, b)
        assert np.abs(got - want).max() < TOL, (N, a, b)


def test_empty_and_errors(be):
    lib = importlib.import_module("code-robchar_amd._lib")
    out = be.mc_fidelity(np.zeros((0, 6)), np.zeros((0, 4, 5, 3)), 5, 0, 2)
    assert out.shape == (0, 4)
    out = be.mc_fidelity(np.ones((3, 6)), np.zeros((3, 0, 5, 3)), 5, 0, 2)
    assert out.shape == (3, 0)
    with pytest.raises(ValueError):
        be.mc_fidelity(np.ones((3, 6)), np.zeros((3, 2, 5, 3)), 5, 0, 5)
    with pytest.raises(ValueError):
        be.mc_fidelity(np.ones((3, 34)), np.zeros((3, 2, 33, 3)), 33, 0, 5)
    with pytest.raises(lib.RobCharHipError):
        be.mc_fidelity(np.ones((3, 6)), np.zeros((3, 2, 5, 3)), 5, 0, 2, ring=True, kernel="tridiag_ql")


@pytest.mark.parametrize("seed", range(6))
def test_random_configs_all_kernels(be, seed):
    """Random (N, in, out, sigma, K) against the oracle for every applicable kernel variant."""
    rng = np.random.default_rng(1000 + seed)
    for _ in range(6):
        N = int(rng.integers(2, 17))
        a, b = int(rng.integers(0, N)), int(rng.integers(0, N))
        if rng.random() < 0.4:
            a, b = 0, N - 1
        C, K = int(rng.integers(1, 6)), int(rng.integers(1, 200))
        sigma = float(rng.choice([0.0, 0.01, 0.05, 0.1, 0.3]))
        ctrl = rand_ctrl(rng, C, N)
        draws = sigma * rng.standard_normal((C, K, N, 3))
        h0 = orc.xxz_delta(N) if rng.random() < 0.3 else None
        want = orc.fidelity_eigh(ctrl, draws, N, a, b, h0_diag=h0)
        for kern in ("auto", "tridiag_ql", "tridiag_adj", "jacobi"):
            got = be.mc_fidelity(ctrl, draws, N, a, b, h0_diag=h0, kernel=kern)
            assert np.abs(got - want).max() < TOL, (N, a, b, sigma, kern)
    # as many configurations again on delocalised rows, N up to 32 (most of the ones above have max F < 1e-3)
    cc.check_random_deloc_configs(be, seed)


def test_torch_device_pointer_path(be):
    """Device-resident inputs through the *_async entry points on torch's current stream."""
    import torch
    rng = np.random.default_rng(5)
    N, C, K = 5, 10, 777
    ctrl = rand_ctrl(rng, C, N)
    draws = 0.05 * rng.standard_normal((C, K, N, 3))
    want = orc.fidelity_eigh(ctrl, draws, N, 0, 4)
    dt = torch.from_numpy(draws).cuda()
    ct = torch.from_numpy(ctrl).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = be.mc_fidelity(ct, dt, N, 0, 4)
        red = be.reduce_metrics(got, dkw_eps=0.01, want_sorted=True)
    s.synchronize()
    assert np.abs(got.cpu().numpy() - want).max() < TOL
    assert np.abs(red["rim1"][0].cpu().numpy() - (1 - want).mean(axis=1)).max() < TOL
    assert np.array_equal(red["sorted"].cpu().numpy(), np.sort(got.cpu().numpy(), axis=1))


def test_shared_draw_set_optimiser_objective(be):
    """One fixed set of R real perturbations applied to every controller (qnewton.py:122-137, :426-444) without
    replicating it: numpy and torch entry, all kernels, mean fidelity."""
    import torch
    noise = importlib.import_module("code-robchar_amd.noise")
    rng = np.random.default_rng(12)
    N, C, R = 6, 33, 100
    ctrl = rand_ctrl(rng, C, N)
    nm = noise.structured_perturbation(Nspin=N, inspin=0, outspin=3, noise=0.05)
    np.random.seed(4)
    dset = nm.fixed_perturbation_set(R)
    np.random.seed(4)
    want_set = np.random.normal(scale=0.05, size=(R, N, 2))
    assert np.array_equal(dset[..., :2], want_set) and not dset[..., 2].any()
    full = np.broadcast_to(dset[None], (C, R, N, 3))
    want = orc.fidelity_eigh(ctrl, full, N, 0, 3)
    for kern in ("auto", "tridiag_adj", "jacobi"):
        got = be.mc_fidelity(ctrl, dset[None], N, 0, 3, kernel=kern)
        assert got.shape == (C, R) and np.abs(got - want).max() < TOL, kern
    got_t = be.mc_fidelity(torch.from_numpy(ctrl).cuda(), torch.from_numpy(dset[None].copy()).cuda(), N, 0, 3)
    assert np.abs(got_t.cpu().numpy() - want).max() < TOL
    assert np.abs(nm.fidelity_ss_av(ctrl, dset) - want.mean(axis=1)).max() < 1e-12


def test_blocking_entries_from_two_threads(be):
    """The blocking C entries are thread-safe per device (per-device lock, workspace and stream)."""
    import threading
    rng = np.random.default_rng(3)
    N, C, K = 5, 20, 300
    jobs = []
    for t in range(4):
        ctrl = rand_ctrl(rng, C, N)
        draws = 0.05 * rng.standard_normal((C, K, N, 3))
        jobs.append([ctrl, draws, None])
    def run(j):
        for _ in range(5):
            j[2] = be.mc_fidelity(j[0], j[1], N, 0, 4)
    th = [threading.Thread(target=run, args=(j,)) for j in jobs]
    [t.start() for t in th]
    [t.join() for t in th]
    for ctrl, draws, got in jobs:
        assert np.abs(got - orc.fidelity_eigh(ctrl, draws, N, 0, 4)).max() < TOL


@pytest.mark.parametrize("N", [5, 7, 8, 10, 12])
def test_mixed_precision_path_close_pairs(be, N):
    """The mixed-precision eigenvalue path (fp32 QL + fp64 Halley step, N = 3..13) on the spectra it finds hardest: two
    resonant sites far apart (biases equal to ~1e-4, everything between them detuned by 2 .. 8 J), so that every sample
    has an eigenvalue pair 1e-5 .. 1e-2 apart - down to far closer than the fp32 phase resolves.  Such tiles leave the one-step path
    (`polish_tiles`), keep stepping, and must still agree with the oracle to 1e-10 in both weight modes; what the
    stepping cannot settle goes to the general path and must agree as well."""
    rng = np.random.default_rng(4242 + N)
    C, K = 24, 1280
    ctrl = np.empty((C, N + 1))
    ctrl[:, :N] = rng.uniform(2.0, 8.0, (C, 1)) * (-1.0) ** np.arange(N) + rng.uniform(-0.5, 0.5, (C, N))
    ctrl[:, 0] = 1.0 + rng.uniform(-0.2, 0.2, C)
    ctrl[:, N - 1] = ctrl[:, 0] + rng.uniform(-1e-4, 1e-4, C)          # resonant ends
    ctrl[:, N] = rng.uniform(20, 30, C)
    draws = 3e-4 * rng.standard_normal((C, K, N, 3))
    for (a, b) in ((0, N - 1), (0, N // 2), (N - 1, 1)):
        be.general_path_tiles(reset=True)
        be.polish_tiles(reset=True)
        got = be.mc_fidelity(ctrl, draws, N, a, b)
        assert be.polish_tiles() > 0, (N, a, b)                          # the stepping path really ran
        assert be.general_path_tiles() <= C * K // 64                    # (any number of tiles may; all must be right)
        ref = orc.fidelity_eigh(ctrl, draws, N, a, b)
        assert np.abs(got - ref).max() < TOL, (N, a, b, np.abs(got - ref).max())
        # the transfer through a detuned chain is weak (fidelities 1e-9 .. 0.3): the weights must be right in
        # RELATIVE terms too, or the absolute tolerance would hide a wrong small number
        assert (np.abs(got - ref) <= 1e-12 + 1e-7 * ref).all(), (N, a, b)
    # the rows mode (all-fp64 QL with accumulated eigenvector rows) is the independent cross-check on the same inputs
    rows = be.mc_fidelity(ctrl, draws, N, 0, N - 1, kernel="tridiag_ql")
    assert np.abs(rows - be.mc_fidelity(ctrl, draws, N, 0, N - 1)).max() < TOL


@pytest.mark.parametrize("N", [5, 7, 10, 13])
def test_close_pairs_stay_on_the_wave_wide_route(be, N):
    """Samples whose spectrum has a pair 1e-3 ... 1e-10 apart WITH O(1) weights on both members (Jacobi matrices with a
    prescribed spectrum, injected through the draws).  Round 2 sent everything closer than 1e-7 of the scale to the
    per-sample general routine (a ~100 us single-lane straggler at N >= 10); now the tile-wide all-fp64 QL (tight split
    tolerance) + product-formula weights carry them for the END-TO-END weights (no general-path tile); the general adjugate
    weights have a 4e-6 threshold (their numerators are recurrences evaluated beside their own roots - the fuzz campaign of
    round 3) and hand such samples to the in-register eigenvector repair.  Parity 1e-10 either way."""
    rng = np.random.default_rng(900 + N)
    C, K = 4, 256
    ctrl = rand_ctrl(rng, C, N)
    ctrl[:, N] = rng.uniform(15, 30, C)
    draws = 0.02 * rng.standard_normal((C, K, N, 3))
    gaps = []
    for c in range(C):
        for k in range(0, K, 7):                       # several per tile, most tiles
            delta = 10.0 ** rng.uniform(-10, -3)
            d, e, true, j = _close_pair_matrix(N, delta, rng)
            shift = rng.uniform(-3, 3)
            _inject(ctrl[c], draws[c, k], d + shift, e)
            gaps.append(delta)
    for (a, b) in ((0, N - 1), (0, N // 2), (N - 2, 1)):
        be.general_path_tiles(reset=True)
        be.polish_tiles(reset=True)
        got = be.mc_fidelity(ctrl, draws, N, a, b)
        ref = orc.fidelity_eigh(ctrl, draws, N, a, b)
        assert np.abs(got - ref).max() < TOL, (N, a, b, np.abs(got - ref).max())
        assert be.polish_tiles() > 0
        if (a, b) == (0, N - 1):
            assert be.general_path_tiles() == 0, (N, a, b)          # end-to-end weights: wave-wide down to 1e-12 of the scale
        else:
            assert be.general_path_tiles() > 0                      # general adjugate weights: below 4e-6 the eigenvector route
    assert min(gaps) < 1e-8


def test_fuzz_regression_cut_chain_near_degenerate(be):
    """The inputs the round-3 fuzz campaign failed on (see tests/test_host_core.py, same fixture) on the GPU: every chain
    kernel, 1e-10."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_r3_adjugate_cut_chain.npz"))
    for name in z["names"]:
        name = str(name)
        N, a, b = (int(v) for v in z[name + "_meta"])
        ctrl, draws = z[name + "_ctrl"], z[name + "_draws"]
        h0 = z[name + "_h0"] if z[name + "_h0"].size else None
        want = orc.fidelity_eigh(ctrl, draws, N, a, b, h0_diag=h0)
        for kern in ("auto", "tridiag_adj", "tridiag_ql"):
            got = be.mc_fidelity(ctrl, draws, N, a, b, h0_diag=h0, kernel=kern)
            assert np.abs(got - want).max() < TOL, (name, kern, np.abs(got - want).max())


@pytest.mark.parametrize("N,xxz", [(10, True), (7, False)])
def test_rare_path_cost_is_bounded(be, N, xxz):
    """A 1e6-evaluation launch in which ONE sample is exactly degenerate must cost at most 1.3x the clean launch (round 2:
    the per-sample LDS routine ran ~100 us at N = 10 - longer than the whole launch; measured now: 120.4 -> 120.8 us).
    Also a launch with a degenerate sample in one tile of a hundred (158 of 15 700 tiles; measured 1.33x at N = 10 - each
    such tile runs the fp32 QL, the stepping attempts, the tile-wide fp64 QL and then the rows-mode QL for its one lane):
    bounded by 1.6x."""
    import torch
    rng = np.random.default_rng(77 + N)
    C, K = 100, 10000
    ctrl = rand_ctrl(rng, C, N)
    cut = N // 2
    ctrl[3, N - cut:N] = ctrl[3, :cut][::-1]             # controller 3 is mirror-symmetric
    ctrl[:, N - cut:N][::2] = ctrl[:, :cut][::2, ::-1]    # ... and so is every second one
    h0 = orc.xxz_delta(N) if xxz else None                # (the XXZ offsets are mirror-symmetric themselves)
    clean = 0.05 * rng.standard_normal((C, K, N, 3))
    one = clean.copy()
    _degenerate_sample(ctrl, one, 2, 4711, N)
    many = clean.copy()
    tiles_per_ctrl = (K + 63) // 64
    hit = []
    for t in range(0, C * tiles_per_ctrl, 50):
        c, k = divmod(t, tiles_per_ctrl)
        if c % 2 == 0:
            _degenerate_sample(ctrl, many, c, k * 64 + 5, N)
            hit.append((c, k * 64 + 5))
    dev = be.compute_device()
    ct = torch.from_numpy(ctrl).to(dev)
    tens = {name: torch.from_numpy(x).to(dev) for name, x in (("clean", clean), ("one", one), ("many", many))}
    out = torch.empty((C, K), dtype=torch.float64, device=dev)

    def run(name):
        return be.mc_fidelity(ct, tens[name], N, 0, N - 1, h0_diag=h0, out=out)

    # results first: the degenerate samples are right (transfer across a cut: 0) and really took the repair path
    be.general_path_tiles(reset=True)
    got = run("one").cpu().numpy()
    assert be.general_path_tiles() == 1
    sel = np.arange(4700, 4730)
    assert np.abs(got[2, sel] - orc.fidelity_eigh(ctrl[2:3], one[2:3, sel], N, 0, N - 1, h0_diag=h0)[0]).max() < TOL
    assert got[2, 4711] < 1e-20
    be.general_path_tiles(reset=True)
    got = run("many").cpu().numpy()
    assert be.general_path_tiles() == len(hit)
    for (c, k) in hit[:: max(1, len(hit) // 20)]:
        assert got[c, k] < 1e-20
    # cost: medians of interleaved launches (HIP events), after a settling burst
    for _ in range(300):
        run("clean")
    torch.cuda.synchronize()
    times = {"clean": [], "one": [], "many": []}
    for rep in range(40):
        for name in times:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(4):
                run(name)
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / 4)
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(f"N={N}: clean {med['clean'] * 1e3:.1f} us, one degenerate sample {med['one'] * 1e3:.1f} us, "
          f"{len(hit)} degenerate samples {med['many'] * 1e3:.1f} us")
    assert med["one"] <= 1.3 * med["clean"], med
    # 158 repaired tiles: +32 ... +36 us on every box of rounds 4 and 5 (N = 7: 90.8 ... 94.4 us against a clean 58.3 ... 62.4 us, i.e.
    # 1.50 ... 1.61x - the RATIO moves with the clean launch's speed, the repair cost does not): bound the cost per repaired tile
    # (measured 0.20 ... 0.23 us at N = 7, 0.25 us at N = 10) and keep a looser ratio
    assert (med["many"] - med["clean"]) * 1e3 <= 0.35 * len(hit), med
    assert med["many"] <= 1.75 * med["clean"], med


def test_sum_rule_guard_on_the_device(be):
    """The a-posteriori guard (tridiag_core.h: kSumRuleGuard) inside the kernels.  (1) It must not send healthy samples to the
    eigenvector route: the benchmark-style workloads of every weight mode and (in, out) class - same site, neighbours, two
    apart, far apart, end to end - stay (almost) off the repair path.  (2) The configuration in which the round-3 fuzz
    campaign found its worst chain error (2.6e-11: N = 6, in = out = 1, |bias| <= 1, a weak bond between mirror halves -
    recurrence noise in the adjugate numerators next to a pair just above the 4e-6 hand-over threshold) now comes out at
    a few 1e-12: the guard catches what the threshold let through."""
    rng = np.random.default_rng(77)
    for N in (5, 7, 10, 13):
        C, K = 40, 640
        ctrl = rand_ctrl(rng, C, N)
        draws = 0.05 * rng.standard_normal((C, K, N, 3))
        be.general_path_tiles(reset=True)
        pairs = [(0, N - 1), (0, 0), (N // 2, N // 2), (N - 1, N - 1), (0, 1), (N // 2, N // 2 - 1), (0, 2), (1, N - 2), (N - 1, 0)]
        for (a, b) in pairs:
            got = be.mc_fidelity(ctrl, draws, N, a, b)
            want = orc.fidelity_eigh(ctrl, draws, N, a, b)
            assert np.abs(got - want).max() < 1e-11, (N, a, b, np.abs(got - want).max())
        tiles = len(pairs) * C * (K // 64)
        rep = be.general_path_tiles()
        print(f"guard, N = {N}: {rep} of {tiles} tiles with a repaired sample on random controllers")
        assert rep <= 0.01 * tiles + 2, (N, rep, tiles)
    # the round-3 worst case, regenerated (scripts/fuzz_parity.py, seed 2150, configuration 17: N = 6, a = b = 1)
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    from host_fuzz_guard import configs
    for meta, ctrl, draws, h0 in configs(2150, 18):
        if meta["it"] != 17:
            continue
        assert (meta["N"], meta["a"], meta["b"]) == (6, 1, 1)
        want = orc.fidelity_eigh(ctrl, draws, 6, 1, 1, h0_diag=h0)
        for kern in ("auto", "tridiag_adj"):
            err = np.abs(be.mc_fidelity(ctrl, draws, 6, 1, 1, h0_diag=h0, kernel=kern) - want).max()
            print(f"round-3 worst fuzz case ({kern}): max |dF| = {err:.2e} (round 3: 2.57e-11)")
            assert err < 1e-11, err


def test_settled_lanes_keep_their_polished_eigenvalues(be):
    """Regression fixture of the round-4 fuzz campaign (seeds 4020 / 4092 / 4117, |bias| ~ 100, |T| ~ 70 .. 95: the worst chain
    cases, 1.05e-11 .. 1.41e-11): healthy samples whose 64-sample TILE took the tile-wide all-fp64 QL because of a neighbour
    had their polished eigenvalues replaced by QL eigenvalues (error ~ N eps scale = 2e-13 absolute - a phase error of 1e-11
    at that T).  Settled lanes now keep what they had: every tile of the fixture (input = one controller row + the tile's 64
    samples, so the wave composition is the campaign's) comes out below 5e-12 in both eigenvalue-only weight modes."""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_r4_tile_fallback.npz"))
    keys = sorted(k[:-5] for k in d.files if k.endswith("_ctrl"))
    assert len(keys) == 15
    worst = 0.0
    for key in keys:
        N, a, b = (int(v) for v in d[key + "_meta"])
        h0 = d[key + "_h0"] if d[key + "_h0"].size else None
        ctrl, draws, want = d[key + "_ctrl"], d[key + "_draws"], d[key + "_want"]
        assert np.abs(orc.fidelity_eigh(ctrl, draws, N, a, b, h0_diag=h0) - want).max() < 1e-13     # the fixture's own oracle values
        before = np.abs(d[key + "_gpu_round4_before"] - want).max()
        for kern in ("auto", "tridiag_adj"):
            err = np.abs(be.mc_fidelity(ctrl, draws, N, a, b, h0_diag=h0, kernel=kern) - want).max()
            worst = max(worst, err)
            assert err < 5e-12, (key, kern, err, before)
    print(f"round-4 fuzz worst tiles: max |dF| = {worst:.2e} (before: up to 1.41e-11)")


def test_hostile_inputs_return_and_leave_their_neighbours_alone():
    """Infinities, NaNs, 1e300s and denormals in controllers (T = inf, a 1e300 bias) and draws, every kernel route (chain: auto /
    rows / adjugate / Jacobi / expm; ring: mixed / all-fp64 / Jacobi), N = 2 ... 24 (`scripts/hostile_inputs.py`, in a process of
    its own under a time limit): every launch returns - all device loops are capped; round 5 found `(int) ceil(log2(inf))`
    squarings in the expm kernel by reading them -, hostile samples hold NaN (or whatever their values honestly give), and the
    clean samples of the same tiles still agree with the oracle to 1e-10."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "hostile_inputs.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-1500:], r.stderr[-1500:])


def test_plain_c_client_of_the_c_abi(be, tmp_path):
    """The boundary without Python in it: `tests/host/c_client.c` (plain C99, host buffers, the blocking entries) built with gcc
    and run as a process of its own; its fidelities and metric rows against the oracle, and its error path (a code and a message)."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "code-robchar_amd", "csrc")
    exe = str(tmp_path / "c_client")
    subprocess.run(["gcc", "-std=c99", "-O1", "-I", os.path.join(root, "include"), "-o", exe, os.path.join(root, "tests", "host", "c_client.c"),
                    "-L", libdir, "-lrobchar_hip", f"-Wl,-rpath,{libdir}"], check=True)
    rng = np.random.default_rng(31)
    for (N, a, b, ring, C, K) in ((5, 0, 2, 0, 3, 130), (7, 0, 6, 0, 2, 64), (6, 1, 4, 1, 2, 70)):
        ctrl = rand_ctrl(rng, C, N)
        draws = 0.05 * rng.standard_normal((C, K, N, 3))
        text = f"{N} {a} {b} {ring} {C} {K}\n" + " ".join(repr(float(v)) for v in ctrl.ravel()) + "\n" + " ".join(repr(float(v)) for v in draws.ravel()) + "\n"
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr[-1000:])
        lines = r.stdout.strip().splitlines()
        assert lines[0].startswith("version ") and int(lines[0].split()[1]) >= 6 and int(lines[0].split()[3]) >= 1
        fid = np.array([float(v) for v in lines[1:1 + C * K]]).reshape(C, K)
        want = orc.fidelity_eigh(ctrl, draws, N, a, b, ring=bool(ring))
        assert np.abs(fid - want).max() < TOL, (N, ring)
        rows = np.array([[float(v) for v in ln.split()] for ln in lines[1 + C * K:1 + C * K + C]])
        assert np.abs(rows[:, 0] - (1.0 - want).mean(axis=1)).max() < TOL and np.abs(rows[:, 1] - want.std(axis=1)).max() < TOL
        assert np.abs(rows[:, 2] - want.min(axis=1)).max() < TOL and np.abs(rows[:, 3] - (want >= 0.95).mean(axis=1)).max() < 1e-12
        assert lines[-1].startswith("bad-argument call: -1 (") and "out of range" in lines[-1]


def test_hip_host_client_on_the_enqueue_only_entries(be, tmp_path):
    """`tests/host/hip_client.cpp`: a HIP host program (hipcc, no Python, no torch) with its own device buffers and TWO streams -
    counter-based draws, the fidelity kernel and the reduction enqueued behind each other through the `_async` entries, nothing
    synchronised until the copies back.  Its fidelities equal the Python layer's on the same stream elements bit for bit (both
    streams), and the oracle's to 1e-10; its metric rows equal `reduce_metrics`'."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "code-robchar_amd", "csrc")
    exe = str(tmp_path / "hip_client")
    subprocess.run([hipcc, "-O1", "--offload-arch=gfx950", "-I", os.path.join(root, "include"), "-o", exe,
                    os.path.join(root, "tests", "host", "hip_client.cpp"), "-L", libdir, "-lrobchar_hip", f"-Wl,-rpath,{libdir}"], check=True)
    rng = np.random.default_rng(41)
    for (N, a, b, C, K, seed, sigma) in ((7, 0, 6, 5, 1000, 123, 0.05), (10, 2, 7, 3, 333, 9, 0.02)):
        ctrl = rand_ctrl(rng, C, N)
        r = subprocess.run([exe, str(N), str(a), str(b), str(C), str(K), str(seed), repr(sigma)],
                           input=" ".join(repr(float(v)) for v in ctrl.ravel()) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr[-1000:])
        vals = r.stdout.split()
        fid_a = np.array([float(v) for v in vals[:C * K]]).reshape(C, K)
        rows = np.array([float(v) for v in vals[C * K:C * K + 4 * C]]).reshape(C, 4)
        fid_b = np.array([float(v) for v in vals[C * K + 4 * C:]]).reshape(C, K)
        draws = be.philox_normal((C, K, N, 3), seed=seed, scale=sigma)
        mine = np.asarray(be.mc_fidelity(ctrl, draws, N, a, b))
        assert np.array_equal(fid_a, mine) and np.array_equal(fid_b, mine)
        assert np.abs(fid_a - orc.fidelity_eigh(ctrl, draws, N, a, b)).max() < TOL
        red = be.reduce_metrics(mine, q_thresholds=(0.95,), dkw_eps=0.0)
        for j, name in enumerate(("rim1", "std", "min")):
            assert np.array_equal(rows[:, j], np.asarray(red[name])[0]), name
        assert np.array_equal(rows[:, 3], np.asarray(red["q"])[0, 0])
