"""`backend.mc_fidelity_grad_philox` - the fidelity gradient with the counter-based draws generated inside the kernel and the
second-moment sums behind the gradient of the variance - on the device: BIT-IDENTICAL to the two-kernel route (`philox_normal` +
`mc_fidelity_grad`) in fid, grad and mean at every pass schedule (one pass: N <= 9; several: N = 10, 11, 12), both parities of
the first element, tile boundaries, both draw modes and per-row sigma; the moment sums against host sums of the same launch's
per-sample outputs; everything against an independent reference (host-regenerated draws, eigh); and through
`scripts/robust_lbfgs.py`.  With static Hamiltonian terms (XXZ diagonal, non-unit couplings of both signs), rows of more than 64
tiles in the row-mean kernel and stream offsets past 2^33: the checks of grad_checks.py (`check_*_grad_philox`).  Shapes are the
smallest that reach those paths: C = 3 rows (one NaN, one with a negative time entry), K = 130 = tiles of 64, 64 and 2 samples.
ROBCHAR_GRAD_FORCED_GENERAL=1 announces a -DRC_GRAD_FORCE_GENERAL=1 variant build (scripts/build_variant.sh), in which every
tile takes the sweep-cap fallback."""
import importlib
import itertools
import os
import sys

import numpy as np
import pytest

import chain_checks as cc
import grad_checks as gc
from oracle import philox_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCED = os.environ.get("ROBCHAR_GRAD_FORCED_GENERAL") == "1"      # a -DRC_GRAD_FORCE_GENERAL=1 variant build
SIGMA = 0.05
SEED = 0x5EED000A
EPS = 2.0 ** -52
IDENTITY_N = (2, 3, 7, 9, 10, 11, 12)
KEYS = ("fid", "grad", "mean")
ALL = KEYS + ("moment",)


ctrl_rows = gc.philox_ctrl      # delocalised rows (the gradients have teeth there), one of them NaN, one with a negative time entry


def fused(be, ctrl, K, N, a, b, offset=0, sigma=SIGMA, seed=SEED, shared=False, want=ALL, h0_diag=None, h0_offdiag=None):
    import torch
    dev = be.compute_device()
    if not isinstance(sigma, float):
        sigma = torch.from_numpy(np.asarray(sigma, dtype=np.float64)).to(dev)
    res = be.mc_fidelity_grad_philox(torch.from_numpy(ctrl).to(dev), K, N, a, b, seed, offset=offset, sigma=sigma, shared=shared,
                                     h0_diag=h0_diag, h0_offdiag=h0_offdiag, want=want)
    return {k: v.cpu().numpy() for k, v in res.items()}


def two_kernels(be, ctrl, K, N, a, b, offset=0, sigma=SIGMA, seed=SEED, shared=False, h0_diag=None, h0_offdiag=None):
    draws = be.philox_normal((1 if shared else ctrl.shape[0], K, N, 3), seed, scale=sigma, offset=offset)
    return be.mc_fidelity_grad(ctrl, draws, N, a, b, h0_diag=h0_diag, h0_offdiag=h0_offdiag)


def assert_same_bits(got, want, what, keys=KEYS):
    gc.assert_same_bits(got, want, what, keys)


def check_identity(be, N, K=130, offsets=(0, 7)):
    ctrl = ctrl_rows(N)
    for (a, b) in gc.grad_pairs(N):
        for offset in offsets:
            want = two_kernels(be, ctrl, K, N, a, b, offset)
            gc.assert_grad_teeth(want["grad"], ("two-kernel route", N, a, b, offset))
            got = fused(be, ctrl, K, N, a, b, offset)
            assert all(np.isnan(want[k][1]).all() for k in KEYS) and all(np.isnan(got[k][1]).all() for k in ALL)
            assert np.isfinite(got["moment"][[0, 2]]).all()
            assert_same_bits(got, want, (N, a, b, offset, K))


@pytest.mark.parametrize("N", IDENTITY_N)
def test_bit_identity_with_the_two_kernel_route(be, N):
    """(a forced variant build: both routes send every tile through the sweep-cap fallback - here the draws element by element
    from philox_element, the textbook QL in LDS - and must still agree bit for bit; the counter counts instead of staying 0)"""
    be.grad_general_tiles(reset=True)
    check_identity(be, N)
    tiles = be.grad_general_tiles(reset=True)
    assert (tiles > 0) if FORCED else (tiles == 0), tiles


@pytest.mark.parametrize("K", (1, 64, 65))
def test_tile_boundaries(be, K):
    check_identity(be, 7, K=K)


@pytest.mark.parametrize("N", (7, 10))
def test_shared_draws(be, N):
    """shared=True is mc_fidelity_grad on the ONE set philox_normal((1, K, N, 3)), and not the per-controller mode"""
    K = 130
    ctrl = ctrl_rows(N)
    for (a, b) in gc.grad_pairs(N):
        for offset in (0, 7):
            want = two_kernels(be, ctrl, K, N, a, b, offset, shared=True)
            gc.assert_grad_teeth(want["grad"], ("two-kernel route, shared set", N, a, b, offset))
            got = fused(be, ctrl, K, N, a, b, offset, shared=True)
            assert_same_bits(got, want, (N, a, b, offset, "shared"))
            per = fused(be, ctrl, K, N, a, b, offset)
            assert np.array_equal(per["fid"][0], got["fid"][0]) and np.array_equal(per["grad"][0], got["grad"][0])
            assert (per["fid"][2] != got["fid"][2]).mean() > 0.99 and not np.array_equal(per["mean"][2], got["mean"][2])


@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("N", (7, 10))
def test_per_row_sigma(be, N, shared):
    """sigma_rows = (0, 0.02, 0.1): every row equals a scalar-sigma call of the two-kernel route for that row - at the row's own
    offset in the per-controller mode, at the same offset in the shared mode; in the sigma = 0 row all K samples carry the same
    bits."""
    K, a, b = 130, 0, N - 1
    rows = np.array([0.0, 0.02, 0.1])
    ctrl = ctrl_rows(N, nan_row=None)
    for offset in (0, 7):
        got = fused(be, ctrl, K, N, a, b, offset, sigma=rows, shared=shared)
        for c, sigma in enumerate(rows):
            off_c = offset if shared else offset + c * K * N * 3
            want = two_kernels(be, ctrl[c:c + 1], K, N, a, b, off_c, sigma=float(sigma), shared=shared)
            assert_same_bits({k: got[k][c:c + 1] for k in KEYS}, want, (N, offset, shared, "row", c))
        gc.assert_grad_teeth(got["grad"], ("per-row sigma", N))
        assert (got["grad"][0] == got["grad"][0, :1]).all() and (got["fid"][0] == got["fid"][0, 0]).all()
        assert not (got["fid"][1] == got["fid"][1, 0]).all()


host_moments = gc.host_moments


@pytest.mark.parametrize("N", (7, 11))
def test_moments_against_the_same_launch(be, N):
    """`moment` = mean(fid^2), mean(fid dF/dx) of the SAME launch's per-sample outputs within K 2^-52 max(1, max |entry|) (the
    bound grad_checks.check_mean_and_shared uses for `mean`); the same bits on a second run, for every subset of `want`, and on a
    side stream."""
    import torch
    K, a, b, offset = 130, 0, N - 1, 7
    ctrl = ctrl_rows(N)
    for shared in (False, True):
        full = fused(be, ctrl, K, N, a, b, offset, shared=shared)
        ok = [0, 2]
        rows = host_moments(full)
        scale = max(1.0, float(np.abs(full["grad"][ok]).max()))
        err = float(np.abs(full["moment"][ok] - rows[ok]).max())
        print(f"moment sums, N = {N}, shared = {shared}: max |kernel - host| = {err:.2e} (bound {K * EPS * scale:.2e})")
        assert err <= K * EPS * scale
        assert np.abs(rows[ok, 1:]).max() > 1e-3 and rows[ok, 0].min() > 1e-3
        assert_same_bits(fused(be, ctrl, K, N, a, b, offset, shared=shared), full, "second run", ALL)
        for r in range(1, len(ALL) + 1):
            for sub in itertools.combinations(ALL, r):
                only = fused(be, ctrl, K, N, a, b, offset, shared=shared, want=sub)
                assert set(only) == set(sub)
                assert_same_bits(only, full, sub, sub)
    dev = be.compute_device()
    side = torch.cuda.Stream(device=dev)
    ct = torch.from_numpy(ctrl).to(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        got = be.mc_fidelity_grad_philox(ct, K, N, a, b, SEED, offset=offset, sigma=SIGMA, shared=True)
    side.synchronize()
    assert all(got[k].device == ct.device for k in ALL)
    assert_same_bits({k: v.cpu().numpy() for k, v in got.items()}, full, "side stream", ALL)


@pytest.mark.parametrize("sigma", (0.05, 0.1))
@pytest.mark.parametrize("N", (5, 10))
def test_independent_reference(be, N, sigma):
    """draws regenerated on the host (oracle/philox_host.py), reference grad_checks.grad_eigh.  fid, grad, mean inside
    chain_checks.TOL / grad_checks.grad_bars; from `fidelity_moments_philox`: var within 4 TOL of np.var(F_ref) (F <= 1:
    |d mean F^2| <= 2 TOL, |d fav^2| <= 2 TOL); grad_var = 2 (mean F dF - fav mean dF) inside 4 (TOL max_k |dF_ref| + the row's
    largest bar) (each of the two products: error of F times |dF| plus F <= 1 times the error of dF); grad_std 2 std = grad_var
    to 1e-14 relative.  Teeth: every std >= 0.01 and every |grad Var| entry of the reference >= 100 x its bound."""
    noise = importlib.import_module("code-robchar_amd.noise")
    C, K, offset = 3, 130, 7
    ctrl = ctrl_rows(N)
    ok = [0, 2]
    draws = philox_host.philox_normal(SEED, offset, C * K * N * 3, sigma).reshape(C, K, N, 3)
    for (a, b) in ((0, N - 1), (min(1, N - 1), N // 2)):
        Fw, Gw = gc.grad_eigh(ctrl, draws, N, a, b)
        gc.assert_grad_teeth(Gw, ("independent reference", N, a, b))
        got = fused(be, ctrl, K, N, a, b, offset, sigma=sigma)
        bars = gc.grad_bars(ctrl, draws, N)
        cc.compare(got["fid"], Fw, ("fused", N, a, b, "fid"))
        e = gc.compare_grad(got["grad"], Gw, bars, ("fused", N, a, b, "grad"))
        mw = np.concatenate([Fw.mean(axis=1)[:, None], Gw.mean(axis=1)], axis=1)
        mb = np.concatenate([np.full((C, 1), gc.TOL), bars.max(axis=1)], axis=1)
        gc.compare_grad(got["mean"], mw, mb, ("fused", N, a, b, "mean"))
        nm = noise.structured_perturbation(Nspin=N, inspin=a, outspin=b, noise=sigma)
        m = nm.fidelity_moments_philox(ctrl, K, SEED, offset=offset)
        assert np.array_equal(m["fav"][ok], got["mean"][ok, 0]) and np.array_equal(m["grad_fav"][ok], got["mean"][ok, 1:])
        ev, eg, smin = assert_moments_match(m, Fw, Gw, bars, (N, a, b, sigma))
        print(f"fused gradient kernel, N = {N}, {a} -> {b}, sigma = {sigma}: worst |grad error| {e[0]:.2e} ({e[1]:.2e} of its bar); "
              f"|var error| {ev:.2e}, grad_var error {eg:.2e} of its bound; smallest std {smin:.3f}")


def assert_moments_match(m, Fw, Gw, bars, what, ok=(0, 2)):
    """`fidelity_moments_philox` against the reference's own moments, bounds and teeth as in the docstring of
    test_independent_reference; returns (|var error|, grad_var error / its bound, smallest std)"""
    ok = list(ok)
    var_w, std_w = np.var(Fw[ok], axis=1), np.std(Fw[ok], axis=1)
    gvar_w = 2.0 * ((Fw[ok][..., None] * Gw[ok]).mean(axis=1) - Fw[ok].mean(axis=1)[:, None] * Gw[ok].mean(axis=1))
    gvar_bound = 4.0 * (gc.TOL * np.abs(Gw[ok]).max(axis=1) + bars[ok].max(axis=1))
    assert std_w.min() >= 0.01, (what, std_w)
    assert (np.abs(gvar_w) >= 100.0 * gvar_bound).all(), (what, float((np.abs(gvar_w) / gvar_bound).min()))
    assert all(np.isnan(v[1]).all() for v in m.values())
    ev, eg = np.abs(m["var"][ok] - var_w).max(), (np.abs(m["grad_var"][ok] - gvar_w) / gvar_bound).max()
    assert ev < 4.0 * gc.TOL, (what, "var", ev)
    assert eg < 1.0, (what, "grad_var", eg)
    assert (np.abs(m["grad_std"][ok] * 2.0 * m["std"][ok][:, None] - m["grad_var"][ok]) <= 1e-14 * np.abs(m["grad_var"][ok])).all()
    assert np.abs(m["std"][ok] - std_w).max() < 4.0 * gc.TOL / std_w.min()          # |sqrt u - sqrt v| <= |u - v| / sqrt v
    return float(ev), float(eg), float(std_w.min())


# ---------------------------------------------------------------------------------------------------------------------------
# static Hamiltonian terms, rows of more than 64 tiles, far stream offsets
# ---------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("N", (2, 3, 7, 10, 12))
def test_static_terms_bit_identity(be, N):
    """h0_diag (XXZ) and non-unit h0_offdiag of both signs reach the kernel that generates its draws exactly as they reach the
    two-kernel route: every case of grad_checks.static_cases, every pair, offsets 0 and 7, both draw modes.  (The general-tile
    counter as in test_bit_identity_with_the_two_kernel_route.)"""
    assert gc.PHILOX_SEED == SEED and gc.PHILOX_SIGMA == SIGMA
    be.grad_general_tiles(reset=True)
    gc.check_static_grad_philox(be, N, reference=False)
    tiles = be.grad_general_tiles(reset=True)
    assert (tiles > 0) if FORCED else (tiles == 0), tiles


@pytest.mark.parametrize("N", (5, 10))
def test_static_terms_independent_reference(be, N):
    """the same cases against grad_eigh with the same terms on host-regenerated draws"""
    worst = gc.Worst()
    gc.check_static_grad_philox(be, N, identity=False, worst=worst)
    print(f"static terms, generated draws: {worst}")


@pytest.mark.parametrize("N", (5, 10))
def test_static_terms_through_the_noise_model(be, N):
    """`structured_perturbation` whose HH carries the XXZ diagonal and the non-unit real couplings: `fidelity_moments_philox` gives
    the bits of the backend call with those h0_* and matches the reference's moments (bounds of test_independent_reference); a
    static imaginary coupling is refused.  At the default sigma = 0.05, on the rows of controller seed 9400 + N: on those of
    9300 + N the reference's std of one row (N = 10, 0 -> 9: 0.0098) is under the 0.01 that the moment comparison wants of it; on
    these the smallest is 0.030 (N = 5) and 0.018 (N = 10)."""
    noise = importlib.import_module("code-robchar_amd.noise")
    K, offset, ok, sigma = 130, 7, [0, 2], SIGMA
    ctrl = ctrl_rows(N, seed=9400 + N)
    h0d, h0o = gc.static_terms(N, "both")
    for (a, b) in ((0, N - 1), (min(1, N - 1), N // 2)):
        nm = noise.structured_perturbation(Nspin=N, inspin=a, outspin=b, noise=sigma)
        nm.HH = gc.static_hh(N, "both")
        for shared in (False, True):
            draws, Fw, Gw = gc.reference_on_host_draws(ctrl, K, N, a, b, offset, shared, h0d, h0o, sigma=sigma)
            gc.assert_static_teeth(Fw, gc.grad_eigh(ctrl, draws, N, a, b)[0], ("noise model", N, a, b))
            m = nm.fidelity_moments_philox(ctrl, K, SEED, offset=offset, shared=shared)
            got = fused(be, ctrl, K, N, a, b, offset, shared=shared, sigma=sigma, want=("mean", "moment"), h0_diag=h0d, h0_offdiag=h0o)
            assert np.array_equal(m["fav"][ok], got["mean"][ok, 0]) and np.array_equal(m["grad_fav"][ok], got["mean"][ok, 1:])
            want = noise.moments_from_sums(got["mean"], got["moment"])
            assert all(np.array_equal(m[k], want[k], equal_nan=True) for k in want)
            bars = gc.grad_bars(ctrl, draws, N, h0d, h0o)
            ev, eg, smin = assert_moments_match(m, Fw, Gw, bars, ("noise model", N, a, b, shared))
            print(f"noise model with static terms, N = {N}, {a} -> {b}, shared = {shared}: |var error| {ev:.2e} (bound {4 * gc.TOL:.1e}), "
                  f"grad_var error {eg:.2e} of its bound; smallest std {smin:.3f}")
        nm.HH[1, 0] += 0.1j
        nm.HH[0, 1] -= 0.1j
        with pytest.raises(NotImplementedError, match="real static couplings"):
            nm.fidelity_moments_philox(ctrl, K, SEED, offset=offset)


@pytest.mark.parametrize("K", (4096, 4097, 8193))
@pytest.mark.parametrize("N", (7, 11))
def test_long_rows(be, N, K):
    """64, 65 and 129 tiles per row: the strided loop of the row-mean kernel takes one, two and three steps (one and three QL
    passes in the gradient kernel)"""
    gc.check_long_rows_grad_philox(be, N, K, report=print)


def test_long_rows_moments_against_the_reference(be):
    """N = 5, K = 4097 (65 tiles): `fidelity_moments_philox` against the reference's own moments, bounds and teeth of
    test_independent_reference"""
    noise = importlib.import_module("code-robchar_amd.noise")
    N, K, offset = 5, 4097, 7
    ctrl = ctrl_rows(N)
    for (a, b) in ((0, N - 1), (min(1, N - 1), N // 2)):
        draws, Fw, Gw = gc.reference_on_host_draws(ctrl, K, N, a, b, offset, False)
        gc.assert_grad_teeth(Gw, ("long rows, reference", N, a, b))
        nm = noise.structured_perturbation(Nspin=N, inspin=a, outspin=b, noise=SIGMA)
        m = nm.fidelity_moments_philox(ctrl, K, SEED, offset=offset)
        ev, eg, smin = assert_moments_match(m, Fw, Gw, gc.grad_bars(ctrl, draws, N), ("long rows", N, a, b))
        print(f"moments over 65 tiles, N = {N}, {a} -> {b}: |var error| {ev:.2e} (bound {4 * gc.TOL:.1e}), grad_var error {eg:.2e} of "
              f"its bound; smallest std {smin:.3f}")


@pytest.mark.parametrize("N", (7, 11))
def test_far_offsets(be, N):
    """the pair counter's low word wraps inside the first tile (offset 2^33 - 32 * 3 N - 1), and a counter with a non-zero high
    word from the start"""
    worst = gc.Worst()
    gc.check_far_offsets_grad_philox(be, N, worst=worst)
    print(f"far stream offsets, generated draws: {worst}")


def test_unsupported_and_rejected(be):
    import torch
    lib = importlib.import_module("code-robchar_amd._lib")
    dev = be.compute_device()
    with pytest.raises(lib.RobCharHipError, match="N <= 12"):
        be.mc_fidelity_grad_philox(torch.zeros((1, 14), dtype=torch.float64, device=dev), 4, 13, 0, 12, seed=1)
    with pytest.raises(lib.RobCharHipError, match="sigma"):
        be.mc_fidelity_grad_philox(torch.zeros((1, 6), dtype=torch.float64, device=dev), 4, 5, 0, 4, seed=1, sigma=-0.1)


def test_robust_lbfgs_with_generated_draws(be, monkeypatch):
    """scripts/robust_lbfgs.py with draws="philox", risk = 1: 1 - fav + std over 256 common random numbers never increases
    between accepted iterates and ends below the start; one launch of the entry per evaluation; the same seed reproduces the
    trace bit for bit."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        robust_lbfgs = importlib.import_module("robust_lbfgs")
    finally:
        sys.path.pop(0)
    calls = []
    entry = be.mc_fidelity_grad_philox

    def counted(*args, **kwargs):
        calls.append((int(args[1]), kwargs.get("shared"), kwargs.get("offset"), tuple(kwargs.get("want"))))
        return entry(*args, **kwargs)

    monkeypatch.setattr(be, "mc_fidelity_grad_philox", counted)
    out = robust_lbfgs.run(draws="philox", risk=1.0, train=256, maxiter=8, verbose=False)
    vals = [out["start"]] + [t[0] for t in out["trace"]]
    assert 1 <= len(out["trace"]) <= 8
    assert all(b <= a for a, b in zip(vals, vals[1:])), vals
    assert out["final"] < out["start"]
    # one launch per evaluation (256 shared draws from offset 0, row sums only) + the test figure (10 000 draws behind them)
    assert len(calls) == out["launches"] + 1
    assert all(c == (256, True, 0, ("mean", "moment")) for c in calls[:-1]) and calls[-1] == (10000, True, 256 * 7 * 3, ("mean", "moment"))
    assert np.isfinite(out["test_final"]) and out["test_std"] > 0.0
    print(f"robust_lbfgs, generated draws: 1 - F + std {out['start']:.6f} -> {out['final']:.6f} in {len(out['trace'])} iterations, "
          f"{out['launches']} launches; test {out['test_final']:.6f}")
    again = robust_lbfgs.run(draws="philox", risk=1.0, train=256, maxiter=8, verbose=False)
    assert again["trace"] == out["trace"] and np.array_equal(again["x"], out["x"]) and again["final"] == out["final"]
