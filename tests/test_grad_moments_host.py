"""`noise.moments_from_sums` and `noise_model_base.fidelity_moments_philox` without a GPU.  Reference: grad_checks.grad_eigh on
delocalised rows with draws from oracle/philox_host.py; the gradients of Var F and std F are compared with central differences
(h = 1e-5) of np.var / np.std of the reference fidelities.  Tolerance 1e-9: the finite-difference floor of this reference is
2.0e-12 for Var and 3.7e-11 for std (measured on these inputs; truncation h^2 f''' / 6 plus 1e-16 / h of rounding), so the bound
is 25 x above the reference's own error and 1e7 below the signal (|grad std| up to 0.085).  The same check must FAIL on two
broken stand-ins of the formula.  `fidelity_moments_philox` runs around a NumPy stand-in of `backend.mc_fidelity_grad_philox`
that regenerates the stream elements the entry documents."""
import importlib

import numpy as np
import pytest

import chain_checks as cc
import grad_checks as gc
from oracle import philox_host

noise = importlib.import_module("code-robchar_amd.noise")
be = importlib.import_module("code-robchar_amd.backend")

SEED, OFFSET, SIGMA, C, K, H, TOL = 0x5EED000A, 7, 0.05, 3, 130, 1e-5, 1e-9
SIZES = (3, 5, 7, 10)
_cache = {}


def reference(N):
    """(ctrl, draws, F, G, central differences of np.var and np.std) - computed once per N, never modified"""
    if N not in _cache:
        ctrl = cc.deloc_ctrl(np.random.default_rng(9300 + N), C, N, 0.5)
        draws = philox_host.philox_normal(SEED, OFFSET, C * K * N * 3, SIGMA).reshape(C, K, N, 3)
        a, b = 0, N - 1
        F, G = gc.grad_eigh(ctrl, draws, N, a, b)
        dvar, dstd = np.empty((C, N + 1)), np.empty((C, N + 1))
        for l in range(N + 1):
            p, m = ctrl.copy(), ctrl.copy()
            p[:, l] += H
            m[:, l] -= H
            Fp, Fm = gc.grad_eigh(p, draws, N, a, b)[0], gc.grad_eigh(m, draws, N, a, b)[0]
            dvar[:, l] = (np.var(Fp, axis=1) - np.var(Fm, axis=1)) / (2 * H)
            dstd[:, l] = (np.std(Fp, axis=1) - np.std(Fm, axis=1)) / (2 * H)
        for v in (ctrl, draws, F, G, dvar, dstd):
            v.setflags(write=False)
        _cache[N] = (ctrl, draws, F, G, dvar, dstd)
    return _cache[N]


def sums(F, G):
    mean = np.concatenate([F.mean(axis=1)[:, None], G.mean(axis=1)], axis=1)
    moment = np.concatenate([(F * F).mean(axis=1)[:, None], (F[..., None] * G).mean(axis=1)], axis=1)
    return mean, moment


def check(moments, N):
    ctrl, draws, F, G, dvar, dstd = reference(N)
    m = moments(*sums(F, G))
    assert np.abs(dstd).max() > 1e-2 and np.abs(dvar).max() > 1e-3, "the reference has no teeth"
    ev, es = float(np.abs(m["grad_var"] - dvar).max()), float(np.abs(m["grad_std"] - dstd).max())
    print(f"N = {N}: grad Var vs central differences {ev:.2e}, grad std {es:.2e} (largest |grad std| {np.abs(dstd).max():.3f})")
    assert ev < TOL and es < TOL, (N, ev, es)
    assert np.abs(m["var"] - np.var(F, axis=1)).max() < 1e-15 and np.abs(m["std"] - np.std(F, axis=1)).max() < 1e-14
    assert np.array_equal(m["fav"], F.mean(axis=1)) and np.array_equal(m["grad_fav"], G.mean(axis=1))


def no_cross_term(mean, moment):
    m = dict(noise.moments_from_sums(mean, moment))
    m["grad_var"] = 2.0 * moment[:, 1:]
    m["grad_std"] = m["grad_var"] / (2.0 * m["std"])[:, None]
    return m


def no_factor_two(mean, moment):
    m = dict(noise.moments_from_sums(mean, moment))
    m["grad_var"] = moment[:, 1:] - mean[:, :1] * mean[:, 1:]
    m["grad_std"] = m["grad_var"] / (2.0 * m["std"])[:, None]
    return m


@pytest.mark.parametrize("N", SIZES)
def test_against_central_differences(N):
    check(noise.moments_from_sums, N)


@pytest.mark.parametrize("broken", (no_cross_term, no_factor_two))
@pytest.mark.parametrize("N", SIZES)
def test_the_check_fails_on_broken_formulas(N, broken):
    with pytest.raises(AssertionError):
        check(broken, N)


def test_zero_variance_convention():
    """K identical samples (a sigma = 0 row): var = std = 0 and grad_std = 0 exactly, nothing NaN; sums that differ by rounding
    only land there too; a NaN row stays NaN; torch tensors give the same numbers"""
    import torch
    F = np.full((2, K), 0.7312345678901234)
    G = np.broadcast_to(np.array([0.3, -0.2, 0.05, 1.1]), (2, K, 4)).copy()
    mean, moment = sums(F, G)
    moment[1] *= 1.0 + 8 * 2.0 ** -52                        # rounding-level disagreement of the two sums
    m = noise.moments_from_sums(mean, moment)
    for k in ("var", "std", "grad_std"):
        assert (m[k] == 0.0).all() and not np.isnan(m[k]).any(), k
    assert not np.isnan(m["grad_var"]).any() and np.abs(m["grad_var"]).max() < 1e-13
    assert np.array_equal(m["fav"], mean[:, 0])
    nan = noise.moments_from_sums(np.full((1, 5), np.nan), np.full((1, 5), np.nan))
    assert all(np.isnan(v).all() for v in nan.values())
    ctrl, draws, Fr, Gr, _, _ = reference(5)
    mean, moment = sums(Fr, Gr)
    want = noise.moments_from_sums(mean, moment)
    got = noise.moments_from_sums(torch.from_numpy(mean), torch.from_numpy(moment))
    assert all(isinstance(got[k], torch.Tensor) and np.array_equal(got[k].numpy(), want[k]) for k in want)
    assert (want["std"] > 0.01).all()


class StandIn:
    """`backend.mc_fidelity_grad_philox` on the CPU (host-regenerated stream elements, eigh formulas); records its calls"""

    def __init__(self):
        self.calls = []

    def __call__(self, controllers, n_draws, nspin, inspin, outspin, seed, offset=0, sigma=0.05, shared=False, h0_diag=None,
                 h0_offdiag=None, want=("fid", "grad", "mean", "moment")):
        ctrl = np.asarray(controllers, dtype=np.float64)
        rows = ctrl.shape[0]
        sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (rows,))
        self.calls.append(dict(rows=rows, K=n_draws, seed=seed, offset=offset, sigma=sig.copy(), shared=shared, want=tuple(want)))
        sets = 1 if shared else rows
        z = philox_host.philox_normal(seed, offset, sets * n_draws * nspin * 3, 1.0).reshape(sets, n_draws, nspin, 3)
        draws = sig[:, None, None, None] * np.broadcast_to(z, (rows, n_draws, nspin, 3))
        F, G = gc.grad_eigh(ctrl, draws, nspin, inspin, outspin, h0_diag, h0_offdiag)
        mean, moment = sums(F, G)
        res = {"fid": F, "grad": G, "mean": mean, "moment": moment}
        return {k: res[k] for k in want}


def test_fidelity_moments_philox_around_a_stand_in(monkeypatch):
    stand = StandIn()
    monkeypatch.setattr(be, "mc_fidelity_grad_philox", stand)
    N = 5
    ctrl, draws, F, G, dvar, dstd = reference(N)
    nm = noise.structured_perturbation(Nspin=N, inspin=0, outspin=N - 1, noise=SIGMA)
    m = nm.fidelity_moments_philox(ctrl, K, SEED, offset=OFFSET)                      # sigma = None: the model's level
    call = stand.calls[-1]
    assert call["want"] == ("mean", "moment") and call["shared"] is False and call["offset"] == OFFSET and call["K"] == K
    assert (call["sigma"] == SIGMA).all() and len(stand.calls) == 1
    assert set(m) == {"fav", "grad_fav", "var", "grad_var", "std", "grad_std"}
    assert np.abs(m["grad_std"] - dstd).max() < TOL and np.abs(m["grad_var"] - dvar).max() < TOL
    assert np.abs(m["fav"] - F.mean(axis=1)).max() < 1e-12 and np.abs(m["std"] - np.std(F, axis=1)).max() < 1e-12
    # shared draws: every row sees row 0's elements; per-row sigma reaches the entry; a sigma = 0 row reports exact zeros
    s = nm.fidelity_moments_philox(ctrl, K, SEED, sigma=np.array([0.0, 0.05, 0.1]), offset=OFFSET, shared=True)
    call = stand.calls[-1]
    assert call["shared"] is True and np.array_equal(call["sigma"], [0.0, 0.05, 0.1])
    assert s["var"][0] == 0.0 and s["std"][0] == 0.0 and (s["grad_std"][0] == 0.0).all() and not np.isnan(s["grad_var"]).any()
    Fs, Gs = gc.grad_eigh(ctrl[1:2], draws[:1], N, 0, N - 1)
    assert np.abs(s["std"][1] - np.std(Fs)).max() < 1e-12 and s["std"][2] > s["std"][1] > 0.0
    # the model's static diagonal is handed on; rings and complex couplings are refused before the entry is reached
    nm.HH[np.arange(N), np.arange(N)] = 0.1 * np.arange(N)
    x = nm.fidelity_moments_philox(ctrl, K, SEED, offset=OFFSET)
    Fx, _ = gc.grad_eigh(ctrl, draws, N, 0, N - 1, h0_diag=0.1 * np.arange(N))
    assert np.abs(x["fav"] - Fx.mean(axis=1)).max() < 1e-12 and np.abs(x["fav"] - m["fav"]).max() > 1e-4
    ncalls = len(stand.calls)
    with pytest.raises(NotImplementedError):
        noise.structured_perturbation(Nspin=N, inspin=0, outspin=N - 1, topo="ring").fidelity_moments_philox(ctrl, K, SEED)
    assert len(stand.calls) == ncalls
