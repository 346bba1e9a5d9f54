"""The references and checks of tests/chain_checks.py, without a GPU: the closed form against the oracle and against
30-digit arithmetic; every data-level GPU check passes on the oracle stand-in (tests/stand_in.py) and FAILS on stand-ins
broken the ways a kernel could be subtly wrong."""
import numpy as np
import pytest

import chain_checks as cc
import stand_in
from gpu_common import rand_ctrl
from oracle import robchar_oracle as orc


@pytest.mark.parametrize("N", list(range(2, 33)))
def test_closed_form_equals_the_oracle(N):
    ctrl = cc.closed_form_ctrl(N, (0.05, -0.3, 0.0, 1.7), np.linspace(0.0, 7.0, 15))
    off = cc.closed_form_offdiag(N)
    draws = np.zeros((ctrl.shape[0], 1, N, 3))
    worst = 0.0
    for a in (0, N - 1):
        for b in range(N):
            want = orc.fidelity_eigh(ctrl, draws, N, a, b, h0_offdiag=off)[:, 0]
            worst = max(worst, np.abs(cc.closed_form_fid(N, ctrl, a, b) - want).max())
    assert worst < 1e-13, worst
    with pytest.raises(ValueError):
        cc.closed_form_fid(N, ctrl, N, 0)


@pytest.mark.parametrize("N", [2, 7, 17, 32])
def test_closed_form_equals_30_digit_arithmetic(N):
    """An eigendecomposition in 30-digit arithmetic (mpmath) of the closed-form chain, independent of LAPACK."""
    mpmath = pytest.importorskip("mpmath")
    with mpmath.workdps(30):
        for g in (0.05, -0.3):
            off = cc.closed_form_offdiag(N)
            H = mpmath.matrix(N, N)
            for n in range(N):
                H[n, n] = mpmath.mpf(g) * (mpmath.mpf(N - 1) / 2 - n)
            for n in range(1, N):
                H[n - 1, n] = H[n, n - 1] = mpmath.mpf(0.5) * mpmath.sqrt(mpmath.mpf(n * (N - n)))
                assert abs(float(H[n, n - 1]) - off[n - 1]) < 1e-15
            lam, V = mpmath.eigsy(H)
            Ts = (0.0, 0.4, 1.3, 3.1)
            ctrl = cc.closed_form_ctrl(N, g, Ts)
            for a in (0, N - 1):
                for b in range(0, N, max(1, N // 6)):
                    want = []
                    for T in Ts:
                        phi = mpmath.fsum(V[b, k] * V[a, k] * mpmath.expjpi(-mpmath.mpf(T) * lam[k] / mpmath.pi) for k in range(N))
                        want.append(float(abs(phi) ** 2))
                    assert np.abs(cc.closed_form_fid(N, ctrl, a, b) - np.array(want)).max() < 1e-14, (N, g, a, b)


def test_teeth_guard_rejects_localised_long_chains():
    """The inputs the long-chain GPU test used alone until now (`rand_ctrl`, biases U(-10, 10)): end to end at N = 24 the
    fidelities are ~1e-21 - zeros would pass an absolute 1e-10 - and the guard says so; delocalised rows pass it."""
    rng = np.random.default_rng(7024)
    N = 24
    draws = 0.05 * rng.standard_normal((4, 150, N, 3))
    want = orc.fidelity_eigh(rand_ctrl(rng, 4, N), draws, N, 0, N - 1)
    with pytest.raises(AssertionError):
        cc.assert_has_teeth(want)
    cc.assert_has_teeth(orc.fidelity_eigh(cc.deloc_ctrl(rng, 4, N, 0.5), draws, N, 0, N - 1))
    cc.compare(want, want, "self")
    with pytest.raises(AssertionError):
        cc.compare(want, np.where(np.arange(150) == 7, np.nan, want), "NaN pattern")


# ------------------------------------------------------------------------------------------------------------------------
# the checks can fail
# ------------------------------------------------------------------------------------------------------------------------


class _Mutant:
    """The oracle stand-in, broken in one way: `kind` in MUTANTS."""

    def __init__(self, kind):
        self.kind = kind

    @staticmethod
    def compute_device():
        return stand_in.compute_device()

    def mc_fidelity(self, controllers, draws, nspin, inspin, outspin, h0_diag=None, h0_offdiag=None, **kw):
        is_torch = type(draws).__module__.startswith("torch")
        c = controllers.cpu().numpy() if type(controllers).__module__.startswith("torch") else np.asarray(controllers)
        d = draws.cpu().numpy() if is_torch else np.asarray(draws)
        c, d = np.array(c, dtype=np.float64), np.array(np.broadcast_to(d, (c.shape[0],) + d.shape[1:]), dtype=np.float64)
        K = d.shape[1]
        if self.kind == "t_fp32":
            c[:, nspin] = c[:, nspin].astype(np.float32)
        elif self.kind == "offdiag_ignored":
            h0_offdiag = None
        elif self.kind == "ragged_lane" and K % 64 and K > 1:
            d[:, K - 1] = d[:, K - 2]                  # the last lane of the ragged tile reads its neighbour's draws
        res = stand_in.mc_fidelity(c, d, nspin, inspin, outspin, h0_diag=h0_diag, h0_offdiag=h0_offdiag)
        if self.kind == "zeros":
            res = np.where(np.isnan(res), np.nan, 0.0)
        elif self.kind == "rel_1e-7":
            res = res * (1.0 + 1e-7)
        if is_torch:
            import torch
            return torch.from_numpy(np.ascontiguousarray(res))
        return res


MUTANTS = ("zeros", "rel_1e-7", "t_fp32", "offdiag_ignored", "ragged_lane")

CHECKS = {
    "long_chain_N17": (lambda be: cc.check_long_chain(be, 17), ("zeros", "rel_1e-7", "t_fp32", "ragged_lane")),
    "long_chain_N25": (lambda be: cc.check_long_chain(be, 25), ("zeros", "rel_1e-7", "t_fp32", "ragged_lane")),
    "closed_form_N5": (lambda be: cc.check_closed_form(be, 5), ("zeros", "rel_1e-7", "t_fp32", "offdiag_ignored")),
    "closed_form_N20": (lambda be: cc.check_closed_form(be, 20), ("zeros", "rel_1e-7", "t_fp32", "offdiag_ignored")),
    "deloc_N9": (lambda be: cc.check_deloc_vs_oracle(be, 9), ("zeros", "rel_1e-7", "t_fp32", "ragged_lane")),
    "random_deloc_seed0": (lambda be: cc.check_random_deloc_configs(be, 0), ("zeros", "rel_1e-7", "t_fp32", "ragged_lane")),
}


@pytest.mark.parametrize("check", sorted(CHECKS))
def test_check_passes_on_the_oracle(check):
    CHECKS[check][0](stand_in)


@pytest.mark.parametrize("check,mutant", [(c, m) for c in sorted(CHECKS) for m in CHECKS[c][1]])
def test_check_catches_the_mutant(check, mutant):
    with pytest.raises(AssertionError):
        CHECKS[check][0](_Mutant(mutant))
    print(f"{check}: mutant {mutant} caught")


def test_every_mutant_is_caught_somewhere():
    assert {m for c in CHECKS.values() for m in c[1]} == set(MUTANTS)
