"""The references and checks of tests/ring_checks.py, without a GPU: the closed forms against the oracle and against 30-digit
arithmetic; the teeth guard against the inputs the ring and directional GPU tests used alone until now; every data-level GPU
check passes on the oracle stand-in (tests/stand_in.py) and FAILS on stand-ins broken the ways a kernel could be subtly wrong;
the product surface (`structured_perturbation` with an edited `HH`) on the stand-in."""
import numpy as np
import pytest

import chain_checks as cc
import ring_checks as rc
import stand_in
from gpu_common import rand_ctrl
from oracle import robchar_oracle as orc


@pytest.mark.parametrize("N", list(range(3, 17)))
def test_flux_ring_equals_the_oracle(N):
    worst = 0.0
    for phi in (np.pi / 2, 0.0, 1.0, -2.5):
        ctrl, off, draws = rc.flux_ring(N, phi, K=1, seed=N)
        for a in (0, N - 1, N // 2):
            for b in range(N):
                want = orc.fidelity_eigh(ctrl, draws, N, a, b, h0_offdiag=off, ring=True)[:, 0]
                worst = max(worst, np.abs(rc.flux_ring_fid(N, phi, ctrl[:, N], a, b) - want).max())
    assert worst < 1e-13, worst
    if N % 2:                                          # odd N: the sign of the flux shows (the ring is not bipartite)
        ctrl, off, draws = rc.flux_ring(N, np.pi / 2, K=1, seed=N)
        flipped = max(np.abs(rc.flux_ring_fid(N, -np.pi / 2, ctrl[:, N], 0, b)
                             - orc.fidelity_eigh(ctrl, draws, N, 0, b, h0_offdiag=off, ring=True)[:, 0]).max() for b in range(N))
        assert flipped > 1e-3, flipped


@pytest.mark.parametrize("N", list(range(3, 17)))
def test_cut_ring_equals_the_oracle(N):
    worst = 0.0
    for cut, phases in rc.CUT_VARIANTS + (("draw", False),):
        ctrl, off, draws, pos_ctrl, k, lam = rc.cut_ring(N, cut, phases, seed=N)
        for ap in (0, N - 1):
            for bp in range(N):
                want = orc.fidelity_eigh(ctrl, draws, N, (k + ap) % N, (k + bp) % N, h0_offdiag=off, ring=True)
                worst = max(worst, np.abs(rc.closed_form_fid(N, pos_ctrl, ap, bp, lam=lam)[:, None] - want).max())
    assert worst < 1e-13, worst


@pytest.mark.parametrize("N", list(range(2, 17)))
def test_complex_field_chain_equals_the_oracle(N):
    """normwise: |closed form - expm| <= 2e-12 max(1, max_out F) per row, F up to ~1e18 at Im g = 1.2"""
    ctrl, off, draws, imag, g = rc.complex_field_chain(N)
    worst = 0.0
    for a in (0, N - 1):
        cfs = np.array([rc.complex_field_fid(N, g, ctrl[:, N], a, b) for b in range(N)])
        scale = np.maximum(1.0, cfs.max(axis=0))
        for b in range(N):
            want = orc.fidelity_expm_loop(ctrl, draws, N, a, b, h0_offdiag=off, diag_imag=imag)[:, 0]
            worst = max(worst, (np.abs(cfs[b] - want) / scale).max())
    assert worst < 2e-12, worst
    if N > 2:                                          # an imaginary field breaks the mirror symmetry: F(0 -> n) != F(N-1 -> N-1-n)
        mirror = np.abs(rc.complex_field_fid(N, g, ctrl[:, N], 0, 1) - rc.complex_field_fid(N, g, ctrl[:, N], N - 1, N - 2))
        assert mirror[g.imag != 0].max() > 1e-3
    with pytest.raises(ValueError):
        rc.complex_field_fid(N, g, ctrl[:, N], N, 0)


@pytest.mark.parametrize("N", [3, 6, 11, 16])
def test_flux_ring_with_imaginary_diagonal_equals_the_oracle(N):
    ctrl, off, draws = rc.flux_ring(N, np.pi / 2, K=1, seed=N)
    for gamma in (0.07, -0.05):
        imag = np.full(draws.shape[:3], gamma)
        for (a, b) in ((0, N // 2), (N - 1, 1), (0, 0)):
            want = orc.fidelity_expm_loop(ctrl, draws, N, a, b, h0_offdiag=off, ring=True, diag_imag=imag)[:, 0]
            cf = np.exp(2 * gamma * np.abs(ctrl[:, N])) * rc.flux_ring_fid(N, np.pi / 2, ctrl[:, N], a, b)
            assert np.abs(cf - want).max() < 1e-13 * max(1.0, cf.max()), (N, gamma, a, b)


@pytest.mark.parametrize("N", [2, 3, 8, 12])
def test_directional_gauge_samples_equal_the_closed_form(N):
    ctrl, off, idx, ab, K = rc.directional_gauge(N, seed=N)
    assert set(idx.tolist()) == set(range(len(orc.directional_directions(N))))
    draws, imag = rc.directional_layout(N, idx, ab, ctrl.shape[0], K)
    assert not imag.any()
    for (a, b) in ((0, N - 1), (N - 1, N // 2), (0, 0)):
        want = orc.fidelity_expm_loop(ctrl, draws, N, a, b, h0_offdiag=off, diag_imag=imag)
        assert np.abs(cc.closed_form_fid(N, ctrl, a, b)[:, None] - want).max() < 1e-13, (N, a, b)


def test_ring_and_complex_field_equal_30_digit_arithmetic():
    """Dense matrix exponentials in 30-digit arithmetic (mpmath), independent of LAPACK and scipy: A (odd and even N, both
    signs of the flux) and C (a generic complex field, and the Jordan block at g = i)."""
    mpmath = pytest.importorskip("mpmath")
    with mpmath.workdps(30):
        for N in (5, 6):
            phi = mpmath.pi / 2
            H = mpmath.matrix(N, N)
            for i in range(1, N):
                H[i, i - 1] = mpmath.expj(phi / (N - 1))
                H[i - 1, i] = mpmath.expj(-phi / (N - 1))
            H[N - 1, 0] = H[0, N - 1] = 1
            for T in (0.4, 1.7, 2.9):
                U = mpmath.expm(-1j * mpmath.mpf(T) * H)
                for (a, b) in ((0, N // 2), (N - 1, 1), (1, 1)):
                    want = float(abs(U[b, a]) ** 2)
                    assert abs(rc.flux_ring_fid(N, np.pi / 2, np.array([T]), a, b)[0] - want) < 1e-14, (N, T, a, b)
        for N, g in ((4, 0.3 + 0.2j), (7, 1j), (5, 1.2j)):
            off = cc.closed_form_offdiag(N)
            H = mpmath.matrix(N, N)
            for n in range(N):
                H[n, n] = mpmath.mpc(g.real, g.imag) * (mpmath.mpf(N - 1) / 2 - n)
            for n in range(1, N):
                H[n - 1, n] = H[n, n - 1] = mpmath.sqrt(mpmath.mpf(n * (N - n))) / 2
                assert abs(float(H[n, n - 1].real) - off[n - 1]) < 1e-15
            for T in (0.5, 2.0, np.pi):
                U = mpmath.expm(-1j * mpmath.mpf(T) * H)
                for a in (0, N - 1):
                    for b in range(N):
                        want = float(abs(U[b, a]) ** 2)
                        got = rc.complex_field_fid(N, np.array([g]), np.array([T]), a, b)[0]
                        assert abs(got - want) <= 1e-13 * max(1.0, want), (N, g, T, a, b, got, want)


def test_teeth_guard_rejects_the_localised_ring_and_directional_inputs():
    """The inputs `test_ring_kernels_vs_oracle` and `test_directional_entry_vs_oracle` used alone until now (`rand_ctrl`,
    biases U(-10, 10)): the far ring pairs and the directional end-to-end pair are ~1e-9 ... 1e-5 - zeros would pass an
    absolute 1e-10 - and the guard says so; the delocalised rows of ring_checks pass it."""
    for N in (8, 13, 16):
        rng = np.random.default_rng(300 + N)
        draws = 0.05 * rng.standard_normal((6, 131, N, 3))
        with pytest.raises(AssertionError):
            cc.assert_has_teeth(orc.fidelity_eigh(rand_ctrl(rng, 6, N), draws, N, 0, N // 2, ring=True))
        cc.assert_has_teeth(orc.fidelity_eigh(rc.deloc_ring_ctrl(rng, 6, N, 0.5), draws, N, 0, N // 2, ring=True))
    for N in (8, 12):
        rng = np.random.default_rng(600 + N)
        draws = 0.05 * rng.standard_normal((5, 50, N, 3))
        with pytest.raises(AssertionError):
            cc.assert_has_teeth(orc.fidelity_eigh(rand_ctrl(rng, 5, N), draws, N, 0, N - 1))


def test_compare_nh_bounds():
    want = np.array([[1e6, 5e3, 1e-5], [0.5, np.nan, 0.2]])
    scale = np.array([[1e6], [1.0]])
    rows = np.array([True, True])
    rc.compare_nh(want, want, scale, 1e-9, rows, "self")
    bump = np.array([[0, 1e-4, 0], [0, 0, 0]])          # 1e-10 of the row's scale 1e6, but 2e-8 relative to F = 5e3
    with pytest.raises(AssertionError):
        rc.compare_nh(want + bump, want, scale, 1e-9, rows, "rel")
    rc.compare_nh(want + bump, want, scale, 1e-9, np.array([False, True]), "rel off")
    with pytest.raises(AssertionError):
        rc.compare_nh(want + [[0, 0, 0], [2e-9, 0, 0]], want, scale, 1e-9, np.array([False, False]), "abs")
    with pytest.raises(AssertionError):
        rc.compare_nh(np.nan_to_num(want), want, scale, 1e-9, rows, "NaN pattern")


# ------------------------------------------------------------------------------------------------------------------------
# the checks can fail
# ------------------------------------------------------------------------------------------------------------------------


def _np(x):
    return x.cpu().numpy() if type(x).__module__.startswith("torch") else np.asarray(x)


def _out(res, like):
    if type(like).__module__.startswith("torch"):
        import torch
        return torch.from_numpy(np.ascontiguousarray(res))
    return res


class _Mutant:
    """The oracle stand-in, broken in one way: `kind` in MUTANTS."""

    def __init__(self, kind):
        self.kind = kind

    @staticmethod
    def compute_device():
        return stand_in.compute_device()

    def _inputs(self, controllers, draws, nspin, inspin, outspin, h0_offdiag, ring):
        c = np.array(_np(controllers), dtype=np.float64)
        d = _np(draws)
        d = np.array(np.broadcast_to(d, (c.shape[0],) + d.shape[1:]), dtype=np.float64)
        K = d.shape[1]
        if self.kind == "t_fp32":
            c[:, nspin] = c[:, nspin].astype(np.float32)
        elif self.kind == "offdiag_ignored":
            h0_offdiag = None
        elif self.kind == "corner_dropped":
            ring = False
        elif self.kind == "conjugated":
            d[..., 2] = -d[..., 2]
        elif self.kind == "in_out_swapped":
            inspin, outspin = outspin, inspin
        elif self.kind == "ragged_lane" and K % 64 and K > 1:
            d[:, K - 1] = d[:, K - 2]                  # the last lane of the ragged tile reads its neighbour's draws
        return c, d, inspin, outspin, h0_offdiag, ring

    def _result(self, res):
        if self.kind == "zeros":
            return np.where(np.isnan(res), np.nan, 0.0)
        if self.kind == "rel_1e-7":
            return res * (1.0 + 1e-7)
        return res

    def mc_fidelity(self, controllers, draws, nspin, inspin, outspin, h0_diag=None, h0_offdiag=None, ring=False, **kw):
        c, d, a, b, off, ring = self._inputs(controllers, draws, nspin, inspin, outspin, h0_offdiag, ring)
        res = stand_in.mc_fidelity(c, d, nspin, a, b, h0_diag=h0_diag, h0_offdiag=off, ring=ring)
        return _out(self._result(res), draws)

    def mc_fidelity_nonhermitian(self, controllers, draws, diag_imag, nspin, inspin, outspin, h0_diag=None, h0_offdiag=None,
                                 ring=False, **kw):
        c, d, a, b, off, ring = self._inputs(controllers, draws, nspin, inspin, outspin, h0_offdiag, ring)
        imag = np.array(_np(diag_imag), dtype=np.float64)
        if self.kind == "imag_sign_flipped":
            imag = -imag
        elif self.kind == "imag_dropped":
            imag = None
        elif self.kind == "ragged_lane" and d.shape[1] % 64 and d.shape[1] > 1:
            imag[:, -1] = imag[:, -2]
        res = stand_in.mc_fidelity_nonhermitian(c, d, imag, nspin, a, b, h0_diag=h0_diag, h0_offdiag=off, ring=ring)
        return _out(self._result(res), draws)

    def mc_fidelity_directional(self, controllers, idx, ab, nspin, inspin, outspin, n_draws, h0_diag=None, h0_offdiag=None):
        c, i, g = np.array(_np(controllers)), _np(idx), _np(ab)
        C, K = c.shape[0], int(n_draws)
        draws, imag = rc.directional_layout(nspin, i, g, C, K)
        if self.kind == "diag_direction_a_plus_ib":
            imag = -imag                               # z[p, p] = a + ib kept instead of the reference's last write a - ib
        elif self.kind == "ragged_lane" and K % 64 and K > 1:
            draws[:, K - 1], imag[:, K - 1] = draws[:, K - 2], imag[:, K - 2]
        c, draws, a, b, off, _ = self._inputs(c, draws, nspin, inspin, outspin, h0_offdiag, False)
        res = stand_in.mc_fidelity_nonhermitian(c, draws, imag, nspin, a, b, h0_diag=h0_diag, h0_offdiag=off)
        return _out(self._result(res), idx)


MUTANTS = ("zeros", "rel_1e-7", "t_fp32", "offdiag_ignored", "corner_dropped", "conjugated", "in_out_swapped",
           "imag_sign_flipped", "imag_dropped", "diag_direction_a_plus_ib", "ragged_lane")

_BASIC = ("zeros", "rel_1e-7", "t_fp32")
CHECKS = {
    # odd N: the flux has a sign; even N: it has none (a conjugated coupling or a swap passes there, by symmetry)
    "flux_ring_N5": (lambda be: rc.check_flux_ring(be, 5),
                     _BASIC + ("offdiag_ignored", "corner_dropped", "conjugated", "in_out_swapped")),
    "flux_ring_N16": (lambda be: rc.check_flux_ring(be, 16), _BASIC + ("offdiag_ignored", "corner_dropped")),
    "cut_ring_N7": (lambda be: rc.check_cut_ring(be, 7), _BASIC + ("offdiag_ignored", "corner_dropped")),
    "ring_deloc_N6": (lambda be: rc.check_ring_deloc(be, 6),
                      _BASIC + ("corner_dropped", "conjugated", "in_out_swapped", "ragged_lane")),
    "ring_deloc_N13": (lambda be: rc.check_ring_deloc(be, 13),
                       _BASIC + ("corner_dropped", "conjugated", "in_out_swapped", "ragged_lane")),
    "complex_field_N6": (lambda be: rc.check_complex_field(be, 6),
                         _BASIC + ("offdiag_ignored", "imag_sign_flipped", "imag_dropped")),
    "flux_ring_nh_N5": (lambda be: rc.check_flux_ring_nh(be, 5),
                        _BASIC + ("offdiag_ignored", "corner_dropped", "conjugated", "in_out_swapped", "imag_sign_flipped",
                                  "imag_dropped")),
    "directional_gauge_N6": (lambda be: rc.check_directional_gauge(be, 6), _BASIC + ("offdiag_ignored",)),
    "directional_deloc_N6": (lambda be: rc.check_directional_deloc(be, 6),
                             _BASIC + ("diag_direction_a_plus_ib", "ragged_lane")),
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


@pytest.mark.parametrize("N", [3, 5, 8])
def test_flux_ring_through_the_noise_model(N, monkeypatch):
    """`structured_perturbation(topo="ring")` with `HH`'s chain bonds edited to e^{i theta} (noise._static_terms splits them
    into h0_offdiag and imaginary draws) on the stand-in: the flux ring's closed form; a conjugated `HH` gives -Phi."""
    import importlib
    stand_in.install(monkeypatch)
    noise = importlib.import_module("code-robchar_amd.noise")
    rc.check_flux_ring_product(noise, N)
    if N % 2:
        with pytest.raises(AssertionError):
            rc.check_flux_ring_product(noise, N, phi=np.pi / 2, conjugate=True)
