"""References, bounds and data-level checks for the derivative of the chain fidelity with respect to the structured noise
(`backend.mc_fidelity_sens`), shaped like grad_checks.py: the `check_*` functions take a backend object, the GPU tests run
them on the device, and a CPU test runs them on a NumPy stand-in, where they must pass, and on broken ones, where they must
fail.

References.  `sens_frechet`: scipy.linalg.expm_frechet on the dense COMPLEX Hamiltonian of the oracle with the complex
directions E = |i><i|, |i><i-1| + h.c. and i|i><i-1| - h.c. (no gauge, no eigensolver).  `sens_eigh`: the Daleckii-Krein
formula on numpy.linalg.eigh of the same matrix with the same directions (still no gauge) - the fast one.

Bounds.  Every direction has norm 1 like a bias, so per entry  TOL max(1, |T|)  (grad_checks);  for the radial derivative
rho = sum g dF/dg that times sum |g|;  for a row mean the row's largest bar.  The fidelity: chain_checks.compare."""
import numpy as np

import chain_checks as cc
import grad_checks as gc
from oracle import robchar_oracle as orc

TOL = cc.TOL
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------


def sens_frechet(ctrl, draws, N, a, b, h0_diag=None, h0_offdiag=None):
    """(F [C, K], S [C, K, N, 3]) by expm_frechet; S[..., 0, 1:] = 0.  NaN rows give NaN."""
    import scipy.linalg as sl
    ctrl, draws = gc._bcast(ctrl, draws)
    nan = np.isnan(ctrl).any(axis=1)
    H = orc.assemble_hamiltonians(np.nan_to_num(ctrl), draws, N, h0_diag, h0_offdiag)
    C, K = H.shape[:2]
    F = np.empty((C, K))
    S = np.zeros((C, K, N, 3))
    for c in range(C):
        T = abs(np.nan_to_num(ctrl[c, N]))
        for k in range(K):
            A = -1j * T * H[c, k]
            phi = sl.expm(A)[b, a]
            F[c, k] = abs(phi) ** 2
            for i in range(N):
                for comp in range(3 if i else 1):
                    E = np.zeros((N, N), complex)
                    if comp == 0:
                        E[i, i] = 1.0
                    elif comp == 1:
                        E[i, i - 1] = E[i - 1, i] = 1.0
                    else:
                        E[i, i - 1], E[i - 1, i] = 1j, -1j
                    _, L = sl.expm_frechet(A, -1j * T * E)
                    S[c, k, i, comp] = 2 * (np.conj(phi) * L[b, a]).real
    F[nan] = np.nan
    S[nan] = np.nan
    return F, S


def sens_eigh(ctrl, draws, N, a, b, h0_diag=None, h0_offdiag=None, chunk=20000, diag_once=False):
    """The same through eigh of the dense complex Hamiltonian, in chunks of samples.
    `diag_once` is a deliberately WRONG variant for the checks' own tests (the j = k term of a bond counted once)."""
    ctrl, draws = gc._bcast(ctrl, draws)
    C, K = draws.shape[:2]
    F = np.empty((C, K))
    S = np.zeros((C, K, N, 3))
    nan = np.isnan(ctrl).any(axis=1)
    cz = np.nan_to_num(ctrl)
    per = max(1, chunk // max(K, 1))
    ii = np.arange(N)
    for c0 in range(0, C, per):
        cs = slice(c0, min(C, c0 + per))
        H = orc.assemble_hamiltonians(cz[cs], draws[cs], N, h0_diag, h0_offdiag)
        lam, V = np.linalg.eigh(H)
        T = np.abs(cz[cs, N])[:, None, None]
        ph = np.exp(-1j * T * lam)
        wo, wi = V[..., b, :], np.conj(V[..., a, :])
        phi = (wo * wi * ph).sum(-1)
        dl = lam[..., :, None] - lam[..., None, :]
        sm = lam[..., :, None] + lam[..., None, :]
        Tm = T[..., None]
        Gam = -1j * Tm * np.exp(-0.5j * Tm * sm) * np.sinc(Tm * dl / (2 * np.pi))
        W = wo[..., :, None] * Gam * wi[..., None, :]                      # dphi[E] = sum_jk W_jk (V^H E V)_jk
        A = np.conj(V) @ W @ np.swapaxes(V, -1, -2)                        # A[i, i'] = sum_jk conj(V_ij) W_jk V_i'k
        P, Q = A[..., ii[1:], ii[1:] - 1], A[..., ii[1:] - 1, ii[1:]]
        if diag_once:
            Wd = W * (1 - np.eye(N))
            Q = (np.conj(V) @ Wd @ np.swapaxes(V, -1, -2))[..., ii[1:] - 1, ii[1:]]
        cphi = np.conj(phi)[..., None]
        F[cs] = abs(phi) ** 2
        S[cs, :, :, 0] = 2 * (cphi * A[..., ii, ii]).real
        S[cs, :, 1:, 1] = 2 * (cphi * (P + Q)).real
        S[cs, :, 1:, 2] = 2 * (cphi * 1j * (P - Q)).real
    F[nan] = np.nan
    S[nan] = np.nan
    return F, S


def radial(draws, S):
    """rho [C, K] = sum_{i, c} g dF/dg (the entries [0][1], [0][2] of S are 0)"""
    _, draws = gc._bcast(np.zeros((S.shape[0], 1)), draws)
    return (draws * S).sum(axis=(-1, -2))


def mean_of(F, draws, S):
    """[C, 3 N + 2] = (mean F, mean rho, mean dF/dg) of the rows"""
    C, K = F.shape
    return np.concatenate([F.mean(axis=1)[:, None], radial(draws, S).mean(axis=1)[:, None], S.mean(axis=1).reshape(C, -1)], axis=1)


def closed_form_dlam(N, ctrl, inspin, outspin, lam=1.0):
    """d/dlam of chain_checks.closed_form_fid (couplings lam * off_i), the way grad_checks.closed_form_grad differentiates
    it in g and T:  c = nz^2 + (1 - nz^2) cos(Om T), Om = hypot(lam, g), nz^2 = g^2 / Om^2."""
    from math import comb
    g = (ctrl[:, 0] - ctrl[:, N - 1]) / (N - 1)
    T = np.abs(ctrl[:, N])
    om = np.hypot(lam, g)
    nz2 = (g / om) ** 2
    cosv, sinv = np.cos(om * T), np.sin(om * T)
    c = nz2 + (1.0 - nz2) * cosv
    m = outspin if inspin == 0 else N - 1 - outspin
    n1 = N - 1
    p, q = (1.0 + c) / 2.0, (1.0 - c) / 2.0
    t1 = (n1 - m) * p ** max(n1 - m - 1, 0) * q ** m if n1 - m > 0 else 0.0
    t2 = m * p ** (n1 - m) * q ** max(m - 1, 0) if m > 0 else 0.0
    dFdc = 0.5 * comb(n1, m) * (t1 - t2)
    dnz2 = -2.0 * g * g * lam / om ** 4
    dcdl = dnz2 * (1.0 - cosv) - (1.0 - nz2) * sinv * T * lam / om
    return dFdc * dcdl


# ------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------


def sens_bars(ctrl, draws, N):
    """([C, K, N, 3] bound on every entry, [C, K] bound on rho)"""
    ctrl, draws = gc._bcast(ctrl, draws)
    t = TOL * np.maximum(1.0, np.abs(np.nan_to_num(ctrl[:, N])))
    bars = np.broadcast_to(t[:, None, None, None], draws.shape).copy()
    return bars, t[:, None] * np.abs(draws).sum(axis=(-1, -2))


def mean_bars(bars, rbars):
    C = bars.shape[0]
    return np.concatenate([np.full((C, 1), TOL), rbars.max(axis=1)[:, None] + 1e-300, bars.max(axis=1).reshape(C, -1)], axis=1)


def assert_sens_teeth(S, what="", imag=False):
    """A comparison must be able to fail: median |dF/dg0| and median |dF/dg1| >= 1e-2, at least half of the g0 and g1 entries
    above 1e-3 and - where the case has a large imaginary component (`imag`) - median |dF/dg2| >= 1e-3.  NaN rows left out."""
    S = np.asarray(S)
    S = S[~np.isnan(S).any(axis=(-1, -2, -3))]
    g0, g1, g2 = np.abs(S[..., 0]), np.abs(S[..., 1:, 1]), np.abs(S[..., 1:, 2])
    m0, m1, m2 = float(np.median(g0)), float(np.median(g1)), float(np.median(g2))
    share = float((np.concatenate([g0.ravel(), g1.ravel()]) > 1e-3).mean())
    assert m0 >= 1e-2 and m1 >= 1e-2 and share >= 0.5, ("the reference cannot tell a wrong kernel from a right one", what, m0, m1, share)
    if imag:
        assert m2 >= 1e-3, ("the imaginary-coupling reference has no teeth", what, m2)
    return m0, m1, m2, share


def compare_sens(got, want, bars, what):
    """every entry inside its bar, NaN exactly where the reference has NaN; (worst abs, worst error / bar, the same in TOL)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    err = np.where(nan, 0.0, np.abs(got - np.where(nan, 0.0, want)))
    frac = err / bars
    assert frac.max() < 1.0, (what, "error / bar", float(frac.max()), "abs", float(err.max()),
                              "at", np.unravel_index(frac.argmax(), frac.shape))
    return float(err.max()), float(frac.max()), float(frac.max() * TOL)


# ------------------------------------------------------------------------------------------------------------------------
# a NumPy stand-in backend and broken variants of it, for the checks' own CPU tests
# ------------------------------------------------------------------------------------------------------------------------

BROKEN = ("zeros", "no_phase", "swapped", "shifted", "diag_once", "rho_no_g0", "mean_by_tiles", "no_h0_diag", "no_h0_offdiag", "re_g1")
PHILOX_BROKEN = ("philox_no_h0_offdiag", "lost_carry", "mean_64_tiles")      # wrong in the entry that generates its draws only
PHILOX_OUTPUTS = ("fid", "sens", "mean")


class StandIn(gc.StandIn):
    """`mc_fidelity_sens`, `mc_fidelity_sens_philox` (+ `mc_fidelity`, `mc_fidelity_grad`, `philox_normal` of grad_checks.StandIn)
    on the CPU.  broken: None or one of BROKEN - "zeros"; "no_phase" (dF/dr in the g1 entry without re/r); "swapped" (g1 <-> g2);
    "shifted" (bond i stored at site i - 1); "diag_once" (B_kk counted once); "rho_no_g0" (rho without the site part);
    "mean_by_tiles" (mean divided by the number of tiles); "no_h0_diag" / "no_h0_offdiag" (the static term ignored); "re_g1"
    (h0_offdiag in the matrix, but the chain rule from (r, theta) to (g1, g2) taken at re = g1) - or one of PHILOX_BROKEN, as in
    grad_checks.StandIn."""

    def __init__(self, broken=None):
        super().__init__(None)
        self.sbroken = broken

    def mc_fidelity_sens(self, ctrl, draws, N, a, b, h0_diag=None, h0_offdiag=None, device=None, want=("fid", "sens", "mean"),
                         _fused=False):
        ctrl, draws = gc._bcast(ctrl, draws)
        h0_diag, h0_offdiag = gc._dropped(self.sbroken, h0_diag, h0_offdiag, _fused)
        F, S = sens_eigh(ctrl, draws, N, a, b, h0_diag, h0_offdiag, diag_once=self.sbroken == "diag_once")
        h0o = np.ones(N - 1) if h0_offdiag is None else np.asarray(h0_offdiag, dtype=np.float64)
        re, im = h0o + draws[:, :, 1:, 1], draws[:, :, 1:, 2]
        cut = (re == 0.0) & (im == 0.0) & ~np.isnan(S[:, :, 1:, 1])
        # The contract, put in BY HAND (and `+ 0.0` on rho below, which turns a -0.0 into +0.0): both parts of an exactly cut bond
        # are 0.0.  The sound stand-in passing check_cut_bond_sens_philox therefore shows only that the check can be met - it is no
        # reference for the zero; the check's teeth are the broken variants "re_g1", "no_h0_offdiag" and "no_phase".
        S[:, :, 1:, 1:][cut] = 0.0
        if self.sbroken == "zeros":
            S = np.where(np.isnan(S), S, 0.0)
        elif self.sbroken == "no_phase":
            with np.errstate(invalid="ignore"):
                S[:, :, 1:, 1] = (re * S[:, :, 1:, 1] + im * S[:, :, 1:, 2]) / np.hypot(re, im)
        elif self.sbroken == "re_g1":
            # dF/dr = (re S1 + im S2) / r, dF/dtheta = re S2 - im S1; back to (g1, g2) with re' = g1 in place of h0 + g1
            with np.errstate(invalid="ignore", divide="ignore"):
                dr, dth = (re * S[:, :, 1:, 1] + im * S[:, :, 1:, 2]) / np.hypot(re, im), re * S[:, :, 1:, 2] - im * S[:, :, 1:, 1]
                r1, r2 = draws[:, :, 1:, 1], np.hypot(draws[:, :, 1:, 1], im)
                S[:, :, 1:, 1] = dr * r1 / r2 - dth * im / r2 ** 2
                S[:, :, 1:, 2] = dr * im / r2 + dth * r1 / r2 ** 2
        elif self.sbroken == "swapped":
            S = S[..., [0, 2, 1]]
        elif self.sbroken == "shifted":
            S[:, :, :-1, 1:] = S[:, :, 1:, 1:].copy()
            S[:, :, -1, 1:] = 0.0
        K, bm = F.shape[1], self.sbroken if _fused else None
        rho = (radial(draws, S) if self.sbroken != "rho_no_g0" else (draws[..., 1:] * S[..., 1:]).sum(axis=(-1, -2))) + 0.0
        M = np.concatenate([gc._row_mean(F, K, bm)[:, None], gc._row_mean(rho, K, bm)[:, None],
                            gc._row_mean(S, K, bm).reshape(F.shape[0], -1)], axis=1)
        if self.sbroken == "mean_by_tiles":
            M = M * K / ((K + 63) // 64)
        res = {"fid": F, "sens": S, "mean": M}
        return {k: v for k, v in res.items() if k in want}

    def mc_fidelity_sens_philox(self, ctrl, K, N, a, b, seed, offset=0, sigma=0.05, h0_diag=None, h0_offdiag=None, want=PHILOX_OUTPUTS):
        ctrl = np.asarray(ctrl, dtype=np.float64)
        draws = gc.host_draws(seed, offset, (ctrl.shape[0], K, N, 3), sigma, self.sbroken == "lost_carry")
        return self.mc_fidelity_sens(ctrl, draws, N, a, b, h0_diag, h0_offdiag, want=want, _fused=True)


# ------------------------------------------------------------------------------------------------------------------------
# checks (backend in, assertion out)
# ------------------------------------------------------------------------------------------------------------------------


def _check_one(be, ctrl, draws, N, a, b, what, worst, key, h0_diag=None, h0_offdiag=None, teeth=True, imag=False, ref=sens_eigh):
    Fw, Sw = ref(ctrl, draws, N, a, b, h0_diag, h0_offdiag)
    if teeth:
        assert_sens_teeth(Sw, what, imag)
    res = be.mc_fidelity_sens(ctrl, draws, N, a, b, h0_diag=h0_diag, h0_offdiag=h0_offdiag)
    bars, rbars = sens_bars(ctrl, draws, N)
    cc.compare(res["fid"], Fw, (what, "fid"))
    out = compare_sens(res["sens"], Sw, bars, (what, "sens"))
    assert (res["sens"][~np.isnan(res["sens"]).any(axis=(-1, -2))][:, 0, 1:] == 0.0).all(), (what, "entries [0][1], [0][2]")
    compare_sens(res["mean"], mean_of(Fw, draws, Sw), mean_bars(bars, rbars), (what, "mean"))
    if worst is not None:
        worst.add(key, out)
    return out


def imag_sigma(N):
    """sigma of the third draw component in the large-imaginary case (module docstring of the tests: the g2 guard)"""
    return 0.5


def check_deloc_sens(be, N, worst=None, ref=sens_eigh):
    """Delocalised rows (chain_checks.deloc_ctrl), C = 5, K = 192 (three tiles), sigma = 0.05, one NaN row, one row with a
    negative time entry, the grad_pairs; a ragged K = 100 case; XXZ offsets; a non-unit h0_offdiag; a case whose imaginary
    coupling draws have sigma = 0.5 (the g2 teeth)."""
    rng = np.random.default_rng(6300 + N)
    C, K = 5, 192
    ctrl = cc.deloc_ctrl(rng, C, N, 0.5)
    ctrl[1, N] = -ctrl[1, N]
    ctrl[3, N // 2] = np.nan
    draws = 0.05 * rng.standard_normal((C, K, N, 3))
    for (a, b) in gc.grad_pairs(N):
        _check_one(be, ctrl, draws, N, a, b, ("deloc", N, a, b), worst, ("deloc", N), ref=ref)
    c2 = cc.deloc_ctrl(rng, 2, N, 0.5)
    d2 = 0.05 * rng.standard_normal((2, 100, N, 3))
    _check_one(be, c2, d2, N, 0, N - 1, ("deloc ragged", N), worst, ("deloc", N), ref=ref)
    _check_one(be, c2, d2, N, N - 1, 0, ("deloc xxz", N), worst, ("deloc", N), h0_diag=orc.xxz_delta(N), ref=ref)
    off = 1.0 + 0.2 * np.cos(np.arange(N - 1))
    _check_one(be, c2, d2, N, 0, N - 1, ("deloc offdiag", N), worst, ("deloc", N), h0_offdiag=off, ref=ref)
    d3 = d2.copy()
    d3[..., 2] *= imag_sigma(N) / 0.05
    _check_one(be, c2, d3, N, 0, N - 1, ("deloc imag", N), worst, ("imag", N), imag=True, ref=ref)


def check_closed_form_sens(be, N, worst=None):
    """The spin-j chain of chain_checks with zero draws: its couplings are lam off_i, so dF/dlam = sum_i off_i dF/dg1_i at
    lam = 1, against the differentiated closed form - no eigensolver anywhere in the reference."""
    ctrl = cc.closed_form_ctrl(N, cc.CF_GS, cc.CF_TS[1:])
    off = cc.closed_form_offdiag(N)
    draws = np.zeros((ctrl.shape[0], 2, N, 3))
    bars = sens_bars(ctrl, draws, N)[0][:, 0]
    bl = (bars[:, 1:, 1] * np.abs(off)).sum(axis=1)
    big = 0.0
    for a in (0, N - 1):
        for b in range(N):
            res = be.mc_fidelity_sens(ctrl, draws, N, a, b, h0_offdiag=off, want=("fid", "sens"))
            S = res["sens"]
            assert np.array_equal(S[:, 0], S[:, 1]), (N, a, b, "identical samples differ")
            want = closed_form_dlam(N, ctrl, a, b)
            err = np.abs(S[:, 0, 1:, 1] @ off - want)
            assert (err < bl).all(), (N, a, b, "dF/dlam", float(err.max()))
            assert (np.abs(S[:, 0, :, 2]) < bars[:, :, 2]).all(), (N, a, b, "imaginary entries of real couplings")
            assert np.abs(res["fid"][:, 0] - cc.closed_form_fid(N, ctrl, a, b)).max() < TOL
            big = max(big, float(np.abs(want).max()))
            if worst is not None:
                worst.add(("closed form", N), (float(err.max()), float((err / bl).max()), 0.0))
    assert big > 0.1, (N, "the closed-form derivative has no teeth", big)


def check_hard_sens(be, N, worst=None, ref=sens_eigh):
    """grad_checks.hard_inputs: everything finite and inside the bars; both coupling entries of the cut bond exactly 0.0."""
    rng = np.random.default_rng(7700 + N)
    for name, ctrl, draws in gc.hard_inputs(N, rng):
        for (a, b) in gc.grad_pairs(N):
            res = be.mc_fidelity_sens(ctrl, draws, N, a, b)
            assert all(np.isfinite(res[k]).all() for k in ("fid", "sens", "mean")), (name, N, a, b)
            Fw, Sw = ref(ctrl, draws, N, a, b)
            bars, rbars = sens_bars(ctrl, draws, N)
            out = compare_sens(res["sens"], Sw, bars, (name, N, a, b))
            compare_sens(res["mean"], mean_of(Fw, draws, Sw), mean_bars(bars, rbars), (name, N, a, b, "mean"))
            assert np.abs(res["fid"] - Fw).max() < TOL, (name, N, a, b)
            if name == "cut":
                assert (res["sens"][:, :, max(1, N // 2), 1:] == 0.0).all(), (N, a, b, "cut bond")
            if worst is not None:
                worst.add(("hard", name), out)


def fid_route_bound(ctrl, draws, N, h0_diag=None):
    """the bound of tests/test_gpu_grad.py between a fidelity from the all-fp64 QL with eigenvector rows and the
    RC_KERNEL_AUTO route: 64 N eps max(1, T ||H||)"""
    norm = gc.grad_bars(ctrl, draws, N, h0_diag)[..., N] / gc.TOL
    T = np.abs(np.nan_to_num(np.asarray(ctrl)[:, N]))[:, None]
    return 64.0 * N * EPS * np.maximum(1.0, T * norm)


def check_consistency(be, N):
    """Against the neighbouring entries and against itself: sens[..., 0] = the bias entries of mc_fidelity_grad within the sum
    of the two bars; fid inside fid_route_bound of mc_fidelity; the same bits on a second run, from a shared (1, K, N, 3) draw
    set and from `want` subsets; mean within K 2^-52 max|entry| of the row means of sens, mean rho of those of sum g sens."""
    rng = np.random.default_rng(4100 + N)
    C, K = 4, 333
    ctrl = cc.deloc_ctrl(rng, C, N, 0.5)
    shared = 0.05 * rng.standard_normal((1, K, N, 3))
    tiled = np.ascontiguousarray(np.broadcast_to(shared, (C, K, N, 3)))
    a, b = 0, N - 1
    r1 = be.mc_fidelity_sens(ctrl, shared, N, a, b)
    r2 = be.mc_fidelity_sens(ctrl, shared, N, a, b)
    r3 = be.mc_fidelity_sens(ctrl, tiled, N, a, b)
    for k in ("fid", "sens", "mean"):
        assert np.array_equal(r1[k], r2[k]), (k, "not reproducible")
        assert np.array_equal(r1[k], r3[k]), (k, "shared set != tiled set")
    for sub in (("mean",), ("sens",), ("fid",), ("fid", "mean")):
        only = be.mc_fidelity_sens(ctrl, shared, N, a, b, want=sub)
        assert set(only) == set(sub) and all(np.array_equal(only[k], r1[k]) for k in sub), sub
    G = be.mc_fidelity_grad(ctrl, shared, N, a, b, want=("grad",))["grad"]
    bars = sens_bars(ctrl, tiled, N)[0][..., 0] + gc.grad_bars(ctrl, tiled, N)[..., :N]
    d = np.abs(r1["sens"][..., 0] - G[..., :N])
    assert (d < bars).all(), ("site entries against mc_fidelity_grad", float((d / bars).max()))
    d = np.abs(r1["fid"] - be.mc_fidelity(ctrl, tiled, N, a, b))
    assert (d <= fid_route_bound(ctrl, tiled, N)).all(), ("fid against mc_fidelity", float(d.max()))
    rows = mean_of(r1["fid"], tiled, r1["sens"])
    scale = max(1.0, float(np.abs(r1["sens"]).max()))
    d = np.abs(r1["mean"] - rows)
    assert d.max() <= K * EPS * scale, ("mean against the row means", float(d.max()))
    return float(d.max())


# ------------------------------------------------------------------------------------------------------------------------
# checks of the entry that generates its draws (`mc_fidelity_sens_philox`): static terms, cut bond, long rows, far offsets
# ------------------------------------------------------------------------------------------------------------------------

PHILOX_SEED = 0x5EED0009
PHILOX_SIGMA = 0.05


def philox_ctrl(N, C=3, nan_row=1, seed=None):
    """delocalised rows (the sensitivities have teeth there), one of them NaN"""
    ctrl = cc.deloc_ctrl(np.random.default_rng(9100 + N if seed is None else seed), C, N, 0.5)
    if nan_row is not None:
        ctrl[nan_row, N // 2] = np.nan
    return ctrl


def _fused(be, ctrl, K, N, a, b, offset, h0d=None, h0o=None, sigma=PHILOX_SIGMA, want=PHILOX_OUTPUTS):
    return gc.to_host(be.mc_fidelity_sens_philox(ctrl, K, N, a, b, PHILOX_SEED, offset=offset, sigma=sigma, h0_diag=h0d, h0_offdiag=h0o,
                                                 want=want))


def _two_kernels(be, ctrl, K, N, a, b, offset, h0d=None, h0o=None, sigma=PHILOX_SIGMA):
    draws = be.philox_normal((ctrl.shape[0], K, N, 3), PHILOX_SEED, scale=sigma, offset=offset)
    return be.mc_fidelity_sens(ctrl, draws, N, a, b, h0_diag=h0d, h0_offdiag=h0o)


def reference_on_host_draws(ctrl, K, N, a, b, offset, h0d=None, h0o=None, sigma=PHILOX_SIGMA):
    """(draws regenerated on the host, F, S of sens_eigh on them)"""
    draws = gc.host_draws(PHILOX_SEED, offset, (ctrl.shape[0], K, N, 3), sigma)
    return (draws,) + sens_eigh(ctrl, draws, N, a, b, h0d, h0o)


def _compare_with_reference(got, ctrl, draws, Fw, Sw, N, what):
    bars, rbars = sens_bars(ctrl, draws, N)
    cc.compare(got["fid"], Fw, (what, "fid"))
    out = compare_sens(got["sens"], Sw, bars, (what, "sens"))
    compare_sens(got["mean"], mean_of(Fw, draws, Sw), mean_bars(bars, rbars), (what, "mean"))
    return out


def check_static_sens_philox(be, N, identity=True, reference=True, K=130, offsets=(0, 7), worst=None):
    """grad_checks.check_static_grad_philox for the sensitivity entry: every case of grad_checks.static_cases and every pair of
    grad_pairs; the guards on the reference alone, then the bits of the two-kernel route (`identity`) and the bars of sens_eigh on
    host-regenerated draws (`reference`)."""
    ctrl = philox_ctrl(N)
    for case in gc.static_cases(N):
        h0d, h0o = gc.static_terms(N, case)
        for (a, b) in gc.grad_pairs(N):
            for offset in offsets:
                what = ("static", case, N, a, b, offset)
                draws, Fw, Sw = reference_on_host_draws(ctrl, K, N, a, b, offset, h0d, h0o)
                gc.assert_static_teeth(Fw, sens_eigh(ctrl, draws, N, a, b)[0], what)
                assert_sens_teeth(Sw, what)
                got = _fused(be, ctrl, K, N, a, b, offset, h0d, h0o)
                assert all(np.isnan(got[k][1]).all() for k in PHILOX_OUTPUTS), what
                if identity:
                    gc.assert_same_bits(got, _two_kernels(be, ctrl, K, N, a, b, offset, h0d, h0o), what, PHILOX_OUTPUTS)
                if reference:
                    out = _compare_with_reference(got, ctrl, draws, Fw, Sw, N, what)
                    if worst is not None:
                        worst.add(("static", case, N), out)



def cut_pairs(N):
    """(in, out) pairs on one side of the bond between the sites m - 1 and m, m = max(1, N // 2) - F is not trivially 0 - and not
    on a side of one site, where F = 1 whatever the controller"""
    m = max(1, N // 2)
    pairs = [(m, N - 1), (N - 1, N - 1)] + ([(0, m - 1)] if m >= 2 else [])
    return m, tuple(dict.fromkeys(pairs))


def check_cut_bond_sens_philox(be, N, K=130, worst=None):
    """h0_offdiag[m - 1] = 0, sigma_rows = (0, 0.05).  The sigma = 0 row has r = 0 on that bond in every sample: everything finite,
    both coupling derivatives of the bond exactly 0.0, the mean rho exactly +0.0.  The sigma = 0.05 row: inside the bars of
    sens_eigh.  Both rows: the bits of the two-kernel route, row by row at the row's own offset."""
    m, pairs = cut_pairs(N)
    h0o = np.ones(N - 1)
    h0o[m - 1] = 0.0
    rows = np.array([0.0, PHILOX_SIGMA])
    ctrl = philox_ctrl(N, C=2, nan_row=None)
    ctrl[:, N] *= (N - m) / N                      # the time an excitation needs to cross the longer piece, not the whole chain
    for (a, b) in pairs:
        side = slice(m, N) if a >= m else slice(0, m)
        for offset in (0, 7):
            what = ("cut bond", N, a, b, offset)
            draws, Fw, Sw = reference_on_host_draws(ctrl, K, N, a, b, offset, None, h0o, sigma=rows)
            m0 = float(np.median(np.abs(Sw[:, :, side, 0])))
            assert np.median(Fw) >= 1e-2 and m0 >= 1e-2, ("the cut-chain reference cannot tell a wrong kernel from a right one", what,
                                                         float(np.median(Fw)), m0)
            got = _fused(be, ctrl, K, N, a, b, offset, None, h0o, sigma=rows)
            assert all(np.isfinite(got[k][0]).all() for k in PHILOX_OUTPUTS), (what, "sigma = 0 row not finite")
            assert (got["sens"][0, :, m, 1:] == 0.0).all(), (what, "coupling derivatives of the cut bond", got["sens"][0, 0, m, 1:])
            assert (got["mean"][0, 2:].reshape(N, 3)[m, 1:] == 0.0).all(), (what, "mean coupling derivatives of the cut bond")
            rho0 = got["mean"][0, 1]
            assert rho0 == 0.0 and not np.signbit(rho0), (what, "mean rho of the sigma = 0 row", rho0)
            assert (got["sens"][0] == got["sens"][0, :1]).all() and (got["fid"][0] == got["fid"][0, 0]).all(), what
            for c, sigma in enumerate(rows):
                want = _two_kernels(be, ctrl[c:c + 1], K, N, a, b, offset + c * K * N * 3, None, h0o, sigma=float(sigma))
                gc.assert_same_bits({k: got[k][c:c + 1] for k in PHILOX_OUTPUTS}, want, (what, "row", c), PHILOX_OUTPUTS)
            out = _compare_with_reference(got, ctrl, draws, Fw, Sw, N, what)
            if worst is not None:
                worst.add(("cut bond", N), out)


def _assert_mean_of_same_launch(res, draws, K, what, report=None):
    ok = ~np.isnan(res["fid"]).any(axis=1)
    rows = mean_of(res["fid"][ok], draws[ok], res["sens"][ok])
    bound = K * EPS * max(1.0, float(np.abs(res["sens"][ok]).max()))
    err = float(np.abs(res["mean"][ok] - rows).max())
    if report is not None:
        report(f"{what}: |mean - host row means| = {err:.2e} ({err / bound:.2e} of the bound)")
    assert err <= bound, (what, "mean against the row means of the same launch", err, bound)


def check_long_rows_sens_philox(be, N, K, report=None):
    """Rows of more than 64 tiles in the row-mean kernel (3 N + 2 entries per part row), C = 3 with a NaN row, draws generated in
    the kernel: mean bit-identical between the two routes and within K 2^-52 max(1, max |entry|) of the host row means of the
    same launch's fid, rho and sens."""
    ctrl = philox_ctrl(N)
    a, b, offset = 0, N - 1, 7
    what = ("long rows", N, K)
    full = _fused(be, ctrl, K, N, a, b, offset)
    assert_sens_teeth(full["sens"], what)
    assert all(np.isnan(full[k][1]).all() for k in PHILOX_OUTPUTS), what
    gc.assert_same_bits(full, _two_kernels(be, ctrl, K, N, a, b, offset), what, PHILOX_OUTPUTS)
    draws = gc.host_draws(PHILOX_SEED, offset, (ctrl.shape[0], K, N, 3), PHILOX_SIGMA)
    _assert_mean_of_same_launch(full, draws, K, f"long rows, generated draws, N = {N}, K = {K}", report)
    only = _fused(be, ctrl, K, N, a, b, offset, want=("mean",))
    gc.assert_same_bits(only, full, (what, "mean alone"), ("mean",))


def check_long_rows_sens(be, N, K, report=None):
    """the same through plain `mc_fidelity_sens` on a draw tensor"""
    ctrl = philox_ctrl(N)
    draws = PHILOX_SIGMA * np.random.default_rng(8800 + N).standard_normal((ctrl.shape[0], K, N, 3))
    res = be.mc_fidelity_sens(ctrl, draws, N, 0, N - 1)
    assert_sens_teeth(res["sens"], ("long rows, draw tensor", N, K))
    assert all(np.isnan(res[k][1]).all() for k in PHILOX_OUTPUTS)
    _assert_mean_of_same_launch(res, draws, K, f"long rows, draw tensor, N = {N}, K = {K}", report)
    gc.assert_same_bits(be.mc_fidelity_sens(ctrl, draws, N, 0, N - 1, want=("mean",)), res, ("long rows", "mean alone"), ("mean",))


def check_far_offsets_sens_philox(be, N, K=130, worst=None):
    """grad_checks.check_far_offsets_grad_philox for the sensitivity entry"""
    ctrl = philox_ctrl(N)
    for offset in (gc.wrap_offset(N), gc.FAR_OFFSET):
        for (a, b) in gc.grad_pairs(N)[:2]:
            what = ("far offset", N, a, b, offset)
            draws, Fw, Sw = reference_on_host_draws(ctrl, K, N, a, b, offset)
            assert_sens_teeth(Sw, what)
            got = _fused(be, ctrl, K, N, a, b, offset)
            gc.assert_same_bits(got, _two_kernels(be, ctrl, K, N, a, b, offset), what, PHILOX_OUTPUTS)
            out = _compare_with_reference(got, ctrl, draws, Fw, Sw, N, what)
            if worst is not None:
                worst.add(("far offset", N), out)
