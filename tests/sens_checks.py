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

BROKEN = ("zeros", "no_phase", "swapped", "shifted", "diag_once", "rho_no_g0", "mean_by_tiles")


class StandIn(gc.StandIn):
    """`mc_fidelity_sens` (+ `mc_fidelity`, `mc_fidelity_grad` of grad_checks.StandIn) on the CPU.  broken: None or one of
    BROKEN - "zeros"; "no_phase" (dF/dr in the g1 entry without re/r); "swapped" (g1 <-> g2); "shifted" (bond i stored at site
    i - 1); "diag_once" (B_kk counted once); "rho_no_g0" (rho without the site part); "mean_by_tiles" (mean divided by the
    number of tiles)."""

    def __init__(self, broken=None):
        super().__init__(None)
        self.sbroken = broken

    def mc_fidelity_sens(self, ctrl, draws, N, a, b, h0_diag=None, h0_offdiag=None, device=None, want=("fid", "sens", "mean")):
        ctrl, draws = gc._bcast(ctrl, draws)
        F, S = sens_eigh(ctrl, draws, N, a, b, h0_diag, h0_offdiag, diag_once=self.sbroken == "diag_once")
        if self.sbroken == "zeros":
            S = np.where(np.isnan(S), S, 0.0)
        elif self.sbroken == "no_phase":
            h0o = np.ones(N - 1) if h0_offdiag is None else np.asarray(h0_offdiag, dtype=np.float64)
            re, im = h0o + draws[:, :, 1:, 1], draws[:, :, 1:, 2]
            S[:, :, 1:, 1] = (re * S[:, :, 1:, 1] + im * S[:, :, 1:, 2]) / np.hypot(re, im)
        elif self.sbroken == "swapped":
            S = S[..., [0, 2, 1]]
        elif self.sbroken == "shifted":
            S[:, :, :-1, 1:] = S[:, :, 1:, 1:].copy()
            S[:, :, -1, 1:] = 0.0
        K = F.shape[1]
        rho = radial(draws, S) if self.sbroken != "rho_no_g0" else (draws[..., 1:] * S[..., 1:]).sum(axis=(-1, -2))
        M = np.concatenate([F.mean(axis=1)[:, None], rho.mean(axis=1)[:, None], S.mean(axis=1).reshape(F.shape[0], -1)], axis=1)
        if self.sbroken == "mean_by_tiles":
            M = M * K / ((K + 63) // 64)
        res = {"fid": F, "sens": S, "mean": M}
        return {k: v for k, v in res.items() if k in want}


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
