"""References, bounds and data-level checks for the gradient of the chain fidelity with respect to the controller
(`backend.mc_fidelity_grad`), shaped like chain_checks.py: the `check_*` functions take a backend object, the GPU tests run
them on the device, and a CPU test runs them on a NumPy stand-in, where they must pass, and on broken ones, where they
must fail.

References.  `grad_frechet`: scipy.linalg.expm_frechet on the dense COMPLEX Hamiltonian of the oracle (no gauge, no
eigensolver).  `grad_eigh`: the spectral formulas on numpy.linalg.eigh of the same matrix - the fast one for full-size inputs.

Bounds.  The fidelity bar is chain_checks.TOL = 1e-10 absolute.  A bias derivative carries one factor of at most T
(|dphi/dx_l| <= T), the time derivative one factor of at most ||H|| <= max|d_i| + 2 max e_i, hence per sample
    |err dF/dx_l| <= TOL max(1, T),       |err dF/dx_N| <= TOL max(1, max_i |d_i| + 2 max_i e_i)
and for the mean over a row the same with the row's largest scale."""
import numpy as np

import chain_checks as cc
from oracle import philox_host
from oracle import robchar_oracle as orc

TOL = cc.TOL
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------


def _bcast(ctrl, draws):
    ctrl = np.asarray(ctrl, dtype=np.float64)
    draws = np.asarray(draws, dtype=np.float64)
    if draws.shape[0] == 1 and ctrl.shape[0] > 1:
        draws = np.broadcast_to(draws, (ctrl.shape[0],) + draws.shape[1:])
    return ctrl, draws


def grad_frechet(ctrl, draws, N, a, b, h0_diag=None, h0_offdiag=None):
    """(F [C, K], G [C, K, N + 1]) by expm_frechet: direction -i T |l><l| for the biases, (-i H U)[out, in] for the time."""
    import scipy.linalg as sl
    ctrl, draws = _bcast(ctrl, draws)
    H = orc.assemble_hamiltonians(ctrl, draws, N, h0_diag, h0_offdiag)
    C, K = H.shape[:2]
    F = np.empty((C, K))
    G = np.empty((C, K, N + 1))
    for c in range(C):
        T, sg = abs(ctrl[c, N]), np.sign(ctrl[c, N])
        for k in range(K):
            A = -1j * T * H[c, k]
            U = sl.expm(A)
            phi = U[b, a]
            for l in range(N):
                E = np.zeros((N, N), complex)
                E[l, l] = -1j * T
                _, L = sl.expm_frechet(A, E)
                G[c, k, l] = 2 * (np.conj(phi) * L[b, a]).real
            F[c, k] = abs(phi) ** 2
            G[c, k, N] = sg * 2 * (np.conj(phi) * (-1j * (H[c, k] @ U))[b, a]).real
    return F, G


def grad_eigh(ctrl, draws, N, a, b, h0_diag=None, h0_offdiag=None, chunk=20000, gamma_diag_only=False):
    """The spectral formulas on eigh of the dense complex Hamiltonian, in chunks of samples.  NaN rows give NaN.
    `gamma_diag_only` is a deliberately WRONG variant for the checks' own tests (Gam_jk replaced by Gam_kk)."""
    ctrl, draws = _bcast(ctrl, draws)
    C, K = draws.shape[:2]
    F = np.empty((C, K))
    G = np.empty((C, K, N + 1))
    nan = np.isnan(ctrl).any(axis=1)
    cz = np.nan_to_num(ctrl)
    per = max(1, chunk // max(K, 1))
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
        if gamma_diag_only:
            Gam = np.broadcast_to((-1j * T * ph)[..., None, :], Gam.shape)
        A = wo[..., None, :] * np.conj(V)            # [.., l, j]
        B = V * wi[..., None, :]                     # [.., l, k]
        X = np.einsum('...lj,...jk,...lk->...l', A, Gam, B)
        F[cs] = abs(phi) ** 2
        G[cs, :, :N] = 2 * (np.conj(phi)[..., None] * X).real
        G[cs, :, N] = np.sign(cz[cs, N])[:, None] * 2 * (np.conj(phi) * (-1j * (wo * wi * ph * lam).sum(-1))).real
    F[nan] = np.nan
    G[nan] = np.nan
    return F, G


def closed_form_grad(N, ctrl, inspin, outspin, lam=1.0):
    """d/dT and d/dg of chain_checks.closed_form_fid for the rows of closed_form_ctrl (inspin = 0 or N - 1):
    F = binom(N-1, m) p^(N-1-m) q^m, p = (1 + c)/2, q = (1 - c)/2, c = nz^2 + (1 - nz^2) cos(Om T).
    Returns (dF/dT, dF/dg) with dF/dg = sum_n ((N - 1)/2 - n) dF/dx_n (the biases are g ((N - 1)/2 - n))."""
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
    # dF/dc = binom/2 [(n1 - m) p^(n1-m-1) q^m - m p^(n1-m) q^(m-1)]
    t1 = (n1 - m) * p ** max(n1 - m - 1, 0) * q ** m if n1 - m > 0 else 0.0
    t2 = m * p ** (n1 - m) * q ** max(m - 1, 0) if m > 0 else 0.0
    dFdc = 0.5 * comb(n1, m) * (t1 - t2)
    dcdT = -(1.0 - nz2) * om * sinv
    # d nz^2 / dg = 2 g lam^2 / om^4,  d om / dg = g / om
    dnz2 = 2.0 * g * lam * lam / om ** 4
    dcdg = dnz2 * (1.0 - cosv) - (1.0 - nz2) * sinv * T * g / om
    return dFdc * dcdT, dFdc * dcdg


# ------------------------------------------------------------------------------------------------------------------------
# static Hamiltonian terms shared by the tests of the kernels that generate their draws
# ------------------------------------------------------------------------------------------------------------------------


def static_cases(N):
    """names of the static-term cases for an N-spin chain: "xxz" (h0_diag = the XXZ diagonal), "off" (non-unit h0_offdiag of
    both signs), "both".  At N = 2 the XXZ diagonal is uniform - a global phase - so "xxz" alone changes nothing and is left out."""
    return ("off", "both") if N == 2 else ("xxz", "off", "both")


def static_terms(N, case):
    """(h0_diag, h0_offdiag) of a case of `static_cases`; None = the default.  The couplings are U(0.6, 1.4) with the sign
    flipped on every odd bond: negative static couplings are legal, and they are what tells re / r from |re| / r."""
    off = np.random.default_rng(N).uniform(0.6, 1.4, N - 1)
    off[1::2] *= -1.0
    return (orc.xxz_delta(N) if case in ("xxz", "both") else None), (off if case in ("off", "both") else None)


def static_hh(N, case="both"):
    """the `HH` matrix of a noise model that carries the static terms of a case: chain hopping h0_offdiag, diagonal h0_diag"""
    h0d, h0o = static_terms(N, case)
    hop = np.arange(1, N)
    HH = np.zeros((N, N), dtype=np.complex128)
    HH[hop, hop - 1] = HH[hop - 1, hop] = np.ones(N - 1) if h0o is None else h0o
    HH[np.arange(N), np.arange(N)] = 0.0 if h0d is None else h0d
    return HH


def assert_static_teeth(F_with, F_without, what=""):
    """The static terms must matter: median |F(with the terms) - F(without)| >= 1e-2 over the non-NaN rows of the REFERENCE, or a
    kernel that drops them would pass."""
    F_with, F_without = np.asarray(F_with), np.asarray(F_without)
    ok = ~np.isnan(F_with).any(axis=-1)
    med = float(np.median(np.abs(F_with[ok] - F_without[ok])))
    assert med >= 1e-2, ("the static terms do not change the reference fidelity enough to be missed", what, med)
    return med


# ------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------


def grad_bars(ctrl, draws, N, h0_diag=None, h0_offdiag=None):
    """[C, K, N + 1] bound on the error of every gradient entry (module docstring)"""
    ctrl, draws = _bcast(ctrl, draws)
    cz = np.nan_to_num(ctrl)
    h0d = np.zeros(N) if h0_diag is None else np.asarray(h0_diag, dtype=np.float64)
    h0o = np.ones(N - 1) if h0_offdiag is None else np.asarray(h0_offdiag, dtype=np.float64)
    d = cz[:, None, :N] + h0d + draws[..., 0]
    e = np.hypot(h0o + draws[:, :, 1:, 1], draws[:, :, 1:, 2])
    norm = np.abs(d).max(-1) + 2.0 * e.max(-1)
    bars = np.empty(draws.shape[:2] + (N + 1,))
    bars[..., :N] = (TOL * np.maximum(1.0, np.abs(cz[:, N])))[:, None, None]
    bars[..., N] = TOL * np.maximum(1.0, norm)
    return bars


def assert_grad_teeth(G, what=""):
    """A gradient comparison must be able to fail: median |dF/dx_l| over the bias entries >= 1e-2 and at least half of all
    entries above 1e-3.  NaN rows are left out."""
    G = np.asarray(G)
    G = G[~np.isnan(G).any(axis=(-1, -2))] if G.ndim == 3 else G
    bias = np.abs(G[..., :-1])
    med, share = float(np.median(bias)), float((np.abs(G) > 1e-3).mean())
    assert med >= 1e-2 and share >= 0.5, ("the reference gradient cannot tell a wrong kernel from a right one", what, med, share)
    return med, share


def compare_grad(got, want, bars, what, T=None):
    """every entry inside its bar, NaN exactly where the reference has NaN; returns (worst abs error, worst error / bar,
    worst bias-entry error per unit of max(1, T))"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    err = np.where(nan, 0.0, np.abs(got - np.where(nan, 0.0, want)))
    frac = err / bars
    per_t = float((err[..., :-1] / bars[..., :-1]).max() * TOL)
    assert frac.max() < 1.0, (what, "error / bar", float(frac.max()), "abs", float(err.max()),
                              "at", np.unravel_index(frac.argmax(), frac.shape))
    return float(err.max()), float(frac.max()), per_t


class Worst:
    """worst (abs, share of the bar, per unit of T) per workload - printed by the GPU tests"""

    def __init__(self):
        self.by = {}

    def add(self, key, res):
        old = self.by.get(key, (0.0, 0.0, 0.0))
        self.by[key] = tuple(max(o, r) for o, r in zip(old, res))

    def __str__(self):
        return "; ".join(f"{k}: abs {a:.1e} of-bar {f:.1e} per-T {t:.1e}" for k, (a, f, t) in sorted(self.by.items(), key=str))


# ------------------------------------------------------------------------------------------------------------------------
# a NumPy stand-in backend (the eigh formulas) and broken variants of it, for the checks' own CPU tests
# ------------------------------------------------------------------------------------------------------------------------


PHILOX_OUTPUTS = ("fid", "grad", "mean", "moment")
WRAP = 2 ** 33                       # the stream element at which the low word of the Box-Muller pair counter (element >> 1) wraps


def host_draws(seed, offset, shape, scale, lost_carry=False):
    """oracle/philox_host.py draws in the layout of `backend.philox_normal`; `scale` a float or one value per leading row.
    `lost_carry` is a deliberately WRONG variant for the checks' own tests: the pair counter's high word stays that of the first
    element, so elements behind a multiple of 2^33 repeat the stream 2^33 elements earlier."""
    n = int(np.prod(shape))
    cut = (offset // WRAP + 1) * WRAP
    if lost_carry and offset < cut < offset + n:
        flat = np.concatenate([philox_host.philox_normal(seed, offset, cut - offset),
                               philox_host.philox_normal(seed, cut - WRAP, offset + n - cut)])
    else:
        flat = philox_host.philox_normal(seed, offset, n)
    z = flat.reshape(shape)
    scale = np.asarray(scale, dtype=np.float64)
    return z * (scale.reshape((-1,) + (1,) * (z.ndim - 1)) if scale.ndim else float(scale))


def _dropped(broken, h0_diag, h0_offdiag, fused=False):
    """the static terms as a broken stand-in sees them"""
    if broken == "no_h0_diag":
        h0_diag = None
    if broken == "no_h0_offdiag" or (fused and broken == "philox_no_h0_offdiag"):
        h0_offdiag = None
    return h0_diag, h0_offdiag


def _row_mean(x, K, broken):
    """the mean over axis 1; broken "mean_64_tiles": only the first 64 tiles of 64 samples are added"""
    if x.shape[1] == 0:
        return np.zeros(x.shape[:1] + x.shape[2:])
    return x[:, :4096].sum(axis=1) / K if broken == "mean_64_tiles" else x.mean(axis=1)


class StandIn:
    """`mc_fidelity_grad` / `mc_fidelity` / `philox_normal` / `mc_fidelity_grad_philox` of the backend on the CPU.  broken: None,
    "zeros", "time_sign" (sign of the time entry dropped for negative x_N), "reversed" (bias entries in reversed order),
    "gamma_diag" (Gam_jk = Gam_kk), "no_h0_diag" / "no_h0_offdiag" (the static term ignored), and in the entry that generates
    its draws only: "philox_no_h0_offdiag", "lost_carry" (`host_draws`), "mean_64_tiles" (row sums stop after 64 tiles)."""

    def __init__(self, broken=None):
        self.broken = broken

    def mc_fidelity(self, ctrl, draws, N, a, b, h0_diag=None, h0_offdiag=None, kernel="auto"):
        return grad_eigh(ctrl, draws, N, a, b, h0_diag, h0_offdiag)[0]

    def philox_normal(self, shape, seed, scale=1.0, offset=0):
        return host_draws(seed, offset, shape, scale)

    def mc_fidelity_grad(self, ctrl, draws, N, a, b, h0_diag=None, h0_offdiag=None, device=None, want=("fid", "grad", "mean"),
                         _fused=False):
        ctrl = np.asarray(ctrl, dtype=np.float64)
        h0_diag, h0_offdiag = _dropped(self.broken, h0_diag, h0_offdiag, _fused)
        F, G = grad_eigh(ctrl, draws, N, a, b, h0_diag, h0_offdiag, gamma_diag_only=self.broken == "gamma_diag")
        if self.broken == "zeros":
            G = np.where(np.isnan(G), G, 0.0)
        elif self.broken == "time_sign":
            G[..., N] = np.sign(ctrl[:, N])[:, None] * G[..., N]          # = 2 Re(conj(phi) dphi/dT) without the sign
        elif self.broken == "reversed":
            G[..., :N] = G[..., :N][..., ::-1]
        K, bm = F.shape[1], self.broken if _fused else None
        res = {}
        if "fid" in want:
            res["fid"] = F
        if "grad" in want:
            res["grad"] = G
        if "mean" in want:
            res["mean"] = np.concatenate([_row_mean(F, K, bm)[:, None], _row_mean(G, K, bm)], axis=1)
        if "moment" in want:
            res["moment"] = np.concatenate([_row_mean(F * F, K, bm)[:, None], _row_mean(F[..., None] * G, K, bm)], axis=1)
        return res

    def mc_fidelity_grad_philox(self, ctrl, K, N, a, b, seed, offset=0, sigma=0.05, shared=False, h0_diag=None, h0_offdiag=None,
                                want=PHILOX_OUTPUTS):
        ctrl = np.asarray(ctrl, dtype=np.float64)
        C = ctrl.shape[0]
        if shared:
            draws = host_draws(seed, offset, (1, K, N, 3), 1.0, self.broken == "lost_carry")
            draws = draws * np.broadcast_to(sigma, (C,))[:, None, None, None]
        else:
            draws = host_draws(seed, offset, (C, K, N, 3), sigma, self.broken == "lost_carry")
        return self.mc_fidelity_grad(ctrl, draws, N, a, b, h0_diag, h0_offdiag, want=want, _fused=True)


# ------------------------------------------------------------------------------------------------------------------------
# checks (backend in, assertion out)
# ------------------------------------------------------------------------------------------------------------------------


def grad_pairs(N):
    return tuple(dict.fromkeys(((0, N - 1), (N - 1, 0), (min(1, N - 1), N // 2), (N // 2, N // 2))))


def _check_one(be, ctrl, draws, N, a, b, what, worst, key, h0_diag=None, h0_offdiag=None, teeth=True, ref=grad_eigh):
    Fw, Gw = ref(ctrl, draws, N, a, b, h0_diag, h0_offdiag)
    if teeth:
        assert_grad_teeth(Gw, what)
    res = be.mc_fidelity_grad(ctrl, draws, N, a, b, h0_diag=h0_diag, h0_offdiag=h0_offdiag)
    bars = grad_bars(ctrl, draws, N, h0_diag, h0_offdiag)
    cc.compare(res["fid"], Fw, (what, "fid"))
    out = compare_grad(res["grad"], Gw, bars, (what, "grad"))
    # the mean over the row: the same bars with the row's largest scale
    mw = np.concatenate([Fw.mean(axis=1)[:, None], Gw.mean(axis=1)], axis=1)
    mb = np.concatenate([np.full((bars.shape[0], 1), TOL), bars.max(axis=1)], axis=1)
    compare_grad(res["mean"], mw, mb, (what, "mean"))
    if worst is not None:
        worst.add(key, out)
    return out


def check_deloc_grad(be, N, worst=None):
    """Delocalised rows (chain_checks.deloc_ctrl), K = 192 (three tiles), sigma = 0.05, one NaN row, one row with a negative
    time entry; pairs end to end both ways, interior, in == out; a ragged K = 100 case; XXZ offsets; non-unit static couplings
    of both signs (`static_terms`) under random draws, with the guard that they matter."""
    rng = np.random.default_rng(5200 + N)
    C, K = 5, 192
    ctrl = cc.deloc_ctrl(rng, C, N, 0.5)
    ctrl[1, N] = -ctrl[1, N]
    ctrl[3, N // 2] = np.nan
    draws = 0.05 * rng.standard_normal((C, K, N, 3))
    for (a, b) in grad_pairs(N):
        _check_one(be, ctrl, draws, N, a, b, ("deloc", N, a, b), worst, ("deloc", N))
    c2 = cc.deloc_ctrl(rng, 2, N, 0.5)
    d2 = 0.05 * rng.standard_normal((2, 100, N, 3))
    _check_one(be, c2, d2, N, 0, N - 1, ("deloc ragged", N), worst, ("deloc", N))
    _check_one(be, c2, d2, N, N - 1, 0, ("deloc xxz", N), worst, ("deloc", N), h0_diag=orc.xxz_delta(N))
    off = static_terms(N, "off")[1]
    assert_static_teeth(grad_eigh(c2, d2, N, 0, N - 1, None, off)[0], grad_eigh(c2, d2, N, 0, N - 1)[0], ("deloc offdiag", N))
    _check_one(be, c2, d2, N, 0, N - 1, ("deloc offdiag", N), worst, ("deloc", N), h0_offdiag=off)


def check_closed_form_grad(be, N, worst=None):
    """The spin-j chain of chain_checks (no draws, non-unit h0_offdiag): dF/dT and dF/dg = sum_n ((N-1)/2 - n) dF/dx_n
    against the differentiated closed form - no eigensolver anywhere in the reference."""
    ctrl = cc.closed_form_ctrl(N, cc.CF_GS, cc.CF_TS[1:])
    off = cc.closed_form_offdiag(N)
    draws = np.zeros((ctrl.shape[0], 2, N, 3))
    coef = (N - 1) / 2 - np.arange(N)
    bars = grad_bars(ctrl, draws, N, None, off)[:, 0]
    big = 0.0
    for a in (0, N - 1):
        for b in range(N):
            res = be.mc_fidelity_grad(ctrl, draws, N, a, b, h0_offdiag=off, want=("fid", "grad"))
            dT, dg = closed_form_grad(N, ctrl, a, b)
            G = res["grad"]
            assert np.array_equal(G[:, 0], G[:, 1]), (N, a, b, "identical samples differ")
            eT = np.abs(G[:, 0, N] - dT)
            eg = np.abs(G[:, 0, :N] @ coef - dg)
            # dF/dg sums N entries with weights |coef|: its bar is the weighted sum of the entries' bars
            bg = (bars[:, :N] * np.abs(coef)).sum(axis=1) + 1e-300
            assert (eT < bars[:, N]).all(), (N, a, b, "dF/dT", float(eT.max()))
            assert (eg < bg).all(), (N, a, b, "dF/dg", float(eg.max()))
            assert np.abs(res["fid"][:, 0] - cc.closed_form_fid(N, ctrl, a, b)).max() < TOL
            big = max(big, float(np.abs(dg).max()))
            if worst is not None:
                worst.add(("closed form", N), (float(max(eT.max(), eg.max())), float(max((eT / bars[:, N]).max(), (eg / bg).max())), 0.0))
    assert big > 0.1, (N, "the closed-form gradient has no teeth", big)


def hard_inputs(N, rng):
    """(name, ctrl, draws) of the inputs a spectral route is most likely to get wrong."""
    K = 3
    z = np.zeros((1, K, N, 3))
    uni = np.zeros((1, N + 1))
    uni[0, N] = 0.6 * N
    mirror = np.zeros((1, N + 1))
    half = rng.uniform(-0.5, 0.5, (N + 1) // 2)
    mirror[0, :N] = np.concatenate([half, half[:N // 2][::-1]])
    mirror[0, N] = -0.6 * N
    clus = np.zeros((1, N + 1))
    clus[0, :N] = rng.uniform(-1e-7, 1e-7, N)
    clus[0, N] = 0.55 * N
    cut = cc.deloc_ctrl(rng, 1, N, 0.5)
    dcut = 0.05 * rng.standard_normal((1, K, N, 3))
    dcut[:, :, max(1, N // 2), 1] = -1.0
    dcut[:, :, max(1, N // 2), 2] = 0.0
    t0 = cc.deloc_ctrl(rng, 1, N, 0.5)
    t0[0, N] = 0.0
    bigb = np.full((1, N + 1), 1e3)
    bigb[0, :N] += rng.uniform(-0.5, 0.5, N)
    bigb[0, N] = 30.0
    rnd = 0.05 * rng.standard_normal((1, K, N, 3))
    return (("uniform", uni, z), ("mirror", mirror, z), ("clustered", clus, z), ("cut", cut, dcut), ("T=0", t0, rnd),
            ("bias 1e3", bigb, rnd))


def check_hard_inputs(be, N, worst=None, ref=grad_eigh):
    rng = np.random.default_rng(7700 + N)
    for name, ctrl, draws in hard_inputs(N, rng):
        for (a, b) in grad_pairs(N):
            res = be.mc_fidelity_grad(ctrl, draws, N, a, b, want=("fid", "grad"))
            assert np.isfinite(res["grad"]).all() and np.isfinite(res["fid"]).all(), (name, N, a, b)
            Fw, Gw = ref(ctrl, draws, N, a, b)
            out = compare_grad(res["grad"], Gw, grad_bars(ctrl, draws, N), (name, N, a, b))
            assert np.abs(res["fid"] - Fw).max() < TOL, (name, N, a, b)
            if worst is not None:
                worst.add(("hard", name), out)


def check_mean_and_shared(be, N=7):
    """mean_out = the row means of grad_out within K 2^-52 max|entry|, the same bits on a second run; the shared draw set
    (1, K, N, 3) = the tiled set bit for bit; `want` subsets give the same bits."""
    rng = np.random.default_rng(99)
    C, K = 4, 333
    ctrl = cc.deloc_ctrl(rng, C, N, 0.5)
    shared = 0.05 * rng.standard_normal((1, K, N, 3))
    tiled = np.ascontiguousarray(np.broadcast_to(shared, (C, K, N, 3)))
    r1 = be.mc_fidelity_grad(ctrl, shared, N, 0, N - 1)
    r2 = be.mc_fidelity_grad(ctrl, shared, N, 0, N - 1)
    r3 = be.mc_fidelity_grad(ctrl, tiled, N, 0, N - 1)
    for k in ("fid", "grad", "mean"):
        assert np.array_equal(r1[k], r2[k]), (k, "not reproducible")
        assert np.array_equal(r1[k], r3[k]), (k, "shared set != tiled set")
    rows = np.concatenate([r1["fid"].mean(axis=1)[:, None], r1["grad"].mean(axis=1)], axis=1)
    scale = np.maximum(np.abs(r1["grad"]).max(), 1.0)
    assert np.abs(r1["mean"] - rows).max() <= K * 2.0 ** -52 * scale, float(np.abs(r1["mean"] - rows).max())
    only = be.mc_fidelity_grad(ctrl, shared, N, 0, N - 1, want=("mean",))
    assert set(only) == {"mean"} and np.array_equal(only["mean"], r1["mean"])
    only = be.mc_fidelity_grad(ctrl, shared, N, 0, N - 1, want=("grad",))
    assert set(only) == {"grad"} and np.array_equal(only["grad"], r1["grad"])


# ------------------------------------------------------------------------------------------------------------------------
# checks of the entry that generates its draws (`mc_fidelity_grad_philox`): static terms, long rows, far stream offsets
# ------------------------------------------------------------------------------------------------------------------------

PHILOX_SEED = 0x5EED000A
PHILOX_SIGMA = 0.05
FAR_OFFSET = 123456789012345


def wrap_offset(N):
    """odd, and the pair counter's low word wraps to 0 inside lane 32's sample of the first tile (3 N elements per sample)"""
    return WRAP - 32 * 3 * N - 1


# controller seeds of the static-term cases where 9300 + N falls under a guard: at N = 3 the "off" case, 0 -> 2, has a median
# |dF/dx_l| of 0.0084 on the rows of seed 9303, under the 1e-2 of assert_grad_teeth; on those of seed 9503 it is 0.055
STATIC_CTRL_SEED = {3: 9503}


def philox_ctrl(N, C=3, nan_row=1, neg_row=2, seed=None):
    """delocalised rows (the gradients have teeth there), one of them NaN, one with a negative time entry"""
    ctrl = cc.deloc_ctrl(np.random.default_rng(9300 + N if seed is None else seed), C, N, 0.5)
    if neg_row is not None:
        ctrl[neg_row, N] = -ctrl[neg_row, N]
    if nan_row is not None:
        ctrl[nan_row, N // 2] = np.nan
    return ctrl


def to_host(res):
    """a dict of NumPy arrays from a dict of NumPy arrays or torch tensors"""
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in res.items()}


def assert_same_bits(got, want, what, keys):
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k], equal_nan=True), (
            what, k, "differs in", int((~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k])))).sum()), "entries, max |diff|",
            float(np.nanmax(np.abs(got[k] - want[k]))))


def _fused(be, ctrl, K, N, a, b, offset, shared, h0d=None, h0o=None, sigma=PHILOX_SIGMA, want=PHILOX_OUTPUTS):
    return to_host(be.mc_fidelity_grad_philox(ctrl, K, N, a, b, PHILOX_SEED, offset=offset, sigma=sigma, shared=shared, h0_diag=h0d,
                                              h0_offdiag=h0o, want=want))


def _two_kernels(be, ctrl, K, N, a, b, offset, shared, h0d=None, h0o=None, sigma=PHILOX_SIGMA):
    draws = be.philox_normal((1 if shared else ctrl.shape[0], K, N, 3), PHILOX_SEED, scale=sigma, offset=offset)
    return be.mc_fidelity_grad(ctrl, draws, N, a, b, h0_diag=h0d, h0_offdiag=h0o)


def reference_on_host_draws(ctrl, K, N, a, b, offset, shared, h0d=None, h0o=None, sigma=PHILOX_SIGMA):
    """(draws regenerated on the host, F, G of grad_eigh on them)"""
    draws = host_draws(PHILOX_SEED, offset, (1 if shared else ctrl.shape[0], K, N, 3), sigma)
    return (draws,) + grad_eigh(ctrl, draws, N, a, b, h0d, h0o)


def _compare_with_reference(got, ctrl, draws, Fw, Gw, N, h0d, h0o, what):
    bars = grad_bars(ctrl, draws, N, h0d, h0o)
    cc.compare(got["fid"], Fw, (what, "fid"))
    out = compare_grad(got["grad"], Gw, bars, (what, "grad"))
    mw = np.concatenate([Fw.mean(axis=1)[:, None], Gw.mean(axis=1)], axis=1)
    mb = np.concatenate([np.full((bars.shape[0], 1), TOL), bars.max(axis=1)], axis=1)
    compare_grad(got["mean"], mw, mb, (what, "mean"))
    return out


def check_static_grad_philox(be, N, identity=True, reference=True, K=130, offsets=(0, 7), worst=None):
    """Every case of `static_cases`, every pair of `grad_pairs`, both draw modes.  On the reference alone first: the static terms
    change F (`assert_static_teeth`) and the gradient has teeth.  `identity`: fid, grad, mean carry the bits of `philox_normal` +
    `mc_fidelity_grad` with the same terms.  `reference`: inside the bars of grad_eigh on host-regenerated draws."""
    ctrl = philox_ctrl(N, seed=STATIC_CTRL_SEED.get(N))
    for case in static_cases(N):
        h0d, h0o = static_terms(N, case)
        for (a, b) in grad_pairs(N):
            for offset in offsets:
                for shared in (False, True):
                    what = ("static", case, N, a, b, offset, "shared" if shared else "per row")
                    draws, Fw, Gw = reference_on_host_draws(ctrl, K, N, a, b, offset, shared, h0d, h0o)
                    assert_static_teeth(Fw, grad_eigh(ctrl, draws, N, a, b)[0], what)
                    assert_grad_teeth(Gw, what)
                    got = _fused(be, ctrl, K, N, a, b, offset, shared, h0d, h0o)
                    assert all(np.isnan(got[k][1]).all() for k in PHILOX_OUTPUTS) and np.isfinite(got["moment"][[0, 2]]).all(), what
                    if identity:
                        assert_same_bits(got, _two_kernels(be, ctrl, K, N, a, b, offset, shared, h0d, h0o), what, ("fid", "grad", "mean"))
                    if reference:
                        out = _compare_with_reference(got, ctrl, draws, Fw, Gw, N, h0d, h0o, what)
                        if worst is not None:
                            worst.add(("static", case, N), out)


def host_moments(res):
    return np.concatenate([(res["fid"] ** 2).mean(axis=1)[:, None], (res["fid"][..., None] * res["grad"]).mean(axis=1)], axis=1)


def host_means(res):
    return np.concatenate([res["fid"].mean(axis=1)[:, None], res["grad"].mean(axis=1)], axis=1)


def check_long_rows_grad_philox(be, N, K, report=None):
    """Rows of more than 64 tiles in the row-mean kernel (K = 4096: one tile per lane; 4097, 8193: a second and third step of the
    strided loop), C = 3 with a NaN row, both draw modes, all four outputs: fid, grad, mean = the bits of the two-kernel route;
    mean and moment within K 2^-52 max(1, max |entry|) of host sums of the same launch's per-sample outputs; the same bits on a
    second run and from the launches that write row sums only."""
    ctrl = philox_ctrl(N)
    a, b, offset, ok = 0, N - 1, 7, [0, 2]
    for shared in (False, True):
        what = ("long rows", N, K, "shared" if shared else "per row")
        full = _fused(be, ctrl, K, N, a, b, offset, shared)
        assert_grad_teeth(full["grad"], what)
        assert all(np.isnan(full[k][1]).all() for k in PHILOX_OUTPUTS), what
        assert_same_bits(full, _two_kernels(be, ctrl, K, N, a, b, offset, shared), what, ("fid", "grad", "mean"))
        bound = K * EPS * max(1.0, float(np.abs(full["grad"][ok]).max()))
        e_mean = float(np.abs(full["mean"][ok] - host_means(full)[ok]).max())
        e_mom = float(np.abs(full["moment"][ok] - host_moments(full)[ok]).max())
        if report is not None:
            report(f"long rows, N = {N}, K = {K}, shared = {shared}: |mean - host| = {e_mean:.2e} ({e_mean / bound:.2e} of the bound), "
                   f"|moment - host| = {e_mom:.2e} ({e_mom / bound:.2e})")
        assert e_mean <= bound, (what, "mean against host sums", e_mean, bound)
        assert e_mom <= bound, (what, "moment against host sums", e_mom, bound)
        assert np.abs(host_moments(full)[ok, 1:]).max() > 1e-3 and host_moments(full)[ok, 0].min() > 1e-3, what
        assert_same_bits(_fused(be, ctrl, K, N, a, b, offset, shared), full, (what, "second run"), PHILOX_OUTPUTS)
        for sub in (("moment",), ("mean", "moment")):
            only = _fused(be, ctrl, K, N, a, b, offset, shared, want=sub)
            assert set(only) == set(sub), (what, sub)
            assert_same_bits(only, full, (what, sub), sub)


def check_far_offsets_grad_philox(be, N, K=130, worst=None):
    """Stream offsets whose pair counter has a non-zero high word (`FAR_OFFSET`) or carries into it inside the first tile
    (`wrap_offset`), both draw modes: the bits of the two-kernel route and inside the bars of grad_eigh on host-regenerated
    draws at the same offsets."""
    ctrl = philox_ctrl(N)
    for offset in (wrap_offset(N), FAR_OFFSET):
        for (a, b) in grad_pairs(N)[:2]:
            for shared in (False, True):
                what = ("far offset", N, a, b, offset, "shared" if shared else "per row")
                draws, Fw, Gw = reference_on_host_draws(ctrl, K, N, a, b, offset, shared)
                assert_grad_teeth(Gw, what)
                got = _fused(be, ctrl, K, N, a, b, offset, shared)
                assert_same_bits(got, _two_kernels(be, ctrl, K, N, a, b, offset, shared), what, ("fid", "grad", "mean"))
                out = _compare_with_reference(got, ctrl, draws, Fw, Gw, N, None, None, what)
                if worst is not None:
                    worst.add(("far offset", N), out)
