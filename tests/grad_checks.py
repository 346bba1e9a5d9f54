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
from oracle import robchar_oracle as orc

TOL = cc.TOL


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


class StandIn:
    """`mc_fidelity_grad` / `mc_fidelity` of the backend on the CPU.  broken: None, "zeros", "time_sign" (sign of the time
    entry dropped for negative x_N), "reversed" (bias entries in reversed order), "gamma_diag" (Gam_jk = Gam_kk)."""

    def __init__(self, broken=None):
        self.broken = broken

    def mc_fidelity(self, ctrl, draws, N, a, b, h0_diag=None, h0_offdiag=None, kernel="auto"):
        return grad_eigh(ctrl, draws, N, a, b, h0_diag, h0_offdiag)[0]

    def mc_fidelity_grad(self, ctrl, draws, N, a, b, h0_diag=None, h0_offdiag=None, device=None, want=("fid", "grad", "mean")):
        ctrl = np.asarray(ctrl, dtype=np.float64)
        F, G = grad_eigh(ctrl, draws, N, a, b, h0_diag, h0_offdiag, gamma_diag_only=self.broken == "gamma_diag")
        if self.broken == "zeros":
            G = np.where(np.isnan(G), G, 0.0)
        elif self.broken == "time_sign":
            G[..., N] = np.sign(ctrl[:, N])[:, None] * G[..., N]          # = 2 Re(conj(phi) dphi/dT) without the sign
        elif self.broken == "reversed":
            G[..., :N] = G[..., :N][..., ::-1]
        res = {}
        if "fid" in want:
            res["fid"] = F
        if "grad" in want:
            res["grad"] = G
        if "mean" in want:
            res["mean"] = np.concatenate([F.mean(axis=1)[:, None], G.mean(axis=1)], axis=1) if F.shape[1] else np.zeros((F.shape[0], N + 2))
        return res


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
    time entry; pairs end to end both ways, interior, in == out; a ragged K = 100 case; XXZ offsets."""
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
