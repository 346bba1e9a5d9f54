"""Workloads with a known, non-trivial answer for the chain fidelity kernels, the bounds they are held to, and the data-level
checks built on them.

`gpu_common.rand_ctrl`'s biases U(-10, 10) make Anderson-localised chains: end-to-end fidelities of 1e-15 ... 1e-26 at
N = 17 ... 32, where an absolute 1e-10 bound passes a kernel that returns zeros.  The workloads here have fidelities of order
one: delocalised controllers (`deloc_ctrl`) and the spin-j chain of `closed_form_*`, whose answer needs no eigensolver.
Every comparison first asks the reference whether it CAN fail (`assert_has_teeth`), then bounds the error in absolute and
relative terms (`compare`).

The `check_*` functions take a backend object (anything with `mc_fidelity` and `compute_device` like
`code-robchar_amd.backend`): the GPU tests run them on the device, and a CPU test runs them on the oracle stand-in
(tests/stand_in.py), where they must pass, and on deliberately broken stand-ins, where they must fail."""
from math import comb

import numpy as np

from oracle import robchar_oracle as orc

TOL = 1e-10          # absolute bound on every sample
REL = 1e-9           # relative bound on samples with F > BIG (measured on the device: ~1e-13)
BIG = 1e-3


def deloc_ctrl(rng, C, N, W):
    """C DELOCALISED controller rows for an N-spin chain: biases U(-W, W) (W = 0.2 ... 1, against the hopping J = 1) and
    T ~ U(0.5 N, 0.7 N), about the time an excitation needs to cross the chain.  At sigma = 0.05: median 0 -> N-1 fidelity
    0.01 ... 0.4 for N = 17 ... 32."""
    x = np.empty((C, N + 1))
    x[:, :N] = rng.uniform(-W, W, (C, N))
    x[:, N] = rng.uniform(0.5 * N, 0.7 * N, C)
    return x


# ------------------------------------------------------------------------------------------------------------------------
# closed form: h0_offdiag[n - 1] = (lam / 2) sqrt(n (N - n)), biases g ((N - 1) / 2 - n), no draws.  Then H = lam Jx + g Jz
# for spin j = (N - 1) / 2 with site n = the state m = j - n, and the transfer from an end is a rotation of the spin:
# F(0 -> n) = C(N - 1, n) ((1 + c) / 2)^(N - 1 - n) ((1 - c) / 2)^n,  c = nz^2 + (1 - nz^2) cos(Omega T),
# Omega = sqrt(lam^2 + g^2), nz = g / Omega; from N - 1 the same with n -> N - 1 - n (mirror symmetry).
# ------------------------------------------------------------------------------------------------------------------------


def closed_form_offdiag(N, lam=1.0):
    n = np.arange(1, N)
    return 0.5 * lam * np.sqrt(n * (N - n))


def closed_form_ctrl(N, gs, Ts):
    """One controller row per (g, T) pair (g outer, T inner): biases g ((N - 1) / 2 - n), transfer time T."""
    gs, Ts = np.atleast_1d(gs), np.atleast_1d(Ts)
    x = np.empty((len(gs) * len(Ts), N + 1))
    x[:, :N] = np.repeat(gs, len(Ts))[:, None] * ((N - 1) / 2 - np.arange(N))
    x[:, N] = np.tile(Ts, len(gs))
    return x


def closed_form_fid(N, ctrl, inspin, outspin, lam=1.0):
    """F(inspin -> outspin) of the rows of `closed_form_ctrl` (inspin = 0 or N - 1), in closed form."""
    if inspin not in (0, N - 1):
        raise ValueError("the closed form is for transfers from an end of the chain")
    g = (ctrl[:, 0] - ctrl[:, N - 1]) / (N - 1)
    T = np.abs(ctrl[:, N])
    om = np.hypot(lam, g)
    nz = g / om
    c = nz * nz + (1.0 - nz * nz) * np.cos(om * T)
    m = outspin if inspin == 0 else N - 1 - outspin
    return comb(N - 1, m) * ((1.0 + c) / 2.0) ** (N - 1 - m) * ((1.0 - c) / 2.0) ** m


# a T grid from the initial state (F(0 -> 0) = 1) to the first full transfer (F(0 -> N - 1) = 0.93 ... 0.96 for N <= 24 at
# g = 0.05): the fidelities span ~0 ... > 0.9 for every `out`
CF_GS = (0.05, -0.3)
CF_TS = np.linspace(0.0, np.pi, 12)


# ------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------


def assert_has_teeth(want, median=1e-2, share=0.5, what=""):
    """A comparison against `want` must be able to fail: its median fidelity is at least `median` and a share of at least
    `share` of the samples is above BIG (where the relative bound applies).  NaN samples (padded rows) are left out."""
    w = np.asarray(want, dtype=np.float64)
    w = w[~np.isnan(w)]
    assert w.size, ("no finite reference values", what)
    med, big = float(np.median(w)), float((w > BIG).mean())
    assert med >= median and big >= share, ("the reference cannot tell a wrong kernel from a right one", what, med, big)


def compare(got, want, what):
    """absolute bound everywhere, relative bound where the fidelity is not tiny, NaN exactly where the reference has NaN;
    returns (max abs, max rel, share F > BIG)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    got, want = got[~nan], want[~nan]
    err = np.abs(got - want)
    big = want > BIG
    rel = float((err[big] / want[big]).max()) if big.any() else 0.0
    assert err.max() < TOL, (what, float(err.max()))
    assert rel < REL, (what, rel)
    return float(err.max()), rel, float(big.mean())


class Worst:
    """worst (abs, rel) per route over the comparisons of a run - for the record (printed by the GPU tests)"""

    def __init__(self):
        self.by = {}

    def add(self, route, res):
        a, r = self.by.get(route, (0.0, 0.0))
        self.by[route] = (max(a, res[0]), max(r, res[1]))

    def __str__(self):
        return "; ".join(f"{k}: abs {a:.1e} rel {r:.1e}" for k, (a, r) in sorted(self.by.items()))


def _teeth_compare(got, want, what, worst=None, route=None, **teeth):
    assert_has_teeth(want, what=what, **teeth)
    res = compare(got, want, what)
    if worst is not None:
        worst.add(route, res)
    return res


def chain_kernels(N):
    """the kernels of the chain topology that accept N spins (the dense ones stop at 16)"""
    return ("auto", "tridiag_adj", "tridiag_ql") + (("jacobi", "expm") if N <= 16 else ())


# ------------------------------------------------------------------------------------------------------------------------
# checks (backend in, assertion out)
# ------------------------------------------------------------------------------------------------------------------------


def oracle_pairs(ctrl, draws, N, pairs, h0_diag=None, ring=False):
    """`orc.fidelity_eigh` for several (in, out) pairs of one workload: one eigendecomposition (the oracle's cost) for all"""
    ctrl = np.asarray(ctrl, dtype=np.float64)
    H = orc.assemble_hamiltonians(np.nan_to_num(ctrl), draws, N, h0_diag, ring=ring)
    lam, V = np.linalg.eigh(H)
    phase = np.exp(-1j * np.abs(np.nan_to_num(ctrl[:, N]))[:, None, None] * lam)
    res = {}
    for (a, b) in pairs:
        phi = (V[..., b, :] * np.conj(V[..., a, :]) * phase).sum(axis=-1)
        f = phi.real * phi.real + phi.imag * phi.imag
        f[np.isnan(ctrl).any(axis=1)] = np.nan
        res[a, b] = f
    return res


LONG_ROUTES = ("auto", "tridiag_adj", "tridiag_ql")


def check_long_chain(be, N, worst=None):
    """16 < N <= 32, every chain route (auto / tridiag_adj: the register-resident adjugate kernel for N <= 24; tridiag_ql and
    everything above 24: the LDS kernel) on delocalised controllers: pairs end to end both ways, interior, a = b; XXZ offsets;
    a NaN row; ragged K; one draw set shared by every controller; device-resident inputs."""
    import torch
    rng = np.random.default_rng(17000 + N)
    C, K = 4, 130                                                        # 2 full tiles + 2 lanes per controller
    ctrl = np.concatenate([deloc_ctrl(rng, 1, N, W) for W in (0.2, 0.5, 1.0, 0.5)])
    ctrl[2, 3] = np.nan                                                  # a padded controller row
    draws = 0.05 * rng.standard_normal((C, K, N, 3))
    pairs = ((0, N - 1), (N - 1, 0), (2, N // 2), (N // 2, N // 2))
    wants = oracle_pairs(ctrl, draws, N, pairs)
    h0 = orc.xxz_delta(N)
    wants_xxz = oracle_pairs(ctrl, draws, N, [(0, N - 1)], h0_diag=h0)
    for kern in LONG_ROUTES:
        for (a, b) in pairs:
            got = be.mc_fidelity(ctrl, draws, N, a, b, kernel=kern)
            _teeth_compare(got, wants[a, b], (N, a, b, kern), worst, kern)
        got = be.mc_fidelity(ctrl, draws, N, 0, N - 1, h0_diag=h0, kernel=kern)
        _teeth_compare(got, wants_xxz[0, N - 1], (N, "xxz", kern), worst, kern)
    # ragged K: a lone lane, one short of a tile, a tile, one over, 2 tiles + 22
    for K2 in (1, 63, 64, 65, 150):
        c2 = deloc_ctrl(rng, 2, N, 0.5)
        d2 = 0.05 * rng.standard_normal((2, K2, N, 3))
        want = oracle_pairs(c2, d2, N, [(0, N - 1)])[0, N - 1]
        for kern in LONG_ROUTES:
            got = be.mc_fidelity(c2, d2, N, 0, N - 1, kernel=kern)
            _teeth_compare(got, want, (N, "K", K2, kern), worst, kern, median=1e-3, share=0.5 if K2 > 1 else 0.0)
    # one draw set for every controller (the optimiser-side objective: draws of shape (1, K, N, 3)), numpy and device-resident
    shared = 0.05 * rng.standard_normal((1, 65, N, 3))
    c3 = deloc_ctrl(rng, 4, N, 0.5)
    want = oracle_pairs(c3, np.broadcast_to(shared, (4,) + shared.shape[1:]), N, [(0, N - 1)])[0, N - 1]
    dev = be.compute_device()
    for kern in LONG_ROUTES:
        got = be.mc_fidelity(c3, shared, N, 0, N - 1, kernel=kern)
        _teeth_compare(got, want, (N, "shared draws", kern), worst, kern)
        got_t = be.mc_fidelity(torch.from_numpy(c3).to(dev), torch.from_numpy(shared.copy()).to(dev), N, 0, N - 1, kernel=kern)
        _teeth_compare(got_t.cpu().numpy(), want, (N, "shared draws, torch", kern), worst, kern)
    # the torch entry (the *_async path on the current stream) with a NaN row and a ragged tile
    got_t = be.mc_fidelity(torch.from_numpy(ctrl).to(dev), torch.from_numpy(draws).to(dev), N, N - 1, 0)
    _teeth_compare(got_t.cpu().numpy(), wants[N - 1, 0], (N, "torch"), worst, "auto")


def check_closed_form(be, N, worst=None):
    """The spin-j chain (non-unit h0_offdiag, no draws) from both ends to every site, every kernel that accepts N, on a T
    grid whose fidelities span ~0 ... > 0.9, against the closed form."""
    ctrl = closed_form_ctrl(N, CF_GS, CF_TS)
    off = closed_form_offdiag(N)
    draws = np.zeros((ctrl.shape[0], 2, N, 3))
    ends = (0, N - 1)
    wants = {(a, b): np.repeat(closed_form_fid(N, ctrl, a, b)[:, None], 2, axis=1) for a in ends for b in range(N)}
    for a in ends:
        # the T grid runs every site's fidelity through its maximum; over all sites the grid is what must have teeth
        assert_has_teeth(np.concatenate([wants[a, b] for b in range(N)]), median=0, share=0.3, what=(N, a))
        assert wants[a, N - 1 - a].max() > 0.9, (N, a)                     # the full transfer to the other end
    for kern in chain_kernels(N):
        for a in ends:
            for b in range(N):
                got = be.mc_fidelity(ctrl, draws, N, a, b, h0_offdiag=off, kernel=kern)
                want = wants[a, b]
                res = compare(got, want, (N, a, b, kern, "closed form"))
                if worst is not None:
                    worst.add(kern, res)


def check_deloc_vs_oracle(be, N, worst=None):
    """2 <= N <= 16: delocalised rows (W = 0.5, T ~ N / 2) end to end and inside the chain, ragged K, XXZ offsets."""
    rng = np.random.default_rng(2100 + N)
    C, K = 6, 193
    ctrl = deloc_ctrl(rng, C, N, 0.5)
    draws = 0.05 * rng.standard_normal((C, K, N, 3))
    draws[:, :3] = 0.0
    for (a, b, h) in ((0, N - 1, None), (N // 2, max(0, N // 2 - 1), orc.xxz_delta(N))):
        want = orc.fidelity_eigh(ctrl, draws, N, a, b, h0_diag=h)
        got = be.mc_fidelity(ctrl, draws, N, a, b, h0_diag=h)
        _teeth_compare(got, want, (N, a, b, h is not None), worst, "auto")


def deloc_configs(seed, n=6):
    """Random (N <= 32, in, out, sigma, K) on delocalised rows, T scaled to the distance |out - in| (measured over 240 such
    configurations: median fidelity >= 0.015 in every one)."""
    rng = np.random.default_rng(31000 + seed)
    for _ in range(n):
        N = int(rng.integers(2, 33))
        if rng.random() < 0.5:
            a, b = 0, N - 1
        else:                                                    # anywhere in the chain, up to 3 sites apart
            a = int(rng.integers(0, N))
            b = int(np.clip(a + rng.integers(-3, 4), 0, N - 1))
        C, K = int(rng.integers(1, 6)), int(rng.integers(1, 200))
        sigma = float(rng.choice([0.0, 0.01, 0.05]))
        W = float(rng.choice([0.2, 0.5]))
        ctrl = deloc_ctrl(rng, C, N, W)
        ctrl[:, N] = rng.uniform(0.5, 0.7, C) * max(abs(b - a), 1)      # about the crossing time of |b - a| sites
        draws = sigma * rng.standard_normal((C, K, N, 3))
        h0 = orc.xxz_delta(N) if rng.random() < 0.3 else None
        yield N, a, b, ctrl, draws, h0


def check_random_deloc_configs(be, seed, worst=None):
    for (N, a, b, ctrl, draws, h0) in deloc_configs(seed):
        want = orc.fidelity_eigh(ctrl, draws, N, a, b, h0_diag=h0)
        assert_has_teeth(want, what=(seed, N, a, b))
        for kern in chain_kernels(N):
            got = be.mc_fidelity(ctrl, draws, N, a, b, h0_diag=h0, kernel=kern)
            res = compare(got, want, (seed, N, a, b, kern))
            if worst is not None:
                worst.add(kern, res)
