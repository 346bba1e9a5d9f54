"""Workloads with a known, non-trivial answer for the ring and the non-Hermitian fidelity kernels, and the data-level checks
built on them (the chain counterpart is tests/chain_checks.py, whose bounds and comparisons are reused here).

`gpu_common.rand_ctrl`'s biases U(-10, 10) localise the excitation: on a ring the far pairs have fidelities of 1e-9 ... 1e-5
and the directional entry's end-to-end pair ~1e-9, so an absolute 1e-10 bound passes a kernel that returns zeros.  Here:

  A  `flux_ring`          every chain bond e^{i theta}, corner 1: flux Phi = (N - 1) theta, plane waves in closed form
  B  `cut_ring`           one chain bond cut exactly: the spin-j chain of chain_checks, walked round the ring from the cut
  C  `complex_field_chain` the spin-j chain in a COMPLEX field g (non-Hermitian; SL(2, C) closed form, Jordan block at g = i lam)
  D  `directional_gauge`   the spin-j chain through the directional entry, every direction, pure-phase (gauge-only) samples
  E  A with a uniform imaginary diagonal gamma: F = exp(2 gamma T) F_A
  and delocalised rings (`deloc_ring_ctrl`) and directional rows against the oracle.

The `check_*` functions take a backend object (`code-robchar_amd.backend` on the GPU, tests/stand_in.py or a broken stand-in
on the CPU) and raise AssertionError on a wrong answer."""
import contextlib
from math import comb

import numpy as np

from chain_checks import (BIG, REL, TOL, _teeth_compare, assert_has_teeth, closed_form_ctrl, closed_form_fid,
                          closed_form_offdiag, compare, oracle_pairs)
from oracle import robchar_oracle as orc

RING_KERNELS = ("auto", "ring_hh", "jacobi", "expm")
FLUXES = (np.pi / 2, 0.0)              # pi / 2: every level pair well apart; 0: exactly degenerate pairs k <-> -k
NH_TOL = 1e-9                          # non-Hermitian bound, relative to S = max(1, max_out F(in -> out)), |Im g| <= 0.5
NH_TOL_EP = 1e-7                       # ... at and near the exceptional point (Im g >= 0.9)


# ------------------------------------------------------------------------------------------------------------------------
# A. flux ring: h0_offdiag = cos theta, draws[..., i, 2] = sin theta (i >= 1): every chain bond H[i, i - 1] = e^{i theta}, the
# corner H[N - 1, 0] = 1, flux Phi = (N - 1) theta.  With a uniform bias the eigenvectors are plane waves:
# F(a -> b) = |(1/N) sum_m exp(i q_m (b - a) - 2 i T cos q_m)|^2, q_m = (2 pi m - Phi) / N.  Odd N tells Phi from -Phi (a
# conjugated coupling, a swapped in / out); even N does not (the ring is bipartite).
# ------------------------------------------------------------------------------------------------------------------------


def flux_ring_fid(N, phi, T, a, b):
    q = (2.0 * np.pi * np.arange(N) - phi) / N
    amp = np.exp(1j * q * (b - a) - 2j * np.abs(np.asarray(T, dtype=np.float64))[:, None] * np.cos(q)).sum(axis=1) / N
    return amp.real ** 2 + amp.imag ** 2


def flux_ring(N, phi, K=2, rows=10, seed=0):
    """(ctrl, h0_offdiag, draws) of the flux ring: one uniform bias per row, T from 0.3 to 0.45 N (one row negative)."""
    rng = np.random.default_rng(seed)
    theta = phi / (N - 1)
    ctrl = np.empty((rows, N + 1))
    ctrl[:, :N] = rng.uniform(-1.0, 1.0, rows)[:, None]
    ctrl[:, N] = np.linspace(0.3, 0.45 * N, rows)
    ctrl[rows // 2, N] *= -1.0                                  # the kernels take |T|
    draws = np.zeros((rows, K, N, 3))
    draws[..., 1:, 2] = np.sin(theta)
    return ctrl, np.full(N - 1, np.cos(theta)), draws


# ------------------------------------------------------------------------------------------------------------------------
# B. cut ring: cut chain bond k = N // 2 (sites k - 1, k) exactly, either through h0_offdiag[k - 1] = 0 or through
# h0_offdiag[k - 1] = 1 and draws[..., k, 1] = -1.  What is left is a chain from site k round the ring to site k - 1: position
# p = site (k + p) mod N.  Biases g ((N - 1) / 2 - p) and bond magnitudes J_p = (lam / 2) sqrt((p + 1)(N - 1 - p)) with
# lam = 2 / sqrt(k (N - k)) make it the spin-j chain of chain_checks (the fixed corner sits at p = N - 1 - k, where J_p = 1);
# the magnitudes go into h0_offdiag (non-unit), a random phase per sample into the draws (a gauge on an open chain).
# ------------------------------------------------------------------------------------------------------------------------


def cut_ring(N, cut="h0", phases=True, K=3, gs=(0.05, -0.3), nT=12, seed=0):
    """(ctrl (site order), h0_offdiag, draws, positions ctrl, k, lam): rows of `closed_form_ctrl` on a T grid up to pi / lam."""
    rng = np.random.default_rng(seed)
    k = N // 2
    lam = 2.0 / np.sqrt(k * (N - k))
    pos_ctrl = closed_form_ctrl(N, gs, np.linspace(0.0, np.pi / lam, nT))
    ctrl = np.empty_like(pos_ctrl)
    ctrl[:, (k + np.arange(N)) % N] = pos_ctrl[:, :N]
    ctrl[:, N] = pos_ctrl[:, N]
    C = ctrl.shape[0]
    off = np.empty(N - 1)
    draws = np.zeros((C, K, N, 3))
    for i in range(1, N):
        if i == k:
            off[i - 1] = 0.0 if cut == "h0" else 1.0
            if cut != "h0":
                draws[..., i, 1] = -1.0
            continue
        p = (i - 1 - k) % N
        J = 0.5 * lam * np.sqrt((p + 1) * (N - 1 - p))
        off[i - 1] = J
        if phases:
            phi = rng.uniform(-np.pi, np.pi, (C, K))
            draws[..., i, 1], draws[..., i, 2] = J * (np.cos(phi) - 1.0), J * np.sin(phi)
    if phases:
        draws[..., 0, 1:] = rng.standard_normal((C, K, 2))      # drawn and dropped by the model (bond 0 does not exist)
    return ctrl, off, draws, pos_ctrl, k, lam


# ------------------------------------------------------------------------------------------------------------------------
# C. the spin-j chain in a complex field g = g_r + i g_i: h0_offdiag = closed_form_offdiag(N), biases g_r ((N - 1) / 2 - n),
# diag_imag g_i ((N - 1) / 2 - n), no draws: H = lam Jx + g Jz.  The spin-j representation extends to SL(2, C): with
# (P, Q) and (Q, R) the columns of exp(-i T / 2 (lam sx + g sz)),
# F(0 -> n) = C(N - 1, n) |P|^(2 (N - 1 - n)) |Q|^(2 n),  F(N - 1 -> n) = C(N - 1, n) |Q|^(2 (N - 1 - n)) |R|^(2 n).
# At g = i lam, H is one nilpotent N x N Jordan block (an exceptional point of size N).
# ------------------------------------------------------------------------------------------------------------------------

CSYM_GS = (0.3 + 0.2j, -0.1 + 0.5j, 0.3j, 0.9j, 0.999j, 1j, 1.2j)


def complex_field_chain(N, gs=CSYM_GS, nT=8, K=1):
    """(ctrl, h0_offdiag, draws, diag_imag, g per row): T from 0 to pi for every g."""
    gs = np.asarray(gs, dtype=np.complex128)
    ctrl = closed_form_ctrl(N, gs.real, np.linspace(0.0, np.pi, nT))
    g = np.repeat(gs, nT)
    imag = np.broadcast_to((g.imag[:, None] * ((N - 1) / 2 - np.arange(N)))[:, None, :], (len(g), K, N)).copy()
    return ctrl, closed_form_offdiag(N), np.zeros((len(g), K, N, 3)), imag, g


def complex_field_fid(N, g, T, a, b, lam=1.0):
    if a not in (0, N - 1):
        raise ValueError("the closed form is for transfers from an end of the chain")
    g = np.asarray(g, dtype=np.complex128)
    T = np.abs(np.asarray(T, dtype=np.float64))
    om = np.sqrt(lam * lam + g * g)
    zero = om == 0
    s = np.where(zero, T / 2, np.sin(om * T / 2) / np.where(zero, 1.0, om))
    P = np.cos(om * T / 2) - 1j * g * s
    Q = -1j * lam * s
    R = np.cos(om * T / 2) + 1j * g * s
    if a == 0:
        return comb(N - 1, b) * np.abs(P) ** (2 * (N - 1 - b)) * np.abs(Q) ** (2 * b)
    return comb(N - 1, b) * np.abs(Q) ** (2 * (N - 1 - b)) * np.abs(R) ** (2 * b)


# ------------------------------------------------------------------------------------------------------------------------
# D. directional entry, gauge-only samples: the spin-j chain (real g), every direction index; a diagonal direction gets
# (a, b) = (0, 0), a bond direction a pure phase J (cos phi - 1, +-sin phi) that turns the coupling without changing its size.
# ------------------------------------------------------------------------------------------------------------------------


def directional_gauge(N, seed=0):
    """(ctrl, h0_offdiag, idx (C K,) int32, ab (C K, 2), K): row c, sample j takes direction (j + c) mod ndir."""
    rng = np.random.default_rng(seed)
    ctrl = closed_form_ctrl(N, (0.05, -0.3), np.linspace(0.0, np.pi, 8))
    off = closed_form_offdiag(N)
    dirs = orc.directional_directions(N)
    C, K = ctrl.shape[0], len(dirs) + 5                                  # every direction in every row, no round K
    idx = ((np.arange(K)[None, :] + np.arange(C)[:, None]) % len(dirs)).reshape(-1).astype(np.int32)
    ab = np.zeros((C * K, 2))
    for s, d in enumerate(idx):
        p, q = dirs[d]
        if p != q:
            J, phi = off[min(p, q)], rng.uniform(-np.pi, np.pi)
            ab[s] = J * (np.cos(phi) - 1.0), J * np.sin(phi) * rng.choice((-1.0, 1.0))
    return ctrl, off, idx, ab, K


def directional_layout(N, idx, ab, C, K):
    """(draws (C, K, N, 3), diag_imag (C, K, N)) of directional samples: the oracle's per-sample layout"""
    draws, imag = np.zeros((C * K, N, 3)), np.zeros((C * K, N))
    for s in range(C * K):
        draws[s], imag[s] = orc.directional_to_layout(N, int(idx[s]), float(ab[s, 0]), float(ab[s, 1]))
    return draws.reshape(C, K, N, 3), imag.reshape(C, K, N)


def deloc_ring_ctrl(rng, C, N, W):
    """C DELOCALISED ring controller rows: biases U(-W, W), T ~ U(0.25 N, 0.4 N).  At sigma = 0.05: median F >= 1e-2 and
    >= 93 % of the samples above 1e-3 for N = 3 ... 16 and the pairs (0, N - 1), (0, N // 2), (N - 1, 1), (1, 1)."""
    x = np.empty((C, N + 1))
    x[:, :N] = rng.uniform(-W, W, (C, N))
    x[:, N] = rng.uniform(0.25 * N, 0.4 * N, C)
    return x


# ------------------------------------------------------------------------------------------------------------------------
# bounds for non-Hermitian results (F may exceed 1 by orders of magnitude)
# ------------------------------------------------------------------------------------------------------------------------


def compare_nh(got, want, scale, bound, rel_rows, what):
    """|got - want| <= bound * scale per sample (scale = max(1, max_out F) of its row, broadcast), REL where F > BIG * scale on
    the rows of `rel_rows`; NaN exactly where the reference has NaN.  Returns (max abs / scale, max rel, share F > BIG scale)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = np.broadcast_to(scale, want.shape)
    bound = np.broadcast_to(bound, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    err = np.where(nan, 0.0, np.abs(got - want)) / scale
    assert (err <= bound).all(), (what, float(err.max()), np.argwhere(err > bound)[:4].tolist())
    big = ~nan & (want > BIG * scale) & np.broadcast_to(np.asarray(rel_rows)[:, None], want.shape)
    rel = float((np.abs(got - want)[big] / want[big]).max()) if big.any() else 0.0
    assert rel < REL, (what, rel)
    return float(err.max()), rel, float(big.mean())


# ------------------------------------------------------------------------------------------------------------------------
# checks (backend in, assertion out)
# ------------------------------------------------------------------------------------------------------------------------


def _ends_to_every_site(be, N, ctrl, off, draws, wants, kernels, worst, tag, **kw):
    for kern in kernels:
        for a, b in wants:
            got = be.mc_fidelity(ctrl, draws, N, a, b, h0_offdiag=off, ring=True, kernel=kern, **kw)
            res = compare(got, wants[a, b], (N, a, b, kern, tag))
            if worst is not None:
                worst.add(kern, res)


def flux_ring_wants(N, phi, ctrl, K):
    return {(a, b): np.repeat(flux_ring_fid(N, phi, ctrl[:, N], a, b)[:, None], K, axis=1) for a in (0, N - 1) for b in range(N)}


def check_flux_ring(be, N, worst=None, fluxes=FLUXES, kernels=RING_KERNELS):
    """A: the flux ring at Phi = pi / 2 and Phi = 0, every ring kernel, from both ends to every site."""
    for phi in fluxes:
        ctrl, off, draws = flux_ring(N, phi, seed=N)
        wants = flux_ring_wants(N, phi, ctrl, draws.shape[1])
        assert_has_teeth(np.concatenate(list(wants.values())), median=0.02, share=0.5, what=(N, phi))
        _ends_to_every_site(be, N, ctrl, off, draws, wants, kernels, worst, ("flux", phi))


CUT_VARIANTS = (("h0", True), ("draw", True), ("h0", False))


def check_cut_ring(be, N, worst=None, variants=CUT_VARIANTS, kernels=RING_KERNELS):
    """B: a ring with one bond cut exactly (through h0_offdiag, or cancelled by the draws) = the spin-j chain, non-unit
    h0_offdiag, random per-sample phases; every ring kernel, from both ends of the cut chain to every site."""
    for cut, phases in variants:
        ctrl, off, draws, pos_ctrl, k, lam = cut_ring(N, cut, phases, seed=N)
        K = draws.shape[1]
        wants = {}
        for ap in (0, N - 1):
            for bp in range(N):
                wants[(k + ap) % N, (k + bp) % N] = np.repeat(closed_form_fid(N, pos_ctrl, ap, bp, lam=lam)[:, None], K, axis=1)
            assert_has_teeth(np.concatenate([wants[(k + ap) % N, (k + bp) % N] for bp in range(N)]), median=0, share=0.3,
                             what=(N, cut, ap))
        assert wants[k, (k - 1) % N].max() > 0.5, (N, "transfer across the cut")
        _ends_to_every_site(be, N, ctrl, off, draws, wants, kernels, worst, ("cut", cut, phases))


def _side_stream(be):
    """a fresh side stream on a GPU backend (released on exit); nothing on a CPU stand-in"""
    if be.compute_device().type == "cuda":
        return be.ring_stream()
    return contextlib.nullcontext()


def check_ring_deloc(be, N, worst=None, kernels=RING_KERNELS):
    """Delocalised rings against the oracle, every ring kernel: every class of (in, out) both ways, XXZ offsets, a NaN row,
    ragged K, one draw set shared by every controller, the torch entry on a fresh side stream."""
    import torch
    rng = np.random.default_rng(19000 + N)
    C, K = 6, 130                                                        # 2 full tiles + 2 lanes per controller
    ctrl = np.concatenate([deloc_ring_ctrl(rng, 1, N, W) for W in (0.2, 0.5, 1.0, 0.5, 0.7, 0.3)])
    ctrl[2, N - 1] = np.nan                                              # a padded controller row
    draws = 0.05 * rng.standard_normal((C, K, N, 3))
    pairs = sorted({(0, N - 1), (N - 1, 0), (0, N // 2), (N // 2, 0), (N - 1, 1), (1, N - 1), (1, 1)})
    wants = oracle_pairs(ctrl, draws, N, pairs, ring=True)
    h0 = orc.xxz_delta(N, ring=True)
    want_xxz = oracle_pairs(ctrl, draws, N, [(0, N // 2)], h0_diag=h0, ring=True)[0, N // 2]
    for kern in kernels:
        for (a, b) in pairs:
            got = be.mc_fidelity(ctrl, draws, N, a, b, ring=True, kernel=kern)
            _teeth_compare(got, wants[a, b], (N, a, b, kern, "ring"), worst, kern)
        got = be.mc_fidelity(ctrl, draws, N, 0, N // 2, h0_diag=h0, ring=True, kernel=kern)
        _teeth_compare(got, want_xxz, (N, "ring xxz", kern), worst, kern)
    for K2 in (1, 63, 64, 65, 150):                                      # a lone lane, one short of a tile, a tile, one over, ...
        c2 = deloc_ring_ctrl(rng, 3, N, 0.5)
        d2 = 0.05 * rng.standard_normal((3, K2, N, 3))
        want = oracle_pairs(c2, d2, N, [(0, N // 2)], ring=True)[0, N // 2]
        for kern in kernels:
            got = be.mc_fidelity(c2, d2, N, 0, N // 2, ring=True, kernel=kern)
            _teeth_compare(got, want, (N, "ring K", K2, kern), worst, kern, median=1e-3, share=0.5 if K2 > 1 else 0.0)
    shared = 0.05 * rng.standard_normal((1, 65, N, 3))
    c3 = deloc_ring_ctrl(rng, 4, N, 0.5)
    want = oracle_pairs(c3, np.broadcast_to(shared, (4,) + shared.shape[1:]), N, [(N - 1, 1)], ring=True)[N - 1, 1]
    dev = be.compute_device()
    for kern in kernels:
        got = be.mc_fidelity(c3, shared, N, N - 1, 1, ring=True, kernel=kern)
        _teeth_compare(got, want, (N, "ring shared draws", kern), worst, kern)
    ct, dt = torch.from_numpy(ctrl).to(dev), torch.from_numpy(draws).to(dev)
    with _side_stream(be) as st:
        if st is not None:
            st.wait_stream(torch.cuda.default_stream(dev))
        got_t = be.mc_fidelity(ct, dt, N, N - 1, 0, ring=True)
        if st is not None:
            st.synchronize()
        got = got_t.cpu().numpy()
    _teeth_compare(got, wants[N - 1, 0], (N, "ring torch side stream"), worst, "auto")


def check_flux_ring_product(noise, N, phi=np.pi / 2, worst=None, conjugate=False):
    """The product surface: `structured_perturbation(topo="ring")` with `HH`'s chain bonds edited to e^{i theta} - the
    couplings reach the kernel as h0_offdiag (real part) plus draws (imaginary part, noise._static_terms) - and zero draws: A.
    (`conjugate`: edit `HH` with e^{-i theta} instead and still expect +Phi - a check of the check.)"""
    ctrl, _, draws = flux_ring(N, phi, seed=N)
    theta = (-phi if conjugate else phi) / (N - 1)
    for (a, b) in ((0, N - 1), (N - 1, 0), (0, N // 2), (1, 1)):
        nm = noise.structured_perturbation(Nspin=N, inspin=a, outspin=b, noise=0.05, topo="ring")
        i = np.arange(1, N)
        nm.HH[i, i - 1] = np.exp(1j * theta)
        nm.HH[i - 1, i] = np.exp(-1j * theta)
        got = nm.fidelity_from_draws(ctrl, np.zeros_like(draws))
        want = np.repeat(flux_ring_fid(N, phi, ctrl[:, N], a, b)[:, None], draws.shape[1], axis=1)
        res = compare(got, want, (N, a, b, "structured_perturbation ring, flux"))
        if worst is not None:
            worst.add("noise.fidelity_from_draws", res)


def check_complex_field(be, N, worst=None, route="csym"):
    """C: the spin-j chain in a complex field through `mc_fidelity_nonhermitian`, from both ends to every site."""
    ctrl, off, draws, imag, g = complex_field_chain(N)
    ep = g.imag >= 0.9
    bound = np.where(ep, NH_TOL_EP, NH_TOL)[:, None]
    for a in (0, N - 1):
        wants = {b: complex_field_fid(N, g, ctrl[:, N], a, b)[:, None] for b in range(N)}
        scale = np.maximum(1.0, np.max([w[:, 0] for w in wants.values()], axis=0))[:, None]
        assert_has_teeth(np.concatenate([w / scale for w in wants.values()]), median=0, share=0.2, what=(N, a))
        for b in range(N):
            got = be.mc_fidelity_nonhermitian(ctrl, draws, imag, N, a, b, h0_offdiag=off)
            res = compare_nh(got, wants[b], scale, bound, np.abs(g.imag) <= 0.5, (N, a, b, route, "complex field"))
            if worst is not None:
                worst.add(route, res)


def check_flux_ring_nh(be, N, worst=None, gammas=(0.07, -0.05)):
    """E: the flux ring with a uniform imaginary diagonal through `mc_fidelity_nonhermitian(ring=True)`: e^{2 gamma T} F_A."""
    ctrl, off, draws = flux_ring(N, np.pi / 2, seed=N)
    C, K = draws.shape[:2]
    for gamma in gammas:
        imag = np.full((C, K, N), gamma)
        growth = np.exp(2.0 * gamma * np.abs(ctrl[:, N]))[:, None]
        wants = {(a, b): growth * flux_ring_fid(N, np.pi / 2, ctrl[:, N], a, b)[:, None] for a in (0, N - 1) for b in range(N)}
        for a in (0, N - 1):
            scale = np.maximum(1.0, np.max([wants[a, b][:, 0] for b in range(N)], axis=0))[:, None]
            for b in range(N):
                got = be.mc_fidelity_nonhermitian(ctrl, draws, imag, N, a, b, h0_offdiag=off, ring=True)
                res = compare_nh(got, np.repeat(wants[a, b], K, axis=1), scale, NH_TOL, np.ones(C, bool),
                                 (N, a, b, gamma, "flux ring nh"))
                if worst is not None:
                    worst.add("nh ring expm", res)


def _directional(be, ctrl, idx, ab, N, a, b, K, **kw):
    import torch
    dev = be.compute_device()
    got = be.mc_fidelity_directional(torch.from_numpy(ctrl).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(ab).to(dev),
                                     N, a, b, K, **kw)
    return got.cpu().numpy()


def check_directional_gauge(be, N, worst=None):
    """D: gauge-only directional samples of the spin-j chain, every direction in every row, both ends to every site."""
    ctrl, off, idx, ab, K = directional_gauge(N, seed=N)
    for a in (0, N - 1):
        wants = {b: np.repeat(closed_form_fid(N, ctrl, a, b)[:, None], K, axis=1) for b in range(N)}
        assert_has_teeth(np.concatenate(list(wants.values())), median=0, share=0.3, what=(N, a))
        for b in range(N):
            res = compare(_directional(be, ctrl, idx, ab, N, a, b, K, h0_offdiag=off), wants[b], (N, a, b, "directional gauge"))
            if worst is not None:
                worst.add("directional", res)


def check_directional_deloc(be, N, worst=None):
    """Delocalised directional rows against the oracle's per-sample expm: every direction, every class of (in, out) with T
    scaled to |out - in|, XXZ offsets and non-unit couplings, a NaN row, K = 173 and a ragged K = 65."""
    rng = np.random.default_rng(23000 + N)
    dirs = orc.directional_directions(N)
    for trial, (a, b) in enumerate(((0, N - 1), (N - 1, 0), (0, N // 2), (N // 2, N // 2), (min(1, N - 1), 0))):
        C, K = (5, 173) if trial != 4 else (3, 65)
        ctrl = np.empty((C, N + 1))
        ctrl[:, :N] = rng.uniform(-0.5, 0.5, (C, N))
        ctrl[:, N] = rng.uniform(0.5, 0.7, C) * max(abs(b - a), 1)
        ctrl[1] = np.nan
        idx = rng.integers(0, len(dirs), C * K).astype(np.int32)
        idx[:len(dirs)] = np.arange(len(dirs))
        ab = rng.standard_normal((C * K, 2)) * (0.05 if trial % 2 else 0.2)
        h0d = orc.xxz_delta(N) if trial in (1, 3) else None
        h0o = rng.uniform(0.7, 1.3, N - 1) if trial == 2 else None
        draws, imag = directional_layout(N, idx, ab, C, K)
        want = orc.fidelity_expm_loop(ctrl, draws, N, a, b, h0_diag=h0d, h0_offdiag=h0o, diag_imag=imag)
        assert_has_teeth(want, what=(N, a, b, "directional"))
        got = _directional(be, ctrl, idx, ab, N, a, b, K, h0_diag=h0d, h0_offdiag=h0o)
        res = compare_nh(got, want, np.maximum(1.0, np.nan_to_num(want)), TOL, np.ones(C, bool), (N, a, b, "directional deloc"))
        if worst is not None:
            worst.add("directional", res)
