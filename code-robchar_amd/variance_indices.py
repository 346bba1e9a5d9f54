"""Variance-based noise sensitivity indices of the fidelity by the pick-freeze scheme - the DEFINITION (NumPy only) the device
entry `backend.mc_fidelity_pickfreeze_philox` (`rc_mc_fidelity_pickfreeze_philox_f64_async`) is held to.

For a group g of noise coordinates the variance decomposition of F over the structured noise z gives

    first-order index   S_g  = Var(E[F | z_g]) / Var F         what z_g explains on its own,
    total-order index   ST_g = E[Var(F | z_~g)] / Var F        what is lost when z_g alone is fixed: S_g plus every interaction,

(the textbook name: Sobol' indices; in this tree "Sobol" means the quasi-random points of sobol.py, so the feature is called
*variance indices* / *pick-freeze* everywhere).

Draw layout and groups.  Coordinate j = 3 i + s of a sample is slot s of site i in the draw layout [N][3] (s = 0 site energy g0_i,
s = 1 / 2 real / imaginary coupling g1_i / g2_i of the sites i - 1, i); j = 1, 2 are the drawn-and-dropped g1_0, g2_0.  A group is
a uint64 mask over the 3 N coordinates: bits >= 3 N must be zero, bits 1 and 2 are allowed and have no effect on F.

The two draw vectors.  Per sample (c, k):  a = elements offset_a + ((c K + k) N + i) 3 + s of the counter-based stream `seed`
scaled by sigma (exactly the draws of `mc_fidelity_philox`),  b = the same with offset_b.  The two element ranges
[offset, offset + C K 3N) must be disjoint, compared as distances modulo 2^64 (a wrapping offset is legal).

Hybrids and fidelities.  h_g = where(mask_g, b, a) - a copy of bits -, fA = F(a), fB = F(b), f_g = F(h_g).

Row means (Jansen's estimators), mean[c][3 + 2 G]:  mean fA, mean fB, D = mean (fA - fB)^2 and per group
T_g = mean (fA - f_g)^2, U_g = mean (fB - f_g)^2: every term a difference rounded once, then a square rounded once; all sums are
of non-negative terms (the cancelling form sum f^2 - (sum f)^2 / K is never used).

Indices.  var = D / 2, total_g = T_g / D, first_g = 1 - U_g / D;  D == 0 (a sigma = 0 row: fA == fB bit for bit) gives var = 0
and NaN indices; a NaN controller row gives NaN everywhere.
"""
from __future__ import annotations

import math

import numpy as np

MAX_NSPIN = 13                       # RC_MAX_NSPIN_PICKFREEZE: limit of the fused kernel (the definition itself has none below 21)
MAX_GROUPS = 64                      # RC_PICKFREEZE_MAX_GROUPS
GROUP_KINDS = ("direction", "kind", "site")
_U64 = 2 ** 64


def coordinate(site: int, slot: int) -> int:
    """Coordinate j = 3 i + s of slot s of site i."""
    return 3 * int(site) + int(slot)


def mask_of(coordinates) -> int:
    """The group mask with the bits of `coordinates` set."""
    m = 0
    for j in coordinates:
        m |= 1 << int(j)
    return m


def check_groups(groups, nspin: int) -> np.ndarray:
    """`groups` as a (G,) uint64 array; raises on more than MAX_GROUPS groups or a bit at or above 3 N."""
    g = [int(m) for m in (groups.reshape(-1).tolist() if isinstance(groups, np.ndarray) else list(groups))]
    if len(g) > MAX_GROUPS:
        raise ValueError(f"groups: at most {MAX_GROUPS} per call, got {len(g)}")
    for i, m in enumerate(g):
        if m < 0 or m >> (3 * int(nspin)):
            raise ValueError(f"groups[{i}] = {m:#x}: a mask bit at or above 3 N = {3 * int(nspin)}")
    return np.array(g, dtype=np.uint64)


def direction_groups(nspin: int):
    """The 3 N - 2 single coordinates F depends on, in the order `noise.directional_perturbation` lists its directions: a
    diagonal element (i, i) is the site energy g0_i; an off-diagonal (p, q) belongs to the bond below site max(p, q), whose first
    mention is the real coupling g1 and whose second (the transposed element) the imaginary coupling g2 -> (masks, labels)."""
    n = int(nspin)
    directions = [(0, 0), (n - 1, n - 1)]
    for d in range(1, n - 1):
        for o in (-1, 0, 1):
            directions.append((d, d + o))
    directions += [(0, 1), (1, 0), (n - 2, n - 1), (n - 1, n - 2)]
    seen, masks, labels = {}, [], []
    for p, q in directions:
        if p == q:
            if ("s", p) in seen:
                continue
            seen[("s", p)] = 1
            masks.append(1 << coordinate(p, 0))
            labels.append(f"g0_{p}")
            continue
        i = max(p, q)
        k = seen.get(("b", i), 0)
        seen[("b", i)] = k + 1
        if k < 2:
            masks.append(1 << coordinate(i, 1 + k))
            labels.append(f"g{1 + k}_{i}")
    return np.array(masks, dtype=np.uint64), labels


def kind_groups(nspin: int):
    """All site energies / all real couplings / all imaginary couplings -> (masks, labels)."""
    n = int(nspin)
    return (np.array([mask_of(coordinate(i, 0) for i in range(n)), mask_of(coordinate(i, 1) for i in range(1, n)),
                      mask_of(coordinate(i, 2) for i in range(1, n))], dtype=np.uint64), ["site", "real", "imag"])


def site_groups(nspin: int):
    """g0_i together with the bond terms g1_i, g2_i below site i (site 0: its energy alone) -> (masks, labels)."""
    n = int(nspin)
    return (np.array([mask_of([coordinate(i, 0)] + ([coordinate(i, 1), coordinate(i, 2)] if i else [])) for i in range(n)],
                     dtype=np.uint64), [f"site_{i}" for i in range(n)])


def named_groups(groups, nspin: int):
    """"direction" / "kind" / "site" or an array of masks -> (checked (G,) uint64 masks, labels)."""
    if isinstance(groups, str):
        if groups not in GROUP_KINDS:
            raise ValueError(f"groups: one of {GROUP_KINDS} or an array of masks, got {groups!r}")
        masks, labels = {"direction": direction_groups, "kind": kind_groups, "site": site_groups}[groups](nspin)
        return check_groups(masks, nspin), labels
    masks = check_groups(groups, nspin)
    return masks, [f"{int(m):#x}" for m in masks]


def ranges_disjoint(offset_a: int, offset_b: int, n_elements: int) -> bool:
    """Are the element ranges [offset, offset + n_elements) disjoint, as distances modulo 2^64?"""
    n = int(n_elements)
    return n == 0 or ((int(offset_b) - int(offset_a)) % _U64 >= n and (int(offset_a) - int(offset_b)) % _U64 >= n)


def default_offset_b(offset: int, C: int, K: int, nspin: int) -> int:
    """offset_b of the entries when none is given: the block behind a's."""
    return (int(offset) + int(C) * int(K) * 3 * int(nspin)) % _U64


def mask_bits(groups, nspin: int) -> np.ndarray:
    """(G, N, 3) booleans: is coordinate 3 i + s in group g?"""
    g = check_groups(groups, nspin)
    j = np.arange(3 * int(nspin), dtype=np.uint64)
    return (((g[:, None] >> j[None, :]) & np.uint64(1)) != 0).reshape(len(g), int(nspin), 3)


def hybrids(a, b, groups) -> np.ndarray:
    """a, b (..., N, 3) -> (G, ..., N, 3): b where the group's mask is set, a elsewhere (a copy of bits)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    bits = mask_bits(groups, a.shape[-2])
    bits = bits.reshape((bits.shape[0],) + (1,) * (a.ndim - 2) + bits.shape[1:])
    return np.where(bits, b[None], a[None])


def evaluate(fidelity, a, b, groups) -> np.ndarray:
    """The G + 2 slabs (G + 2, C, K): slab 0 = fidelity(a), 1 = fidelity(b), 2 + g = fidelity(h_g), with `fidelity` a function of a
    (C, K, N, 3) draw tensor -> (C, K)."""
    h = hybrids(a, b, groups)
    return np.stack([np.asarray(fidelity(t), dtype=np.float64) for t in [np.asarray(a), np.asarray(b)] + list(h)])


def means_from_fidelities(fid) -> np.ndarray:
    """fid (G + 2, C, K) -> mean (C, 3 + 2 G): the exactly rounded means (math.fsum) of the once-rounded terms."""
    fid = np.asarray(fid, dtype=np.float64)
    G, C, K = fid.shape[0] - 2, fid.shape[1], fid.shape[2]
    fa, fb = fid[0], fid[1]
    sq = lambda u, v: (u - v) * (u - v)
    cols = [fa, fb, sq(fa, fb)]
    for g in range(G):
        cols += [sq(fa, fid[2 + g]), sq(fb, fid[2 + g])]
    out = np.empty((C, 3 + 2 * G))
    for c in range(C):
        for j, col in enumerate(cols):
            out[c, j] = math.fsum(col[c]) / K if K and not np.isnan(col[c]).any() else np.nan
    return out


def indices_from_means(mean) -> dict:
    """mean (..., 3 + 2 G) -> {"fav" (...,): mean fA, "var": D / 2, "total" (..., G): T_g / D, "first": 1 - U_g / D}.  D == 0
    gives var = 0 and NaN indices; NaN rows stay NaN."""
    mean = np.asarray(mean, dtype=np.float64)
    D = mean[..., 2]
    T, U = mean[..., 3::2], mean[..., 4::2]
    with np.errstate(divide="ignore", invalid="ignore"):
        den = np.where(D == 0.0, np.nan, D)[..., None]
        return {"fav": mean[..., 0].copy(), "var": D / 2.0, "total": T / den, "first": 1.0 - U / den}


def over_replicates(values) -> tuple:
    """values (R, ...) -> (mean over the replicates, std(ddof = 1) / sqrt(R)); R >= 2."""
    values = np.asarray(values, dtype=np.float64)
    R = values.shape[0]
    with np.errstate(invalid="ignore"):
        return values.mean(axis=0), values.std(axis=0, ddof=1) / np.sqrt(R)
