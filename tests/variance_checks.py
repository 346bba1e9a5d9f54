"""Checks of the pick-freeze entry behind the variance indices, written against a backend object (anything with
`mc_fidelity_pickfreeze_philox` like `code-robchar_amd.backend`), and a NumPy stand-in for it: the oracle's `fidelity_eigh` on
`oracle/philox_host.py` draws plus the definition module `code-robchar_amd/variance_indices.py`.  The GPU tests run the checks on
the device; tests/test_variance_checks.py runs them on the stand-in, where they must pass, and on deliberately broken stand-ins,
where they must fail."""
import importlib
import math

import numpy as np

import chain_checks as cc
import grad_checks as gc
from oracle import philox_host
from oracle import robchar_oracle as orc

vi = importlib.import_module("code-robchar_amd.variance_indices")

SEED = 0x5EEDF00D1234
SIGMA = 0.05
EPS = 2.0 ** -52
MEAN_ABS = 5e-10     # means of squared differences: |d (x - y)^2| <= 2 |x - y| 2e-10 + 4e-20 with |x - y| <= 1
SELF_REL = 32 * EPS  # a row mean against the fsum of the launch's own terms: < 20 roundings of non-negative terms for K <= 2^18


def groups_under_test(N):
    """the 3 kinds + all directions + the empty mask + the full mask + {1, 2} -> (masks, index of empty, of full, of {1, 2})"""
    kinds, _ = vi.kind_groups(N)
    dirs, _ = vi.direction_groups(N)
    masks = np.concatenate([kinds, dirs, np.array([0, (1 << (3 * N)) - 1, 0b110], dtype=np.uint64)])
    G = len(masks)
    return masks, G - 3, G - 2, G - 1


def host_draws(C, K, N, seed, offset, sigma):
    """(C, K, N, 3): row c scaled by sigma[c] (a float: every row)"""
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (C,))
    out = np.empty((C, K, N, 3))
    for c in range(C):
        out[c] = philox_host.philox_normal(seed, offset + c * K * N * 3, K * N * 3, float(sig[c])).reshape(K, N, 3)
    return out


def to_host(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in res.items()}


class StandIn:
    """`mc_fidelity_pickfreeze_philox` in NumPy.  `broken`: one of BROKEN - a deliberate mistake the checks must catch."""

    def __init__(self, broken=None):
        self.broken = broken

    def mc_fidelity_pickfreeze_philox(self, controllers, n_draws, nspin, inspin, outspin, seed, groups, offset=0, offset_b=None,
                                      sigma=0.05, h0_diag=None, h0_offdiag=None, want=("mean",), kernel="auto"):
        ctrl = np.asarray(controllers, dtype=np.float64)
        C, K, N = ctrl.shape[0], int(n_draws), nspin
        masks = vi.check_groups(groups, N)
        if offset_b is None:
            offset_b = vi.default_offset_b(offset, C, K, N)
        if not vi.ranges_disjoint(offset, offset_b, C * K * 3 * N):
            raise ValueError("offset_b: the element ranges of offset and offset_b overlap")
        a = host_draws(C, K, N, seed, offset, sigma)
        b = host_draws(C, K, N, seed, offset if self.broken == "b_from_offset_a" else offset_b, 1.0 if self.broken == "sigma_a_only" else sigma)
        if self.broken == "index_3s_plus_i":          # the transposed layout: bit s N + i (3 s + i at N = 3) instead of 3 i + s
            bits = np.zeros((len(masks), N, 3), dtype=bool)
            for g, m in enumerate(masks):
                for i in range(N):
                    for s in range(3):
                        j = s * N + i
                        bits[g, i, s] = (int(m) >> j) & 1
            h = np.where(bits[:, None, None], b[None], a[None])
        elif self.broken == "roles_swapped":
            h = vi.hybrids(b, a, masks)
        else:
            h = vi.hybrids(a, b, masks)
        F = lambda d: orc.fidelity_eigh(ctrl, d, N, inspin, outspin, h0_diag=h0_diag, h0_offdiag=h0_offdiag)
        fid = np.stack([F(a), F(b)] + [F(t) for t in h]) if K else np.empty((len(masks) + 2, C, 0))
        mean = vi.means_from_fidelities(fid)
        if self.broken == "t_u_exchanged":
            mean[:, 3::2], mean[:, 4::2] = mean[:, 4::2].copy(), mean[:, 3::2].copy()
        if self.broken == "mean_over_tiles" and K:
            mean *= K / (64.0 * ((K + 63) // 64))
        if self.broken == "mean_first_64_tiles" and K > 64 * 64:      # the strided loop over a row's tiles stops after one trip
            mean = vi.means_from_fidelities(fid[:, :, :64 * 64]) * (64 * 64 / K)
        if self.broken == "slab_one_off" and len(masks) > 1:
            fid = np.concatenate([fid[:2], np.roll(fid[2:], 1, axis=0)])
        res = {"fid": fid, "mean": mean}
        return {k: res[k] for k in want}

    def mc_fidelity_philox(self, controllers, n_draws, nspin, inspin, outspin, seed, offset=0, sigma=0.05, h0_diag=None, h0_offdiag=None):
        """the existing fused route the slabs 0 and 1 are held to: the same draws, the same oracle"""
        ctrl = np.asarray(controllers, dtype=np.float64)
        draws = host_draws(ctrl.shape[0], int(n_draws), nspin, seed, offset, sigma)
        return orc.fidelity_eigh(ctrl, draws, nspin, inspin, outspin, h0_diag=h0_diag, h0_offdiag=h0_offdiag)


# mistakes that show at any K (`run_all`), and those that need a row of more than 64 tiles (`check_long_rows`)
LONG_ROW_BROKEN = ("mean_first_64_tiles",)
BROKEN = ("roles_swapped", "t_u_exchanged", "b_from_offset_a", "index_3s_plus_i", "sigma_a_only", "mean_over_tiles", "slab_one_off") + LONG_ROW_BROKEN
MIN_D = 1e-4         # mean (fA - fB)^2 of a live row of the reference: 2e5 MEAN_ABS, so a wrong hybrid cannot hide under the bound


def reference(ctrl, K, N, a, b, masks, offset, offset_b, sigma=SIGMA, h0_diag=None, h0_offdiag=None, seed=SEED):
    """The independent answer: `fidelity_eigh` on `philox_host` hybrids -> (fid (G + 2, C, K), mean (C, 3 + 2 G))"""
    C = ctrl.shape[0]
    A, B = host_draws(C, K, N, seed, offset, sigma), host_draws(C, K, N, seed, offset_b, sigma)
    fid = vi.evaluate(lambda d: orc.fidelity_eigh(ctrl, d, N, a, b, h0_diag=h0_diag, h0_offdiag=h0_offdiag), A, B, masks)
    return fid, vi.means_from_fidelities(fid)


def check_against_reference(be, N, K, a, b, teeth=False):
    """slabs: the project's parity bounds; means of squared differences: MEAN_ABS; the NaN row all NaN"""
    ctrl = gc.philox_ctrl(N)
    C = ctrl.shape[0]
    masks, *_ = groups_under_test(N)
    off, off_b = 11, 11 + C * K * 3 * N + 5
    got = to_host(be.mc_fidelity_pickfreeze_philox(ctrl, K, N, a, b, SEED, masks, offset=off, offset_b=off_b, sigma=SIGMA,
                                                   want=("fid", "mean")))
    fid, mean = reference(ctrl, K, N, a, b, masks, off, off_b)
    live = ~np.isnan(ctrl).any(axis=1)
    # asserted on the reference alone: the fidelities are not tiny, and a and b give different ones
    cc.assert_has_teeth(fid[0], what=("pick-freeze", N, K, a, b))
    assert (mean[live, 2] >= MIN_D).all(), ("D", N, K, a, b, mean[live, 2])
    if teeth:
        D, T = mean[live, 2], mean[live, 3::2]
        print("teeth", N, K, (a, b), "D", D, "max T/D", (T / D[:, None])[:, :-3].max(), "min T/D of a direction", (T / D[:, None])[:, 3:-3].min())
        assert (D >= 1e-3).all(), ("D", D)
        assert (T / D[:, None])[:, :-3].max() >= 0.2 and (T / D[:, None])[:, 3:-3].min() <= 0.02, "the groups cannot tell the indices apart"
    assert got["fid"].shape == fid.shape and got["mean"].shape == mean.shape
    worst = [cc.compare(got["fid"][e], fid[e], ("slab", e, N, K, a, b)) for e in range(fid.shape[0])]
    assert np.isnan(got["mean"][~live]).all() and not np.isnan(got["mean"][live]).any()
    err = np.abs(got["mean"][live] - mean[live])
    print("reference", N, K, (a, b), "slabs max abs", max(w[0] for w in worst), "max rel", max(w[1] for w in worst), "means max abs", err.max())
    assert err[:, :2].max() < cc.TOL and err[:, 2:].max() < MEAN_ABS, err.max()


def check_means_against_own_slabs(be, N, K, a, b):
    """"mean" against math.fsum over the launch's own per-sample values: SELF_REL; exact identities of the special masks"""
    ctrl = gc.philox_ctrl(N)
    masks, i_empty, i_full, i_12 = groups_under_test(N)
    got = to_host(be.mc_fidelity_pickfreeze_philox(ctrl, K, N, a, b, SEED, masks, offset=3, sigma=SIGMA, want=("fid", "mean")))
    want = vi.means_from_fidelities(got["fid"])
    live = ~np.isnan(ctrl).any(axis=1)
    assert np.isnan(got["mean"][~live]).all() and np.isnan(got["fid"][:, ~live]).all()
    g, w = got["mean"][live], want[live]
    assert (np.abs(g - w) <= SELF_REL * np.abs(w)).all(), ("row means", N, K, float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300))))
    D = g[:, 2]
    T, U = g[:, 3::2], g[:, 4::2]
    assert (g[:, 2:] >= 0.0).all()
    assert (T[:, i_empty] == 0.0).all() and np.array_equal(U[:, i_empty], D), "empty mask"
    assert (U[:, i_full] == 0.0).all() and np.array_equal(T[:, i_full], D), "full mask"
    assert (T[:, i_12] == 0.0).all(), "mask {1, 2}"
    # masks that differ only in bits 1, 2 give equal bits
    both = to_host(be.mc_fidelity_pickfreeze_philox(ctrl, K, N, a, b, SEED, masks | np.uint64(0b110), offset=3, sigma=SIGMA,
                                                   want=("mean",)))["mean"]
    assert np.array_equal(both[live][:, :3 + 2 * i_empty], g[:, :3 + 2 * i_empty])


def check_long_rows(be, N, K, upload=None):
    """Rows of more than 64 tiles in the row-mean kernel, whose lanes stride over a row's tiles (K = 4096: one tile per lane; 4097:
    a second step for lane 0 only; 8193: a third).  "mean" against math.fsum over the launch's own slabs (SELF_REL: K <= 2^18), the
    same bits without "fid", slabs 0 and 1 the bits of `mc_fidelity_philox` at the two offsets, the means against the independent
    reference.  `upload`: what turns the controller array into the argument `be.mc_fidelity_philox` takes (a device tensor)."""
    ctrl = gc.philox_ctrl(N)
    C, a, b = ctrl.shape[0], 0, N - 1
    masks, *_ = groups_under_test(N)
    off, off_b = 7, 7 + C * K * 3 * N + 1
    call = lambda want: to_host(be.mc_fidelity_pickfreeze_philox(ctrl, K, N, a, b, SEED, masks, offset=off, offset_b=off_b, sigma=SIGMA,
                                                                 want=want))
    got = call(("fid", "mean"))
    live = ~np.isnan(ctrl).any(axis=1)
    assert got["fid"].shape == (len(masks) + 2, C, K) and got["mean"].shape == (C, 3 + 2 * len(masks))
    assert np.isnan(got["mean"][~live]).all() and np.isnan(got["fid"][:, ~live]).all() and not np.isnan(got["mean"][live]).any()
    want = vi.means_from_fidelities(got["fid"])
    g, w = got["mean"][live], want[live]
    rel = float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300)))
    print("long rows", N, K, "means against own slabs, worst relative", rel, "of", SELF_REL)
    assert (np.abs(g - w) <= SELF_REL * np.abs(w)).all(), ("row means", N, K, rel)
    assert np.array_equal(call(("mean",))["mean"], got["mean"], equal_nan=True), ("mean alone", N, K)
    ct = ctrl if upload is None else upload(ctrl)
    for slab, o in ((0, off), (1, off_b)):
        one = be.mc_fidelity_philox(ct, K, N, a, b, SEED, offset=o, sigma=SIGMA)
        one = one.cpu().numpy() if hasattr(one, "cpu") else np.asarray(one)
        assert np.array_equal(got["fid"][slab], one, equal_nan=True), ("mc_fidelity_philox", slab, N, K)
    mean = reference(ctrl, K, N, a, b, masks, off, off_b)[1]
    assert (mean[live, 2] >= MIN_D).all(), ("D", N, K, mean[live, 2])
    err = np.abs(g - mean[live])
    print("long rows", N, K, "means against the reference: F", err[:, :2].max(), "squared differences", err[:, 2:].max())
    assert err[:, :2].max() < cc.TOL and err[:, 2:].max() < MEAN_ABS, (N, K, err.max())


def _philox_slab(be, ct, K, N, a, b, offset):
    one = be.mc_fidelity_philox(ct, K, N, a, b, SEED, offset=offset, sigma=SIGMA)
    return one.cpu().numpy() if hasattr(one, "cpu") else np.asarray(one)


def assert_means_of_own_slabs(got, live, what):
    """"mean" against math.fsum over the same launch's "fid": SELF_REL; NaN rows NaN"""
    want = vi.means_from_fidelities(got["fid"])
    assert got["mean"].shape == want.shape, what
    assert np.isnan(got["mean"][~live]).all() and np.isnan(got["fid"][:, ~live]).all() and not np.isnan(got["mean"][live]).any(), what
    g, w = got["mean"][live], want[live]
    assert (np.abs(g - w) <= SELF_REL * np.abs(w)).all(), ("row means", what, float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300))))
    assert (g[:, 2:] >= 0.0).all(), what
    return g


def check_no_groups(be, N, K=65, upload=None):
    """G = 0, the short end of the group range (slabs A and B only): "fid" (2, C, K) = the two `mc_fidelity_philox` launches bit for
    bit, "mean" (C, 3) = the first three columns of a launch with groups bit for bit"""
    ctrl = gc.philox_ctrl(N)
    C = ctrl.shape[0]
    ct = ctrl if upload is None else upload(ctrl)
    none = np.zeros(0, dtype=np.uint64)
    masks, *_ = groups_under_test(N)
    for (a, b) in ((0, N - 1), (N // 2, max(N // 2 - 1, 0))):
        off, off_b = 9, 9 + C * K * 3 * N + 3
        call = lambda m, want: to_host(be.mc_fidelity_pickfreeze_philox(ctrl, K, N, a, b, SEED, m, offset=off, offset_b=off_b, sigma=SIGMA,
                                                                        want=want))
        got = call(none, ("fid", "mean"))
        assert got["fid"].shape == (2, C, K) and got["mean"].shape == (C, 3), (N, a, b)
        for slab, o in ((0, off), (1, off_b)):
            assert np.array_equal(got["fid"][slab], _philox_slab(be, ct, K, N, a, b, o), equal_nan=True), ("G = 0", slab, N, a, b)
        cc.assert_has_teeth(got["fid"][0], what=("G = 0", N, a, b))
        full = call(masks, ("mean",))["mean"]
        assert np.array_equal(got["mean"], full[:, :3], equal_nan=True), ("G = 0, means", N, a, b)
        assert np.array_equal(call(none, ("mean",))["mean"], got["mean"], equal_nan=True), ("G = 0, mean alone", N, a, b)
        assert_means_of_own_slabs(got, ~np.isnan(ctrl).any(axis=1), ("G = 0", N, a, b))


def check_every_subset(be, K):
    """G = 64 at N = 2, the long end of the group range: the masks 0 .. 63 are every subset of the 6 coordinates.  Means against own
    slabs, the exact identities (T = 0 and U = D for the empty mask, the mirror for the full mask, T = 0 for every mask inside
    {1, 2}; masks that differ only in bits 1, 2 give the same slab), slabs and means against the independent reference."""
    N = 2
    ctrl = gc.philox_ctrl(N)
    C = ctrl.shape[0]
    masks = np.arange(64, dtype=np.uint64)
    live = ~np.isnan(ctrl).any(axis=1)
    for (a, b) in ((0, 1), (1, 0)):
        off, off_b = 5, 5 + C * K * 3 * N + 7
        got = to_host(be.mc_fidelity_pickfreeze_philox(ctrl, K, N, a, b, SEED, masks, offset=off, offset_b=off_b, sigma=SIGMA,
                                                       want=("fid", "mean")))
        assert got["fid"].shape == (66, C, K) and got["mean"].shape == (C, 131)
        g = assert_means_of_own_slabs(got, live, ("every subset", K, a, b))
        D, T, U = g[:, 2], g[:, 3::2], g[:, 4::2]
        assert (D > 0.0).all()
        assert (T[:, 0] == 0.0).all() and np.array_equal(U[:, 0], D), "empty mask"
        assert (U[:, 63] == 0.0).all() and np.array_equal(T[:, 63], D), "full mask"
        assert (T[:, [0, 2, 4, 6]] == 0.0).all(), "masks inside {1, 2}"
        assert (T[:, [m for m in range(64) if m & ~6]] > 0.0).all(), "every other mask moves F"
        for m in range(64):
            assert np.array_equal(got["fid"][2 + m], got["fid"][2 + (m | 6)], equal_nan=True), ("bits 1, 2 have no effect", m)
        fid, mean = reference(ctrl, K, N, a, b, masks, off, off_b)
        cc.assert_has_teeth(fid[0], what=("every subset", K, a, b))
        assert (mean[live, 2] >= MIN_D).all()
        for e in range(66):
            cc.compare(got["fid"][e], fid[e], ("every subset, slab", e, K, a, b))
        err = np.abs(g - mean[live])
        assert err[:, :2].max() < cc.TOL and err[:, 2:].max() < MEAN_ABS, err.max()
    return got


def limit_masks():
    """64 masks at N = 13: the 39 single coordinates, then 25 random masks over the 39 bits from a fixed seed, each with at least one
    bit >= 32 set (the high word of the mask is read)"""
    rng = np.random.default_rng(1364)
    masks = [1 << j for j in range(39)]
    while len(masks) < 64:
        m = int(rng.integers(0, 2 ** 39))
        if m >> 32:
            masks.append(m)
    return np.array(masks, dtype=np.uint64)


def run_all(be, N=3, K=65, pair=None):
    a, b = (0, N - 1) if pair is None else pair
    check_against_reference(be, N, K, a, b)
    check_means_against_own_slabs(be, N, K, a, b)
