"""The pick-freeze kernel behind the variance indices (`backend.mc_fidelity_pickfreeze_philox`, ABI 20) on the device: bit
identity of every slab with the routes that exist (the fused Philox kernel for a and b, the tensor kernel on the materialised hybrid
tensors), the row means against the launch's own per-sample values and the exact identities of the special masks, the independent
reference (oracle `fidelity_eigh` on `philox_host` hybrids), per-row sigma / static terms / far and wrapping offsets, the repair
routes, and the layers above (`noise_variance_indices_philox`, `MCDataSim.get_variance_dict`).
Shapes: C = 3 rows of `grad_checks.philox_ctrl` (one NaN row, one negative time), K in {1, 63, 64, 65, 130} ({1, 65, 130} at N = 8, 9,
11, 12), an end-to-end pair (ends mode) and an interior pair (adjugate mode), and EVERY instantiation N = 2 ... 13.  Where the kernel
holds the two draw vectors a and b of a sample (`pickfreeze_reg_a`, `pickfreeze_reg_b`, `pickfreeze_min_waves`):
    N = 2        a and b in registers, three waves per SIMD; all-fp64
    N = 3        the same hold; the first mixed-precision size
    N = 4, 5, 6  a and b in registers, two waves per SIMD
    N = 7        a in registers, b in LDS, two waves (the headline size)
    N = 8        the first size with a and b both in LDS, one wave
    N = 9, 10    both in LDS
    N = 11       both in LDS: the largest all-LDS footprint
    N = 12       the only size with a split 4 coordinates in registers / 32 in LDS
    N = 13       the limit: a split 10 in registers / 29 in LDS
Long rows (K = 4096, 4097, 8193: more than one step of the row-mean kernel's loop over a row's tiles) and the ends of the group range
(G = 0, 1, 64) follow the per-size tests."""
import importlib

import numpy as np
import pytest

import grad_checks as gc
import variance_checks as vc

pytestmark = pytest.mark.gpu
vi = importlib.import_module("code-robchar_amd.variance_indices")
SIZES = tuple(range(2, 14))
KS = (1, 63, 64, 65, 130)


def ks(N):
    return (1, 65, 130) if N in (8, 9, 11, 12) else KS


def pairs(N):
    return ((0, N - 1), (N // 2, max(N // 2 - 1, 0)) if N > 2 else (1, 1))


@pytest.fixture(scope="module")
def dev(be):
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def draw_tensor(be, dev, C, K, N, offset, sigma):
    """(C, K, N, 3) on the device: row c = elements offset + c K 3N ... of stream SEED scaled by sigma[c] (a float: all rows)"""
    import torch
    t = torch.empty((C, K, N, 3), dtype=torch.float64, device=dev)
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (C,))
    for c in range(C):
        be.philox_normal((K, N, 3), vc.SEED, scale=float(sig[c]), offset=(offset + c * K * N * 3) % 2 ** 64, out=t[c])
    return t


def tensor_route(be, dev, ctrl, K, N, a, b, masks, offset, offset_b, sigma, h0_diag=None, h0_offdiag=None):
    """the G + 2 slabs from the entries that exist: two draw tensors, torch.where, mc_fidelity"""
    import torch
    C = ctrl.shape[0]
    A, B = draw_tensor(be, dev, C, K, N, offset, sigma), draw_tensor(be, dev, C, K, N, offset_b, sigma)
    bits = torch.as_tensor(vi.mask_bits(masks, N), device=dev)
    ct = torch.as_tensor(ctrl, device=dev)
    F = lambda d: be.mc_fidelity(ct, d.contiguous(), N, a, b, h0_diag=h0_diag, h0_offdiag=h0_offdiag).cpu().numpy()
    return np.stack([F(A), F(B)] + [F(torch.where(bits[g][None, None], B, A)) for g in range(len(masks))])


def fused(be, ctrl, K, N, a, b, masks, offset, offset_b, sigma=vc.SIGMA, want=("fid", "mean"), **kw):
    return vc.to_host(be.mc_fidelity_pickfreeze_philox(ctrl, K, N, a, b, vc.SEED, masks, offset=offset, offset_b=offset_b, sigma=sigma,
                                                       want=want, **kw))


def same_bits(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got, want, equal_nan=True), (what, int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum()), "entries differ")


@pytest.mark.parametrize("N", SIZES)
def test_bit_identity_with_the_routes_that_exist(be, dev, N):
    import torch
    ctrl = gc.philox_ctrl(N)
    C = ctrl.shape[0]
    masks, *_ = vc.groups_under_test(N)
    ct = torch.as_tensor(ctrl, device=dev)
    for K in ks(N):
        for (a, b) in pairs(N):
            off = 7 + K                              # odd and even offsets, odd and even 3 N K
            off_b = off + C * K * 3 * N + 1
            got = fused(be, ctrl, K, N, a, b, masks, off, off_b)
            for slab, o in ((0, off), (1, off_b)):
                same_bits(got["fid"][slab], be.mc_fidelity_philox(ct, K, N, a, b, vc.SEED, offset=o, sigma=vc.SIGMA).cpu().numpy(),
                          ("mc_fidelity_philox", slab, N, K, a, b))
            same_bits(got["fid"], tensor_route(be, dev, ctrl, K, N, a, b, masks, off, off_b, vc.SIGMA), ("tensor route", N, K, a, b))
            # the means: the same bits with and without the per-sample output, and on a second run
            alone = fused(be, ctrl, K, N, a, b, masks, off, off_b, want=("mean",))["mean"]
            same_bits(alone, got["mean"], ("mean alone", N, K, a, b))
            same_bits(fused(be, ctrl, K, N, a, b, masks, off, off_b)["mean"], got["mean"], ("second run", N, K, a, b))


@pytest.mark.parametrize("N", SIZES)
def test_means_against_own_slabs_and_exact_identities(be, N):
    for K in ks(N):
        for (a, b) in pairs(N):
            vc.check_means_against_own_slabs(be, N, K, a, b)


def test_sigma_zero_row_has_no_variance(be):
    N, K = 7, 130
    ctrl = gc.philox_ctrl(N)
    masks, *_ = vc.groups_under_test(N)
    got = fused(be, ctrl, K, N, 0, N - 1, masks, 0, None, sigma=np.array([0.0, 0.05, 0.05]))
    assert (got["mean"][0, 2:] == 0.0).all() and got["mean"][0, 0] == got["mean"][0, 1] > 0.0
    same_bits(got["fid"][1, 0], got["fid"][0, 0], "sigma = 0: fA == fB")
    idx = vi.indices_from_means(got["mean"])
    assert idx["var"][0] == 0.0 and np.isnan(idx["total"][0]).all() and np.isnan(idx["first"][0]).all()
    assert np.isnan(got["mean"][1]).all() and idx["var"][2] > 0.0


@pytest.mark.parametrize("N", SIZES)
def test_independent_reference(be, N):
    for K in (65, 130):
        for (a, b) in pairs(N):
            vc.check_against_reference(be, N, K, a, b)


def test_reference_has_teeth_on_the_shipped_rows(be, lbfgs_n7):
    """the shipped N = 7, 0 -> 6 rows: the indices differ by group (asserted on the reference alone), and the device agrees"""
    N, K, C = 7, 256, 3
    ctrl = np.ascontiguousarray(lbfgs_n7["ctrl_0-6"][:C])
    masks, *_ = vc.groups_under_test(N)
    off_b = C * K * 3 * N
    fid, mean = vc.reference(ctrl, K, N, 0, N - 1, masks, 0, off_b)
    D, T = mean[:, 2], mean[:, 3::2]
    print("D", D, "max T/D", (T / D[:, None])[:, :-3].max(axis=1), "smallest direction T/D", (T / D[:, None])[:, 3:-3].min(axis=1))
    assert (D >= 1e-3).all() and ((T / D[:, None])[:, :-3].max(axis=1) >= 0.2).all() and ((T / D[:, None])[:, 3:-3].min(axis=1) <= 0.02).all()
    got = fused(be, ctrl, K, N, 0, N - 1, masks, 0, off_b)
    err = np.abs(got["mean"] - mean)
    assert np.abs(got["fid"] - fid).max() < 1e-10 and err[:, :2].max() < 1e-10 and err[:, 2:].max() < vc.MEAN_ABS


@pytest.mark.parametrize("N,offset", ((7, gc.FAR_OFFSET), (7, None), (10, None), (3, 2 ** 63 + 1), (8, None), (12, None)))
def test_row_sigma_static_terms_far_and_wrapping_offsets(be, dev, N, offset):
    """offset None: `grad_checks.wrap_offset` - the low word of the pair counter wraps inside the first tile of A"""
    import torch
    offset = gc.wrap_offset(N) if offset is None else offset
    ctrl = gc.philox_ctrl(N)
    C, K = ctrl.shape[0], 65
    masks, *_ = vc.groups_under_test(N)
    rng = np.random.default_rng(N)
    h0d, h0o = rng.uniform(-0.3, 0.3, N), rng.uniform(0.8, 1.2, N - 1)          # (XXZ-like static diagonal, uneven couplings)
    sigma = np.array([0.02, 0.05, 0.11])
    off_b = offset + C * K * 3 * N + 2 ** 20
    for (a, b) in pairs(N):
        got = fused(be, ctrl, K, N, a, b, masks, offset, off_b, sigma=sigma, h0_diag=h0d, h0_offdiag=h0o)
        same_bits(got["fid"], tensor_route(be, dev, ctrl, K, N, a, b, masks, offset, off_b, sigma, h0d, h0o), ("tensor route", N, a, b))
    with pytest.raises(ValueError, match="overlap"):
        fused(be, ctrl, K, N, 0, N - 1, masks, offset, offset + C * K * 3 * N - 1)
    # element ranges that wrap at 2^64 (the generator of the draw tensor does not take them): the fused Philox kernel's bits
    ct, sg = torch.as_tensor(ctrl, device=dev), torch.as_tensor(sigma, device=dev)
    far_a, far_b = 2 ** 64 - 1000, 2 ** 64 - 1000 - C * K * 3 * N
    got = fused(be, ctrl, K, N, 0, N - 1, masks, far_a, far_b, sigma=sigma, h0_diag=h0d, h0_offdiag=h0o)
    for slab, o in ((0, far_a), (1, far_b)):
        same_bits(got["fid"][slab], be.mc_fidelity_philox(ct, K, N, 0, N - 1, vc.SEED, offset=o, sigma=sg, h0_diag=h0d,
                                                          h0_offdiag=h0o).cpu().numpy(), ("wrap at 2^64", slab, N))
    with pytest.raises(ValueError, match="overlap"):
        fused(be, ctrl, K, N, 0, N - 1, masks, far_a, 100)                      # inside A's range behind the wrap


@pytest.mark.parametrize("N", (4, 10, 12))
def test_repair_routes_keep_the_bits(be, dev, N):
    """Inputs the tensor kernel already handles (tests/test_gpu_chain.py's hard cases): a mirror-symmetric controller on a chain
    cut in the middle (static coupling 0 there) with sigma = 0 has an exactly degenerate spectrum - the eigenvalue-only weights
    bail out and the rows-mode repair runs -, a row with near-degenerate biases and a tiny sigma sits beside it."""
    C, K, cut = 3, 130, N // 2
    rng = np.random.default_rng(4242 + N)
    ctrl = gc.cc.deloc_ctrl(rng, C, N, 0.5)
    ctrl[0, N - cut:N] = ctrl[0, :cut][::-1]
    ctrl[2, :N] = rng.uniform(-1e-6, 1e-6, N)
    h0o = np.ones(N - 1)
    h0o[cut - 1] = 0.0
    sigma = np.array([0.0, 0.05, 1e-9])
    masks, *_ = vc.groups_under_test(N)
    off_b = C * K * 3 * N
    for (a, b) in ((0, cut - 1), (1, 1)):
        be.general_path_tiles(reset=True)
        got = fused(be, ctrl, K, N, a, b, masks, 0, off_b, sigma=sigma, h0_offdiag=h0o)
        tiles = be.general_path_tiles()
        print("repair", N, (a, b), tiles, "tiles")
        assert tiles > 0
        same_bits(got["fid"], tensor_route(be, dev, ctrl, K, N, a, b, masks, 0, off_b, sigma, None, h0o), ("repair, tensor route", N, a, b))
        assert np.nanmax(got["fid"]) > 1e-3


@pytest.mark.parametrize("N,K", ((2, 4096), (2, 4097), (3, 8193), (8, 4097)))
def test_long_rows_through_the_row_mean_kernel(be, dev, N, K):
    """more than 64 tiles per row: one tile per lane, a second step for lane 0 only, a third step, and the all-LDS hold"""
    import torch
    vc.check_long_rows(be, N, K, upload=lambda c: torch.as_tensor(c, device=dev))


@pytest.mark.parametrize("N", (3, 10))
def test_no_groups(be, dev, N):
    """G = 0: slabs A and B only, three mean columns"""
    import torch
    vc.check_no_groups(be, N, upload=lambda c: torch.as_tensor(c, device=dev))


@pytest.mark.parametrize("N", (3, 13))
def test_one_group_of_the_top_coordinate(be, dev, N):
    """G = 1, the mask of bit 3 N - 1 alone (the imaginary coupling below the last site)"""
    ctrl = gc.philox_ctrl(N)
    C, K = ctrl.shape[0], 65
    masks = np.array([1 << (3 * N - 1)], dtype=np.uint64)
    off, off_b = 4, 4 + C * K * 3 * N
    for (a, b) in pairs(N):
        got = fused(be, ctrl, K, N, a, b, masks, off, off_b)
        assert got["fid"].shape == (3, C, K) and got["mean"].shape == (C, 5)
        same_bits(got["fid"], tensor_route(be, dev, ctrl, K, N, a, b, masks, off, off_b, vc.SIGMA), ("G = 1, tensor route", N, a, b))
        g = vc.assert_means_of_own_slabs(got, ~np.isnan(ctrl).any(axis=1), ("G = 1", N, a, b))
        if (a, b) == (0, N - 1):
            assert (g[:, 3] > 0.0).all() and (g[:, 4] > 0.0).all()          # the coordinate moves F, and is not all of the noise


@pytest.mark.parametrize("K", (65, 130))
def test_every_subset_of_the_coordinates_at_two_spins(be, dev, K):
    """G = 64 at N = 2 - the full argument block, 66 slabs: the masks 0 ... 63 are every subset of the 6 coordinates"""
    N = 2
    vc.check_every_subset(be, K)
    ctrl = gc.philox_ctrl(N)
    masks = np.arange(64, dtype=np.uint64)
    off, off_b = 5, 5 + ctrl.shape[0] * K * 3 * N + 7
    for (a, b) in ((0, 1), (1, 0)):
        got = fused(be, ctrl, K, N, a, b, masks, off, off_b, want=("fid",))
        same_bits(got["fid"], tensor_route(be, dev, ctrl, K, N, a, b, masks, off, off_b, vc.SIGMA), ("every subset, tensor route", K, a, b))


def test_sixty_four_groups_at_the_largest_size(be, dev):
    """G = 64 at N = 13: every single coordinate and 25 random masks that reach into the mask's high word"""
    N, K = 13, 65
    ctrl = gc.philox_ctrl(N)
    masks = vc.limit_masks()
    off, off_b = 6, 6 + ctrl.shape[0] * K * 3 * N + 1
    for (a, b) in pairs(N):
        got = fused(be, ctrl, K, N, a, b, masks, off, off_b)
        assert got["fid"].shape == (66, ctrl.shape[0], K)
        same_bits(got["fid"], tensor_route(be, dev, ctrl, K, N, a, b, masks, off, off_b, vc.SIGMA), ("G = 64, tensor route", N, a, b))
        vc.assert_means_of_own_slabs(got, ~np.isnan(ctrl).any(axis=1), ("G = 64", N, a, b))
        assert np.nanmax(got["fid"]) > 1e-3


def test_through_the_noise_model(be):
    noise = importlib.import_module("code-robchar_amd.noise")
    N, K, R, C = 5, 130, 4, 2
    model = noise.structured_perturbation(Nspin=N, inspin=0, outspin=N - 1, noise=0.05)
    ctrl = gc.philox_ctrl(N, C=C, nan_row=None, neg_row=1)
    res = model.noise_variance_indices_philox(ctrl, K, vc.SEED, groups="kind", replicates=R, offset=5)
    masks, labels = vi.kind_groups(N)
    assert res["labels"] == labels and np.array_equal(res["groups"], masks)
    # the definition on the same stream blocks: replicate r reads a at offset + r C K 3N, b at offset + (R + r) C K 3N
    block = C * K * 3 * N
    idx = []
    for r in range(R):
        mean = fused(be, ctrl, K, N, 0, N - 1, masks, 5 + r * block, 5 + (R + r) * block, want=("mean",))["mean"]
        ref = vc.reference(ctrl, K, N, 0, N - 1, masks, 5 + r * block, 5 + (R + r) * block)[1]
        assert np.abs(mean - ref).max() < vc.MEAN_ABS
        idx.append(vi.indices_from_means(mean))
    for k in ("var", "first", "total"):
        m, se = vi.over_replicates(np.stack([i[k] for i in idx]))
        assert np.array_equal(res[k], m) and np.array_equal(res[k + "_se"], se), k
    one = model.noise_variance_indices_philox(ctrl, K, vc.SEED, groups="site")
    assert one["first"].shape == (C, N) and "first_se" not in one and (one["total"] >= 0).all()


def test_get_variance_dict_end_to_end(be, tmp_path, monkeypatch):
    """`MCDataSim.get_variance_dict` on the seeded small setup of tests/test_gpu_mcdatasim.py: the table equals the definition on the
    launch's stream blocks (inside the parity bounds), the padded rows are NaN, the sigma = 0 level has no variance."""
    import json
    import os
    mcmod = importlib.import_module("code-robchar_amd.mc_data_sim")
    monkeypatch.chdir(tmp_path)
    N, C, K = 5, 6, 130
    rng = np.random.default_rng(3)
    le = {}
    for a in ("ppo", "lbfgs"):
        x = gc.cc.deloc_ctrl(rng, C if a == "ppo" else C - 2, N, 0.5)          # lbfgs: fewer controllers than asked for -> NaN rows
        le[a] = {("%d" % N if a == "lbfgs" else "0.05"): {"controller": x.tolist()}}
    noises = np.array([0.0, 0.05, 0.1])
    os.makedirs("experiments/var")
    json.dump(le, open(f"experiments/var/ppo_spin_{N}_0-4_c_{C}", "w"))
    sim = mcmod.MCDataSim(experiment_name="var", Nspin=N, inspin=0, outspin=4, noises=noises, bootreps=K, training_noise=0.05,
                          numcontrollers=C, verbose=False, seed=5, cache_format="json")
    table = sim.get_variance_dict(groups="kind")
    masks, labels = vi.kind_groups(N)
    for a, nvalid in (("ppo", C), ("lbfgs", C - 2)):
        t = table[a]
        ctrl = np.array(next(iter(le[a].values()))["controller"])
        var, first, total, fav = (np.array(t[k], dtype=np.float64) for k in ("var", "first", "total", "fav"))
        assert t["groups"] == labels and var.shape == (3, C) and total.shape == (3, C, 3)
        assert np.isnan(var[:, nvalid:]).all() and np.isnan(total[:, nvalid:]).all() and not np.isnan(var[:, :nvalid]).any()
        assert (var[0, :nvalid] == 0.0).all() and np.isnan(total[0]).all()
        per = nvalid * K * 3 * N
        for j in (1, 2):
            mean = vc.reference(ctrl, K, N, 0, 4, masks, j * per, 3 * per + j * per, sigma=float(noises[j]), seed=5)[1]
            want = vi.indices_from_means(mean)
            assert np.abs(fav[j, :nvalid] - want["fav"]).max() < 1e-10 and np.abs(var[j, :nvalid] - want["var"]).max() < vc.MEAN_ABS
            # indices: quotients of two means known to MEAN_ABS each
            bound = 4 * vc.MEAN_ABS / mean[:, 2].min()
            assert np.abs(total[j, :nvalid] - want["total"]).max() < bound and np.abs(first[j, :nvalid] - want["first"]).max() < bound
    assert os.path.exists(sim.get_mcname(0.05, noises) + "v")
