"""Placement tests: every entry of backend.py that takes or returns device tensors, run with its tensors inside guarded arenas
(tests/arena.py) - the suite's other GPU tests pass tensors that start an allocation of exactly their size, where a store past
the end, an element left unwritten, a read past an input and a dependence on the 16-byte phase of a pointer all go unseen.

The protocol, the same for every case (`placement`):
  1. the PLAIN call (exact-size tensors from the default allocator) is held against the component's own reference with the
     component's own compare function and bars - nothing new is tolerated here;
  2. the same call again for shift in {0, 1} (the float64 bodies at 0 / 8 mod 16 bytes) x the poison around the inputs in
     {sentinel NaN, finite}: every input through `arena.place`, every tensor the backend allocates through `arena.empty`
     (`torch.empty` patched), and where the entry has `out=` a second run with `out=` carved from the arena;
  3. after a synchronise: (a) every guard word intact, (b) no element of a returned tensor still the sentinel, (c) every returned
     tensor bit-identical to the plain call - the library's contract is that placement changes no arithmetic (README; DESIGN.md
     "Placement"), so (c) is an equality.
The shapes are the smallest that reach the edges: a one-sample tail behind a full tile (K = 65), a lone lane (K = 1), odd rows
(odd N: `align16 == 0` whatever the pointer), even rows with K = 65 (`align16 == 1` with an odd piece count in the tail), a base
pointer at 8 mod 16 (`align16 == 0` by the pointer alone), a NaN controller row in the middle wherever the entry documents one."""
import math
import time

import numpy as np
import pytest

import bootstrap_checks as bc
import chain_checks as cc
import grad_checks as gc
import lbfgs_box_checks as lbc
import lbfgs_checks as lc
import listed_checks as lsc
import reduce_checks as rc
import ring_checks as rg
import sens_checks as sc
import tail_select_checks as tsc
import times_checks as tc
from arena import FILLS, Arena
from oracle import philox_host
from oracle import robchar_oracle as orc

pytestmark = pytest.mark.gpu
COMBOS = [(shift, fill) for shift in (0, 1) for fill in FILLS]
SIGMA = 0.05


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_gpu_placement.py: {time.perf_counter() - t0:.1f} s wall")


@pytest.fixture(scope="module")
def dev(be):
    return be.compute_device()


# ------------------------------------------------------------------------------------------------------------------------
# the protocol
# ------------------------------------------------------------------------------------------------------------------------


def tensors(res):
    """the tensors of a result (a tensor, a tuple of tensors, or a dict that may hold other things) by name"""
    if isinstance(res, dict):
        return {k: v for k, v in res.items() if hasattr(v, "data_ptr")}
    if isinstance(res, (tuple, list)):
        return {str(i): v for i, v in enumerate(res)}
    return {"out": res}


def host(res):
    return {k: v.cpu().numpy() for k, v in tensors(res).items()}


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    return np.array_equal(x.view(np.uint64), y.view(np.uint64)) if x.dtype == np.float64 else np.array_equal(x, y)


def up(dev, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def plain_call(dev, call, inputs):
    """step 1: `call(None, **inputs on the device)` -> host arrays by name"""
    return host(call(None, **{k: up(dev, v) for k, v in inputs.items()}))


def placement(dev, call, inputs, plain, what, unchecked=(), outs=(False,)):
    """steps 2 and 3.  `call(arena or None, **inputs)` -> the entry's result; with `outs` = (False, True) it is called a second
    time per combination as `call(arena, out=True, **inputs)` and then hands the entry an `out=` carved by `arena.empty`.
    `unchecked`: returned tensors the entry does not document as fully written (guards and bits are still checked)."""
    import torch
    for shift, fill in COMBOS:
        for with_out in outs:
            ar = Arena(shift=shift, device=dev)
            tag = (what, "shift", shift, "poison", fill, "out=" if with_out else "")
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(torch, "empty", ar.empty)
                placed = {k: (None if v is None else ar.place(v, fill)) for k, v in inputs.items()}
                res = tensors(call(ar, out=True, **placed) if with_out else call(ar, **placed))
            assert any(" empty " in b.name for b in ar.blocks), (tag, "nothing was allocated through the arena")
            try:
                ar.check_guards()
                for k, t in res.items():
                    if k not in unchecked:
                        ar.assert_written(t, k)
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}") from None
            got = host(res)
            assert sorted(got) == sorted(plain), (tag, sorted(got), sorted(plain))
            for k in got:
                if not same_bits(got[k], plain[k]):
                    diff = ~((got[k] == plain[k]) | ((got[k] != got[k]) & (plain[k] != plain[k]))) if got[k].shape == plain[k].shape else None
                    raise AssertionError(f"{tag}: '{k}' depends on where its tensors sit: "
                                         f"{'shape' if diff is None else int(diff.sum())} of {got[k].size} entries differ from the plain call"
                                         + ("" if diff is None or not diff.any() else f", the first at flat index {int(np.flatnonzero(diff)[0])}"))


def teeth(want, K, what):
    """chain_checks.assert_has_teeth; a single sample per row cannot carry the share guard (as in chain_checks.check_long_chain)"""
    if K > 1:
        cc.assert_has_teeth(want, what=what)
    else:
        cc.assert_has_teeth(want, median=1e-3, share=0.0, what=what)


def deloc_rows(rng, C, N, nan=True):
    """delocalised rows with T = N / 2 + 1 ... 5 (just behind the first arrival at the far end); C >= 3: the middle row NaN"""
    ctrl = cc.deloc_ctrl(rng, C, N, 0.5)
    ctrl[:, N] = N / 2 + rng.uniform(1.0, 5.0, C)
    if nan and C >= 3:
        ctrl[C // 2, N // 2] = np.nan
    return ctrl


# ------------------------------------------------------------------------------------------------------------------------
# mc_fidelity: chain (every kernel), ring, generated draws
# ------------------------------------------------------------------------------------------------------------------------

CHAIN_N = (2, 4, 7, 16, 17, 24, 25, 32)


def chain_cases(N):
    """(tag, ctrl, draws, reference) per shape: (C, K) = (3, 65) and (2, 1), K = 130 at N = 4 and 7, one shared draw set"""
    rng = np.random.default_rng(41000 + N)
    shapes = [(3, 65, False), (2, 1, False), (3, 65, True)] + ([(3, 130, False)] if N in (4, 7) else [])
    for C, K, shared in shapes:
        ctrl = deloc_rows(rng, C, N)
        draws = SIGMA * rng.standard_normal((1 if shared else C, K, N, 3))
        full = np.broadcast_to(draws, (C, K, N, 3))
        yield (N, C, K, "shared" if shared else "per row"), ctrl, draws, cc.oracle_pairs(ctrl, full, N, [(0, N - 1)])[0, N - 1]


@pytest.mark.parametrize("N", CHAIN_N)
def test_mc_fidelity_chain(be, dev, N):
    for tag, ctrl, draws, want in chain_cases(N):
        teeth(want, draws.shape[1], tag)
        for kern in cc.chain_kernels(N):
            def call(ar, ctrl, draws, out=False):
                import torch
                o = torch.empty((ctrl.shape[0], draws.shape[1]), dtype=torch.float64, device=dev) if out else None
                return be.mc_fidelity(ctrl, draws, N, 0, N - 1, kernel=kern, out=o)
            plain = plain_call(dev, call, {"ctrl": ctrl, "draws": draws})
            cc.compare(plain["out"], want, (tag, kern))
            placement(dev, call, {"ctrl": ctrl, "draws": draws}, plain, (tag, kern), outs=(False, True))


RING_N = (3, 7, 10, 11, 16)


def ring_case(N):
    rng = np.random.default_rng(42000 + N)
    ctrl = rg.deloc_ring_ctrl(rng, 3, N, 0.5)
    ctrl[1, N // 2] = np.nan
    draws = SIGMA * rng.standard_normal((3, 65, N, 3))
    return ctrl, draws, cc.oracle_pairs(ctrl, draws, N, [(0, N // 2)], ring=True)[0, N // 2]


@pytest.mark.parametrize("N", RING_N)
def test_mc_fidelity_ring(be, dev, N):
    ctrl, draws, want = ring_case(N)
    cc.assert_has_teeth(want, what=("ring", N))

    def call(ar, ctrl, draws, out=False):
        import torch
        o = torch.empty((3, 65), dtype=torch.float64, device=dev) if out else None
        return be.mc_fidelity(ctrl, draws, N, 0, N // 2, ring=True, out=o)
    plain = plain_call(dev, call, {"ctrl": ctrl, "draws": draws})
    cc.compare(plain["out"], want, ("ring", N))
    placement(dev, call, {"ctrl": ctrl, "draws": draws}, plain, ("ring", N), outs=(False, True))


PHILOX_SEED = 0x5EED00A7


def philox_case(N, offset):
    rng = np.random.default_rng(43000 + N)
    C, K = 3, 65
    ctrl = deloc_rows(rng, C, N)
    sig = np.array([0.05, 0.03, 0.08])
    draws = philox_host.philox_normal(PHILOX_SEED, offset, C * K * N * 3, 1.0).reshape(C, K, N, 3) * sig[:, None, None, None]
    return ctrl, sig, orc.fidelity_eigh(ctrl, draws, N, 0, N - 1)


@pytest.mark.parametrize("N", (2, 7, 14, 16))
def test_mc_fidelity_philox(be, dev, N):
    for offset in (0, 7):
        ctrl, sig, want = philox_case(N, offset)
        cc.assert_has_teeth(want, what=("philox", N, offset))

        def call(ar, ctrl, sig, out=False):
            import torch
            o = torch.empty((3, 65), dtype=torch.float64, device=dev) if out else None
            return be.mc_fidelity_philox(ctrl, 65, N, 0, N - 1, PHILOX_SEED, offset=offset, sigma=sig, out=o)
        plain = plain_call(dev, call, {"ctrl": ctrl, "sig": sig})
        cc.compare(plain["out"], want, ("philox", N, offset))
        placement(dev, call, {"ctrl": ctrl, "sig": sig}, plain, ("philox", N, offset), outs=(False, True))


# ------------------------------------------------------------------------------------------------------------------------
# gradient and sensitivity entries
# ------------------------------------------------------------------------------------------------------------------------

DERIV_N = (2, 7, 10, 12)


def deriv_cases(N, seed):
    rng = np.random.default_rng(seed + N)
    for C, K in ((3, 65), (2, 1)):
        for shared in (False, True):
            ctrl = deloc_rows(rng, C, N)
            yield (N, C, K, "shared" if shared else "per row"), ctrl, SIGMA * rng.standard_normal((1 if shared else C, K, N, 3))


def derivative_entry(be, dev, entry, outputs, N, tag, ctrl, draws, compare_all):
    def make(want):
        return lambda ar, ctrl, draws: entry(ctrl, draws, N, 0, N - 1, want=want)
    inputs = {"ctrl": ctrl, "draws": draws}
    plain = plain_call(dev, make(outputs), inputs)
    compare_all(plain)
    placement(dev, make(outputs), inputs, plain, (tag, outputs))
    only = plain_call(dev, make(("mean",)), inputs)
    assert list(only) == ["mean"] and same_bits(only["mean"], plain["mean"]), (tag, "the mean alone")
    placement(dev, make(("mean",)), inputs, only, (tag, "mean alone"))


@pytest.mark.parametrize("N", DERIV_N)
def test_mc_fidelity_grad(be, dev, N):
    for tag, ctrl, draws in deriv_cases(N, 44000):
        Fw, Gw = gc.grad_eigh(ctrl, draws, N, 0, N - 1)
        teeth(Fw, draws.shape[1], tag)
        derivative_entry(be, dev, be.mc_fidelity_grad, be.GRAD_OUTPUTS, N, tag, ctrl,
                         draws, lambda got: gc._compare_with_reference(got, ctrl, draws, Fw, Gw, N, None, None, tag))


@pytest.mark.parametrize("N", DERIV_N)
def test_mc_fidelity_sens(be, dev, N):
    for tag, ctrl, draws in deriv_cases(N, 45000):
        Fw, Sw = sc.sens_eigh(ctrl, draws, N, 0, N - 1)
        teeth(Fw, draws.shape[1], tag)
        derivative_entry(be, dev, be.mc_fidelity_sens, be.SENS_OUTPUTS, N, tag, ctrl, draws,
                         lambda got: sc._compare_with_reference(got, ctrl, draws, Fw, Sw, N, tag))


@pytest.mark.parametrize("N", (7, 12))
def test_mc_fidelity_grad_philox(be, dev, N):
    K, offset = 65, 7
    ctrl = gc.philox_ctrl(N)                                             # C = 3: row 1 NaN, row 2 with a negative time entry
    for shared in (False, True):
        tag = ("grad philox", N, "shared" if shared else "per row")
        draws, Fw, Gw = gc.reference_on_host_draws(ctrl, K, N, 0, N - 1, offset, shared)
        cc.assert_has_teeth(Fw, what=tag)

        def call(ar, ctrl):
            return be.mc_fidelity_grad_philox(ctrl, K, N, 0, N - 1, gc.PHILOX_SEED, offset=offset, sigma=gc.PHILOX_SIGMA, shared=shared)
        plain = plain_call(dev, call, {"ctrl": ctrl})
        gc._compare_with_reference(plain, ctrl, draws, Fw, Gw, N, None, None, tag)
        ok = [0, 2]                                                      # the moment sums against host sums of the same launch
        bound = K * gc.EPS * max(1.0, float(np.abs(plain["grad"][ok]).max()))
        assert np.abs(plain["moment"][ok] - gc.host_moments(plain)[ok]).max() <= bound and np.isnan(plain["moment"][1]).all(), tag
        placement(dev, call, {"ctrl": ctrl}, plain, tag)


@pytest.mark.parametrize("N", (7, 12))
def test_mc_fidelity_sens_philox(be, dev, N):
    K, offset = 65, 7
    ctrl = sc.philox_ctrl(N)
    draws, Fw, Sw = sc.reference_on_host_draws(ctrl, K, N, 0, N - 1, offset)
    cc.assert_has_teeth(Fw, what=("sens philox", N))

    def call(ar, ctrl):
        return be.mc_fidelity_sens_philox(ctrl, K, N, 0, N - 1, sc.PHILOX_SEED, offset=offset, sigma=sc.PHILOX_SIGMA)
    plain = plain_call(dev, call, {"ctrl": ctrl})
    sc._compare_with_reference(plain, ctrl, draws, Fw, Sw, N, ("sens philox", N))
    placement(dev, call, {"ctrl": ctrl}, plain, ("sens philox", N))


@pytest.mark.parametrize("N", (7, 12))
def test_mc_fidelity_grad_listed(be, dev, N):
    K, offset = 130, 7
    full = lsc.Full(gc.philox_ctrl(N), K, N, 0, N - 1, offset=offset)
    full.teeth(("listed", N))
    rng = np.random.default_rng(46000 + N)
    for L in (1, 65):
        listed = lsc.random_list(rng, 3, L, K, empties=L > 1)
        weights = rng.uniform(-1.0, 2.0, (3, L))
        if L > 1:
            assert ((listed < 0) | (listed >= K)).any() and (listed[:, 0] == listed[:, 1]).all()

        def call(ar, ctrl, listed, weights):
            return be.mc_fidelity_grad_listed(ctrl, K, listed, weights, nspin=N, inspin=0, outspin=N - 1, seed=lsc.SEED, offset=offset,
                                              sigma=lsc.SIGMA)
        inputs = {"ctrl": full.ctrl, "listed": listed, "weights": weights}
        plain = plain_call(dev, call, inputs)
        assert sorted(plain) == ["fid", "grad", "sum"]
        lsc.compare(plain, full, listed, weights, ("listed", N, L))
        placement(dev, call, inputs, plain, ("listed", N, L))


# ------------------------------------------------------------------------------------------------------------------------
# readout-time grids
# ------------------------------------------------------------------------------------------------------------------------

GRIDS = {1: (np.array([1.1]), np.array([0.25]), np.array([0.7])),
         3: (np.array([0.8, 1.0, 1.2]), np.array([0.0, -0.25, 0.5]), np.array([0.4, 0.3, -0.1]))}
TIMES_SEED = 0x5EED00A8


def compare_times(got, want, weights, tag):
    cc.compare(got["fid"], want, (tag, "slabs"))
    assert np.array_equal(got["min"], got["fid"].min(axis=0), equal_nan=True), (tag, "min")
    assert np.array_equal(got["wsum"], tc.weighted_sum(weights, got["fid"]), equal_nan=True), (tag, "wsum")
    assert np.isnan(got["min"][1]).all() and np.isnan(got["wsum"][1]).all() and np.isnan(got["fid"][:, 1]).all(), (tag, "NaN row")


@pytest.mark.parametrize("N", (2, 7, 16))
def test_mc_fidelity_times(be, dev, N):
    rng = np.random.default_rng(47000 + N)
    ctrl = deloc_rows(rng, 3, N)
    draws = SIGMA * rng.standard_normal((3, 65, N, 3))
    for M, (tscale, tshift, weights) in GRIDS.items():
        want = tc.reference_slabs(ctrl, draws, N, 0, N - 1, tscale, tshift)
        cc.assert_has_teeth(want, what=("times", N, M))

        def call(ar, ctrl, draws):
            return be.mc_fidelity_times(ctrl, draws, N, 0, N - 1, tscale=tscale, tshift=tshift, weights=weights, want=be.TIMES_OUTPUTS)
        plain = plain_call(dev, call, {"ctrl": ctrl, "draws": draws})
        compare_times(plain, want, weights, ("times", N, M))
        placement(dev, call, {"ctrl": ctrl, "draws": draws}, plain, ("times", N, M))


@pytest.mark.parametrize("N", (2, 7, 16))
def test_mc_fidelity_times_philox(be, dev, N):
    rng = np.random.default_rng(48000 + N)
    ctrl = deloc_rows(rng, 3, N)
    draws = gc.host_draws(TIMES_SEED, 7, (3, 65, N, 3), SIGMA)
    for M, (tscale, tshift, weights) in GRIDS.items():
        want = tc.reference_slabs(ctrl, draws, N, 0, N - 1, tscale, tshift)
        cc.assert_has_teeth(want, what=("times philox", N, M))

        def call(ar, ctrl):
            return be.mc_fidelity_times_philox(ctrl, 65, N, 0, N - 1, TIMES_SEED, offset=7, sigma=SIGMA, tscale=tscale, tshift=tshift,
                                               weights=weights, want=be.TIMES_OUTPUTS)
        plain = plain_call(dev, call, {"ctrl": ctrl})
        compare_times(plain, want, weights, ("times philox", N, M))
        placement(dev, call, {"ctrl": ctrl}, plain, ("times philox", N, M))


# ------------------------------------------------------------------------------------------------------------------------
# the arena sees DEVICE stores (tests/test_arena.py shows the same on CPU tensors): an entry is handed, as its `out=`, a view that
# is deliberately one element off the body - the kernel stays inside the view it was given, and inside memory the test owns
# ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shift", (0, 1))
def test_arena_sees_device_stores(be, dev, shift):
    import torch
    n = 515

    def run(delta, length):
        ar = Arena(shift=shift, device=dev)
        body = ar.empty((n,), dtype=torch.float64, device=dev)
        view = torch.as_strided(body, (length,), (1,), body.storage_offset() + delta)
        be.philox_normal((length,), PHILOX_SEED, scale=SIGMA, out=view)
        return ar, body
    ar, body = run(0, n)
    ar.check_guards()
    ar.assert_written(body)
    ar, body = run(0, n + 1)                                             # one element past the end
    with pytest.raises(AssertionError, match=r"block #0 empty float64\[515\], after the body, 1 word\(s\) changed, the nearest 1 element"):
        ar.check_guards()
    ar.assert_written(body)
    ar, body = run(-1, n)                                                # one element early: a guard word hit, the last element left alone
    with pytest.raises(AssertionError, match=r"block #0 empty float64\[515\], before the body, 1 word\(s\) changed, the nearest 1 element"):
        ar.check_guards()
    with pytest.raises(AssertionError, match=r"unwritten: 1 of 515 element\(s\) .* the first at flat index 514"):
        ar.assert_written(body)
    ar, body = run(n + 4095, 1)                                          # the outermost guard word
    with pytest.raises(AssertionError, match=r"after the body, 1 word\(s\) changed, the nearest 4096 element"):
        ar.check_guards()


# ------------------------------------------------------------------------------------------------------------------------
# draws
# ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n, offset", [(1, 0), (1, 1), (2, 1), (512, 0), (515, 7)])
def test_philox_normal(be, dev, n, offset):
    """(1, 1), (2, 1), (515, 7): the stream starts and / or ends inside a Box-Muller pair, whose other half must not be stored"""
    want = philox_host.philox_normal(PHILOX_SEED, offset, n, SIGMA)

    def call(ar, out=False):
        import torch
        if out:
            return be.philox_normal((n,), PHILOX_SEED, scale=SIGMA, offset=offset, out=torch.empty((n,), dtype=torch.float64, device=dev))
        return be.philox_normal((n,), PHILOX_SEED, scale=SIGMA, offset=offset, device=dev, as_torch=True)
    plain = plain_call(dev, call, {})
    assert plain["out"].shape == (n,) and np.abs(plain["out"] - want).max() < 1e-15
    placement(dev, call, {}, plain, ("philox_normal", n, offset), outs=(False, True))


@pytest.mark.parametrize("periods, period, skip", [(1, 1, 0), (3, 7, 1), (2, 700, 3)])
def test_legacy_normal_periods(be, dev, periods, period, skip):
    """NumPy's own stream is the reference; (2, 700, 3) crosses a 624-word block of the generator.  Every run starts from the same
    saved state (with a cached normal), and the global state is put back afterwards."""
    scales = np.linspace(0.02, 0.1, periods)
    saved = np.random.get_state()
    try:
        np.random.seed(4900 + period)
        np.random.normal()
        start = np.random.get_state()
        assert start[3] == 1
        want = np.stack([np.random.normal(scale=scales[p], size=period)[skip:] for p in range(periods)])
        end = np.random.get_state()
        ends = []

        def call(ar, out=False):
            import torch
            np.random.set_state(start)
            o = torch.empty((periods, period - skip), dtype=torch.float64, device=dev) if out else None
            res = be.legacy_normal_periods(periods, period, skip, scales, out=o, device=dev)
            ends.append(np.random.get_state())
            return res
        plain = plain_call(dev, call, {})
        assert be.legacy_device_exact() and np.array_equal(plain["out"], want)
        placement(dev, call, {}, plain, ("legacy", periods, period, skip), outs=(False, True))
        for st in ends:
            assert np.array_equal(st[1], end[1]) and st[2:] == end[2:]
    finally:
        np.random.set_state(saved)


def directional_layout(N, idx, ab):
    """(draws (n, N, 3), diag_imag (n, N)) of directional samples given by (direction index, a, b): the reference's direction
    list and element pair restated with NumPy (as in tests/test_gpu_directional.py)"""
    dirs = [(0, 0), (N - 1, N - 1)] + [(d, d + o) for d in range(1, N - 1) for o in (-1, 0, 1)] + [(0, 1), (1, 0), (N - 2, N - 1), (N - 1, N - 2)]
    draws, imag = np.zeros((idx.size, N, 3)), np.zeros((idx.size, N))
    for s in range(idx.size):
        (p, q), (a, b) = dirs[idx[s]], ab[s]
        if p == q:
            draws[s, p, 0], imag[s, p] = a, -b
        elif p == q + 1:
            draws[s, p, 1], draws[s, p, 2] = a, b
        else:
            draws[s, q, 1], draws[s, q, 2] = a, -b
    return draws, imag, len(dirs)


def test_directional(be, dev):
    """`directional_draws_device` (NumPy's calls are the reference), then `mc_fidelity_directional` on its output placed in the arena
    (the oracle's per-sample expm of the dense matrix is the reference)"""
    N, C, K = 7, 2, 65
    n, ndir = C * K, 3 * N
    saved = np.random.get_state()
    try:
        np.random.seed(5000)
        np.random.normal()
        start = np.random.get_state()
        want_idx, want_ab = np.empty(n, dtype=np.int32), np.empty((n, 2))
        for i in range(n):
            want_idx[i] = np.random.randint(low=0, high=ndir)
            want_ab[i] = np.random.normal(scale=SIGMA, size=2)
        end = np.random.get_state()
        ends = []

        def call(ar):
            np.random.set_state(start)
            res = be.directional_draws_device(n, ndir, SIGMA, device=dev)
            ends.append(np.random.get_state())
            return res
        plain = plain_call(dev, call, {})
        assert be.legacy_device_exact() and np.array_equal(plain["0"], want_idx) and np.array_equal(plain["1"], want_ab)
        assert plain["0"].dtype == np.int32
        placement(dev, call, {}, plain, "directional draws")
        for st in ends:
            assert np.array_equal(st[1], end[1]) and st[2:] == end[2:]
    finally:
        np.random.set_state(saved)
    ctrl = deloc_rows(np.random.default_rng(5001), C, N)
    idx, ab = want_idx.copy(), want_ab
    idx[:ndir] = np.arange(ndir)                                         # every direction at least once
    draws, imag, nd = directional_layout(N, idx, ab)
    assert nd == ndir
    want = orc.fidelity_expm_loop(ctrl, draws.reshape(C, K, N, 3), N, 0, N - 1, diag_imag=imag.reshape(C, K, N))
    cc.assert_has_teeth(want, what="directional")

    def entry(ar, ctrl, idx, ab, out=False):
        import torch
        o = torch.empty((C, K), dtype=torch.float64, device=dev) if out else None
        return be.mc_fidelity_directional(ctrl, idx, ab, N, 0, N - 1, K, out=o)
    inputs = {"ctrl": ctrl, "idx": idx, "ab": ab}
    plain = plain_call(dev, entry, inputs)
    assert (np.abs(plain["out"] - want) / np.maximum(1.0, want)).max() < 1e-10
    placement(dev, entry, inputs, plain, "directional entry", outs=(False, True))


def test_mc_fidelity_nonhermitian(be, dev):
    N, C, K = 5, 2, 65
    rng = np.random.default_rng(5100)
    ctrl = deloc_rows(rng, C, N)
    draws = SIGMA * rng.standard_normal((C, K, N, 3))
    imag = 0.1 * rng.standard_normal((C, K, N))
    want = orc.fidelity_expm_loop(ctrl, draws, N, 0, N - 1, diag_imag=imag)
    cc.assert_has_teeth(want, what="non-Hermitian")

    def call(ar, ctrl, draws, imag):
        return be.mc_fidelity_nonhermitian(ctrl, draws, imag, N, 0, N - 1)
    inputs = {"ctrl": ctrl, "draws": draws, "imag": imag}
    plain = plain_call(dev, call, inputs)
    assert np.abs(plain["out"] - want).max() < 1e-10 * max(1.0, np.abs(want).max())
    placement(dev, call, inputs, plain, "non-Hermitian")


# ------------------------------------------------------------------------------------------------------------------------
# what is made of the fidelities: reductions, the row sort, p-RIM, the tail, the bootstrap
# ------------------------------------------------------------------------------------------------------------------------


def reduce_slab(K, C, thr):
    """grid rows of reduce_checks (exact integer reference); C >= 3: the middle row all NaN"""
    J, nan = rc.grid_slab(K, C, thr if len(thr) else (0.75,), 0)
    if C >= 3:
        nan[C // 2] = True
    return J, nan


@pytest.mark.parametrize("C, K", [(3, 65), (2, 1), (2, 16385)])
def test_reduce_metrics(be, dev, C, K):
    """K = 16385: the first row length on the bitonic route, which pads its rows with +inf to 2^15 in a workspace"""
    for thr in ((), (0.75, 1.0)):
        F, thr_a, ref = rc.case(("placement", K, C, len(thr)), lambda: reduce_slab(K, C, thr), rc.GRID, 16, thr)
        F = F.copy()                                                     # (the shared case is read-only)
        srt = np.sort(F, axis=1)
        for overlapped in (True, False):
            tag = ("reduce", C, K, len(thr), overlapped)

            def call(ar, fid):
                return be.reduce_metrics(fid, q_thresholds=thr_a, dkw_eps=rc.EPS, want_sorted=True, overlapped=overlapped)
            plain = plain_call(dev, call, {"fid": F})
            rc.compare(plain, ref, tag)
            ok = ~np.isnan(F).any(axis=1)
            assert np.array_equal(plain["sorted"][ok], srt[ok]) and plain["sorted"][~ok].tobytes() == F[~ok].tobytes(), tag
            placement(dev, call, {"fid": F}, plain, tag)
    # the packed form: `out=` is the (15, R) tensor itself, the library's two thresholds (not on the grid: the counts by NumPy)
    F, _, ref = rc.case(("placement", K, C, 2), lambda: reduce_slab(K, C, (0.75, 1.0)), rc.GRID, 16, (0.75, 1.0))
    F = F.copy()
    for overlapped in (True, False):
        def packed(ar, fid, out=False):
            import torch
            o = torch.empty((be.PACKED_ROWS, C), dtype=torch.float64, device=dev) if out else None
            return be.reduce_packed(fid, rc.EPS, out=o, overlapped=overlapped)
        plain = plain_call(dev, packed, {"fid": F})
        P = plain["out"]                                                 # (backend.packed_views, on the host copy)
        views = {"rim1": P[0:3], "std": P[3:6], "min": P[6:9], "q": P[9:15].reshape(3, 2, C)}
        q = np.stack([np.stack([((np.clip(F + s, 0.0, 1.0) >= t) & ~np.isnan(F)).sum(axis=1) / K for t in be.Q_THRESHOLDS])
                      for s in (0.0, -rc.EPS, rc.EPS)])
        rc.compare(views, dict(ref, q=q), ("packed", C, K, overlapped))
        placement(dev, packed, {"fid": F}, plain, ("packed", C, K, overlapped), outs=(False, True))


def test_rim_p(be, dev):
    import mpmath
    C, K, p = 3, 65, 2.5
    u = np.random.default_rng(5200).integers(1, rc.GRID + 1, (C, K))
    F = 1.0 - u / float(rc.GRID)                                         # exact
    F[1] = np.nan

    def call(ar, fid):
        return be.rim_p(fid, p)
    plain = plain_call(dev, call, {"fid": F})
    with mpmath.workdps(40):
        for c in (0, 2):
            e = (mpmath.fsum((mpmath.mpf(int(v)) / rc.GRID) ** mpmath.mpf(p) for v in u[c]) / K) ** mpmath.mpf(1.0 / p)
            assert float(abs(mpmath.mpf(float(plain["out"][c])) - e) / e) <= rc.rimp_bound(K, p), c
    assert np.isnan(plain["out"][1]) and plain["out"].shape == (C,)
    placement(dev, call, {"fid": F}, plain, "rim_p")


@pytest.mark.parametrize("alpha, m", [(0.5 / 65, 1), (0.25, 17), (0.995, 65)])
def test_tail_select(be, dev, alpha, m):
    C, K = 3, 65
    F = np.random.default_rng(5300).random((C, K))
    F[1, 40] = np.nan
    assert tsc.tail_len(K, alpha) == m
    exp = dict(zip(("list", "weight", "var"), tsc.expected(F, alpha)))
    for want in (be.TAIL_SELECT_OUTPUTS, ("list",)):
        def call(ar, fid):
            return be.tail_select(fid, alpha, want=want)
        plain = plain_call(dev, call, {"fid": F})
        assert sorted(plain) == sorted(want)
        for k in want:
            assert plain[k].dtype == exp[k].dtype and np.array_equal(plain[k], exp[k], equal_nan=(k == "var")), (alpha, k)
        assert (plain["list"][1] == -1).all()
        placement(dev, call, {"fid": F}, plain, ("tail_select", alpha, want))


def boot_rows():
    """C = 3 rows that are permutations of j / 64, j = 0 .. 64, the middle one with a NaN: the row mean is exactly 1 / 2, every
    g = f - m a multiple of 2^-6 and every g^2 one of 2^-12, so all sums of K = 65 of them are exact in any order
    (bootstrap_checks.exact_rows at K = 65)"""
    rng = np.random.default_rng(5400)
    F = np.stack([rng.permutation(65) / 64.0 for _ in range(3)])
    g = F - F.sum(axis=1, keepdims=True) / 65
    assert (F.sum(axis=1) / 65 == 0.5).all() and np.all(g * 64.0 == np.round(g * 64.0))
    F[1, 30] = np.nan
    return F


@pytest.mark.parametrize("route", ("lds", "global"))
def test_bootstrap_metrics(be, dev, route):
    F, B, seed, offset, thr = boot_rows(), 3, 0x5EED00A9, 7, (0.25, 0.5)
    want = bc.ref_exact_replicates(F, B, seed, offset, thr)
    full = None
    for outputs in (be.BOOTSTRAP_OUTPUTS, ("replicates",), ("summary",)):
        def call(ar, fid):
            return be.bootstrap_metrics(fid, B, seed, offset=offset, q_thresholds=thr, want=outputs, route=route)
        plain = plain_call(dev, call, {"fid": F})
        assert sorted(plain) == sorted(outputs)
        if full is None:
            full = plain
            rep, s = plain["replicates"], plain["summary"]
            assert rep.shape == want.shape == (5, 3, B) and s.shape == (5, 4, 3)
            for j in (0, 2, 3, 4):                                       # (bootstrap_checks.assert_exact_against_host)
                assert rep[j].tobytes() == want[j].tobytes(), (route, j)
            ok = [0, 2]
            assert np.all(np.abs(rep[1][ok] ** 2 - want[1][ok]) <= 2.0 * np.spacing(want[1][ok])) and np.isnan(rep[:, 1]).all()
            assert len(np.unique(rep[0][ok])) > 3
            # the summary against NumPy on the entry's own replicates (bootstrap_checks.check_summary_against_numpy; ranks 0 and B - 1)
            assert np.isnan(s[:, :, 1]).all()
            for j in range(5):
                for c in ok:
                    x = rep[j, c]
                    scale = np.abs(x).max()
                    assert s[j, 2, c] == x.min() and s[j, 3, c] == x.max(), (route, j, c)
                    assert abs(s[j, 0, c] - math.fsum(x) / B) <= B * bc.U * scale, (route, j, c)
                    var = math.fsum((x - math.fsum(x) / B) ** 2) / (B - 1)
                    assert abs(s[j, 1, c] ** 2 - var) <= 4 * B * bc.U * max(1.0, scale ** 2), (route, j, c)
        else:
            assert all(same_bits(plain[k], full[k]) for k in outputs), (route, outputs)
        placement(dev, call, {"fid": F}, plain, ("bootstrap", route, outputs))


# ------------------------------------------------------------------------------------------------------------------------
# the batched L-BFGS state machine, fed by the gradient entry
# ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("boxed", (False, True), ids=("unbounded", "boxed"))
@pytest.mark.parametrize("N, m", [(3, 1), (3, 5), (12, 1), (12, 5)])
def test_lbfgs(be, dev, N, m, boxed):
    """init, three advance steps on the "mean" rows of `mc_fidelity_grad_philox` at the trial points, result: every guard after
    every call, the state's own content against the definition (lbfgs.py) bit for bit"""
    lbfgs = lc.lbfgs
    C, n, K, steps = 5, N + 1, 65, 3
    rng = np.random.default_rng(5500 + 10 * N + m)
    x0 = cc.deloc_ctrl(rng, C, N, 0.5)
    x0[2, N // 2] = np.nan
    mask = np.ones((C, n))
    mask[::3, n - 1] = 0.0
    lo, hi = np.full((C, n), -0.35), np.full((C, n), 0.35)
    lo[:, N], hi[:, N] = np.nan_to_num(x0[:, N]) - 1.0, np.nan_to_num(x0[:, N]) + 0.5
    inputs = {"x0": x0, "mask": mask}
    if boxed:
        inputs.update(lo=lo, hi=hi)

    def call(ar, x0, mask, lo=None, hi=None):
        check = ar.check_guards if ar is not None else (lambda: None)
        bounds = (lo, hi) if boxed else None
        out = {}
        state, trial = be.lbfgs_init(x0, mask, m=m, bounds=bounds)
        check()
        out["state0"], out["trial0"] = state.clone(), trial.clone()
        for i in range(1, steps + 1):
            mean = be.mc_fidelity_grad_philox(trial, K, N, 0, N - 1, gc.PHILOX_SEED, sigma=SIGMA, want=("mean",))["mean"]
            check()
            be.lbfgs_advance(state, trial, mean, None, m=m, kind="one_minus", bounds=bounds)
            check()
            out[f"mean{i}"], out[f"state{i}"], out[f"trial{i}"] = mean, state.clone(), trial.clone()
        out.update(be.lbfgs_result(state, trial, m=m))
        check()
        out["state"], out["trial"] = state, trial
        return out
    plain = plain_call(dev, call, inputs)
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    mc = lbc.definition(x0, mask, lo, hi, m=m) if boxed else lc.definition(x0, mask, m=m)
    assert same(plain["state0"], mc.state_array()) and same(plain["trial0"], mc.trial), "init"
    for i in range(1, steps + 1):
        mc.advance(*lbfgs.objective("one_minus", plain[f"mean{i}"]))
        assert same(plain[f"state{i}"], mc.state_array()) and same(plain[f"trial{i}"], mc.trial), ("advance", i)
    assert same(plain["x"], mc.x) and same(plain["f"], mc.f) and same(plain["grad"], mc.g)
    assert np.array_equal(plain["status"], mc.status) and np.array_equal(plain["iters"], mc.iters) and np.array_equal(plain["evals"], mc.evals)
    assert plain["status"].dtype == np.int32 and plain["iters"].dtype == np.int64 and plain["status"][2] == 5 and (mc.evals >= steps).any()
    placement(dev, call, inputs, plain, ("lbfgs", N, m, boxed), unchecked=tuple(k for k in plain if k.startswith("state")))
