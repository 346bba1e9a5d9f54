"""References, bounds and data-level checks of the listed-sample weighted fidelity gradient (`backend.mc_fidelity_grad_listed`),
shaped like grad_checks.py: the `check_*` functions take a backend object, the GPU tests run them on the device, and a CPU test
runs them on a NumPy stand-in, where they must pass, and on broken ones, where they must fail.

Reference.  grad_checks.grad_eigh (numpy.linalg.eigh on the dense complex Hamiltonian) on ALL K draws of every row, regenerated on
the host with oracle/philox_host.py, then gathered through the list - computed once per case and shared by the list lengths.

Bounds (the project's).  Per sample: 1e-10 absolute on F, 1e-10 max(1, |T|) on a bias entry, 1e-10 max(1, ||H||) on the time entry
(grad_checks.grad_bars).  For a weighted sum of L slots:  sum_j |w_j| bar_j  +  L 2^-52 sum_j |w_j g_j|  - every term inside its
bar, plus the rounding of L - 1 additions of terms of that size."""
import numpy as np

import chain_checks as cc
import grad_checks as gc
from oracle import robchar_oracle as orc

TOL, EPS = gc.TOL, gc.EPS
SEED, SIGMA = gc.PHILOX_SEED, gc.PHILOX_SIGMA
OUTPUTS = ("fid", "grad", "sum")
LENGTHS = (1, 63, 64, 65, 129)


# ------------------------------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------------------------------


def full_draws(C, K, N, offset, shared, sigma):
    """(C, K, N, 3) host draws of either stream convention; `sigma` a float or one value per row"""
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (C,))
    if shared:
        return gc.host_draws(SEED, offset, (1, K, N, 3), 1.0) * sig[:, None, None, None]
    return gc.host_draws(SEED, offset, (C, K, N, 3), sig)


class Full:
    """The reference on all K draws of every row: draws, F (C, K), G (C, K, N+1), bars (C, K, N+2) = (F's bar, the gradient's)"""

    def __init__(self, ctrl, K, N, a, b, offset=0, shared=False, h0d=None, h0o=None, sigma=SIGMA):
        self.ctrl, self.K, self.N, self.a, self.b = np.asarray(ctrl, dtype=np.float64), K, N, a, b
        self.kw = dict(offset=offset, shared=shared, h0_diag=h0d, h0_offdiag=h0o, sigma=sigma)
        self.draws = full_draws(self.ctrl.shape[0], K, N, offset, shared, sigma)
        self.F, self.G = gc.grad_eigh(self.ctrl, self.draws, N, a, b, h0d, h0o)
        gb = gc.grad_bars(self.ctrl, self.draws, N, h0d, h0o)
        self.bars = np.concatenate([np.full(gb.shape[:2] + (1,), TOL), gb], axis=2)
        self.nan = np.isnan(self.ctrl).any(axis=1)

    def teeth(self, what):
        """the comparison must be able to fail: median F >= 1e-2 and median |dF/dx| >= 1e-2 over the non-NaN rows"""
        mf = float(np.median(self.F[~self.nan]))
        mg = float(np.median(np.abs(self.G[~self.nan])))
        assert mf >= 1e-2 and mg >= 1e-2, ("the reference cannot tell a wrong kernel from a right one", what, mf, mg)

    def gather(self, listed, weights=None):
        """(fid (C, L), grad (C, L, N+1), sum (C, N+2), bars (C, L, N+2), sum bar (C, N+2)) of a list"""
        listed = np.asarray(listed)
        C, L = listed.shape
        ok = (listed >= 0) & (listed < self.K)
        idx = np.where(ok, listed, 0)
        V = np.concatenate([self.F[..., None], self.G], axis=2)                     # (C, K, N+2)
        Vl = np.take_along_axis(V, idx[..., None], 1)
        Bl = np.take_along_axis(self.bars, idx[..., None], 1)
        Vl[~ok] = np.nan
        Bl[~ok] = 1.0
        w = np.ones((C, L)) if weights is None else np.asarray(weights, dtype=np.float64)
        w = np.where(ok, w, 0.0)[..., None]
        terms = w * np.where(ok[..., None], Vl, 0.0)
        total = terms.sum(axis=1)
        total[self.nan] = np.nan
        sbar = (np.abs(w) * np.where(ok[..., None], Bl, 0.0)).sum(axis=1) + L * EPS * np.abs(terms).sum(axis=1)
        sbar[self.nan] = 1.0                                                       # (NaN row: the NaN pattern is what is compared)
        Bl[self.nan] = 1.0
        return Vl[..., 0], Vl[..., 1:], total, Bl, sbar + 1e-300


def run(be, full, listed, weights=None, want=OUTPUTS, **over):
    kw = dict(full.kw, **over)
    return gc.to_host(be.mc_fidelity_grad_listed(full.ctrl, full.K, np.asarray(listed, dtype=np.int32), weights, nspin=full.N,
                                                 inspin=full.a, outspin=full.b, seed=SEED, want=want, **kw))


def compare(got, full, listed, weights, what):
    """every output that `got` holds against the gathered reference; returns the worst error / bar"""
    Fw, Gw, Sw, bars, sbar = full.gather(listed, weights)
    worst = 0.0
    if "fid" in got:
        assert got["fid"].shape == Fw.shape, (what, "fid shape")
        assert np.array_equal(np.isnan(got["fid"]), np.isnan(Fw)), (what, "fid", "NaN pattern")
        err = float(np.nanmax(np.abs(got["fid"] - Fw), initial=0.0))
        assert err < TOL, (what, "fid", err)
        worst = max(worst, err / TOL)
    if "grad" in got:
        worst = max(worst, gc.compare_grad(got["grad"], Gw, bars[..., 1:], (what, "grad"))[1])
    if "sum" in got:
        worst = max(worst, gc.compare_grad(got["sum"], Sw, sbar, (what, "sum"))[1])
    return worst


def random_list(rng, C, L, K, empties=True):
    """draws of a row in random order WITH repeats; about one slot in six empty (-1, K, K + 7, a large negative value)"""
    listed = rng.integers(0, K, (C, L)).astype(np.int32)
    if L >= 3:
        listed[:, 1] = listed[:, 0]                                    # a repeat in every row
    if empties:
        hole = rng.random((C, L)) < 1.0 / 6.0
        if L >= 3:
            hole[:, :2] = False
            hole[:, 2] = True
        listed[hole] = rng.choice(np.array([-1, K, K + 7, -2 ** 31], dtype=np.int64), int(hole.sum())).astype(np.int32)
    return listed


# ------------------------------------------------------------------------------------------------------------------------
# a NumPy stand-in backend and broken variants of it, for the checks' own CPU tests
# ------------------------------------------------------------------------------------------------------------------------


class StandIn(gc.StandIn):
    """`mc_fidelity_grad_listed` (and, from grad_checks.StandIn, `mc_fidelity_grad_philox`) on the CPU.  broken: None,
    "weights_ignored" (w = 1), "empty_counted" (an empty slot is taken as draw 0), "index_as_slot" (slot s takes draw s, not
    list[s]), "row_offset_dropped" (every row takes row 0's draws: c K missing in the stream element), "sum_64_tiles" (the
    row sums stop after 64 tiles of 64 slots)."""

    def __init__(self, broken=None):
        super().__init__(None)
        self.how = broken

    def mc_fidelity_grad_listed(self, ctrl, K, listed, weights=None, *, nspin, inspin, outspin, seed, offset=0, sigma=0.05,
                                shared=False, h0_diag=None, h0_offdiag=None, want=OUTPUTS):
        assert seed == SEED
        ctrl = np.asarray(ctrl, dtype=np.float64)
        full = Full(ctrl, K, nspin, inspin, outspin, offset, shared, h0_diag, h0_offdiag, sigma)
        if self.how == "row_offset_dropped" and not shared:
            sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (ctrl.shape[0],))
            unit = gc.host_draws(SEED, offset, (1, K, nspin, 3), 1.0)
            full.draws = unit * sig[:, None, None, None]
            full.F, full.G = gc.grad_eigh(ctrl, full.draws, nspin, inspin, outspin, h0_diag, h0_offdiag)
        listed = np.array(listed, dtype=np.int64)
        L = listed.shape[1]
        if self.how == "index_as_slot":
            listed = np.where((listed >= 0) & (listed < K), np.arange(L)[None, :] % K, listed)
        if self.how == "empty_counted":
            listed = np.where((listed >= 0) & (listed < K), listed, 0)
        if self.how == "weights_ignored":
            weights = None
        F, G, S, _, _ = full.gather(listed, weights)
        if self.how == "sum_64_tiles":
            S = full.gather(listed[:, :4096], None if weights is None else np.asarray(weights)[:, :4096])[2]
        res = {"fid": F, "grad": G, "sum": S}
        return {k: res[k] for k in want}


# ------------------------------------------------------------------------------------------------------------------------
# checks (backend in, assertion out)
# ------------------------------------------------------------------------------------------------------------------------

C_ROWS, K_DRAWS = 3, 200


def pairs(N):
    return gc.grad_pairs(N)[:2]


def check_reference(be, N, lengths=LENGTHS, report=None):
    """Delocalised rows (one NaN, one with a negative time entry), two (in, out) pairs, every length of `lengths`: random lists
    with repeats and empty slots, random weights of both signs - fid, grad and sum against the reference."""
    ctrl = gc.philox_ctrl(N, C=C_ROWS)
    rng = np.random.default_rng(4100 + N)
    worst = 0.0
    for (a, b) in pairs(N):
        full = Full(ctrl, K_DRAWS, N, a, b, offset=7)
        full.teeth(("reference", N, a, b))
        for L in lengths:
            listed = random_list(rng, C_ROWS, L, K_DRAWS)
            weights = rng.uniform(-1.0, 2.0, (C_ROWS, L))
            got = run(be, full, listed, weights)
            assert all(np.isnan(got[k][1]).all() for k in OUTPUTS), ("NaN row", N, a, b, L)
            worst = max(worst, compare(got, full, listed, weights, ("reference", N, a, b, L)))
    if report is not None:
        report(f"reference, N = {N}: worst error / bar = {worst:.2e}")


def check_identity(be, N, report=None):
    """list = arange(K), no weights, against `mc_fidelity_grad_philox` on all K draws: fid and grad within the bars, fid within
    64 N eps max(1, T ||H||) (NOT bit-equal: the full launch votes its sweep counts per wave), sum / K within the sum bar of mean."""
    ctrl = gc.philox_ctrl(N, C=C_ROWS)
    a, b = pairs(N)[0]
    full = Full(ctrl, K_DRAWS, N, a, b, offset=7)
    listed = np.tile(np.arange(K_DRAWS, dtype=np.int32), (C_ROWS, 1))
    got = run(be, full, listed)
    ref = gc.to_host(be.mc_fidelity_grad_philox(ctrl, K_DRAWS, N, a, b, SEED, offset=7, sigma=SIGMA, want=("fid", "grad", "mean")))
    ok = ~full.nan
    assert all(np.isnan(got[k][full.nan]).all() for k in OUTPUTS)
    bars = full.bars
    ef = np.abs(got["fid"][ok] - ref["fid"][ok])
    eg = np.abs(got["grad"][ok] - ref["grad"][ok])
    assert (ef < bars[ok][..., 0]).all() and (eg < bars[ok][..., 1:]).all(), ("identity list", N, float(ef.max()), float(eg.max()))
    cz = np.nan_to_num(ctrl)
    d = cz[:, None, :N] + full.draws[..., 0]
    e = np.hypot(1.0 + full.draws[:, :, 1:, 1], full.draws[:, :, 1:, 2])
    norm = np.abs(d).max(-1) + 2.0 * e.max(-1)                                      # ||H|| per sample, as in grad_checks.grad_bars
    tight = 64 * N * EPS * np.maximum(1.0, np.abs(cz[:, N])[:, None] * norm)
    assert (ef <= tight[ok]).all(), ("identity list: fid against the header's bound", N, float((ef / tight[ok]).max()))
    sbar = full.gather(listed)[4]
    es = np.abs(got["sum"][ok] / K_DRAWS - ref["mean"][ok])
    assert (es < sbar[ok]).all(), ("identity list: sum / K against mean", N, float((es / sbar[ok]).max()))
    compare(got, full, listed, None, ("identity list", N))
    if report is not None:
        report(f"identity list, N = {N}: fid {float(ef.max()):.2e} ({float((ef / tight[ok]).max()):.2e} of 64 N eps max(1, T||H||)), "
               f"grad {float(eg.max()):.2e}, differing fid bits in {int((ef > 0).sum())} of {ef.size}")


def check_position_independence(be, N):
    """The same samples in a permuted list, in a longer list padded with empty slots, and alone (L = 1): the same bits."""
    ctrl = gc.philox_ctrl(N, C=C_ROWS, nan_row=None)
    a, b = pairs(N)[0]
    full = Full(ctrl, K_DRAWS, N, a, b, offset=7)
    rng = np.random.default_rng(4300 + N)
    base = np.stack([rng.permutation(K_DRAWS)[:70] for _ in range(C_ROWS)]).astype(np.int32)
    want = ("fid", "grad")
    r0 = run(be, full, base, want=want)
    full.teeth(("position", N))
    assert np.isfinite(r0["fid"]).all()
    perm = rng.permutation(70)
    r1 = run(be, full, base[:, perm], want=want)
    for k in want:
        assert np.array_equal(r1[k], r0[k][:, perm]), ("permuted list", N, k)
    padded = np.full((C_ROWS, 150), -1, dtype=np.int32)
    where = np.sort(rng.permutation(150)[:70])
    padded[:, where] = base
    r2 = run(be, full, padded, want=want)
    for k in want:
        assert np.array_equal(r2[k][:, where], r0[k]), ("padded list", N, k)
        hole = np.ones(150, dtype=bool)
        hole[where] = False
        assert np.isnan(r2[k][:, hole]).all(), ("padded list: empty slots", N, k)
    for s in (0, 37, 69):
        r3 = run(be, full, base[:, s:s + 1], want=want)
        for k in want:
            assert np.array_equal(r3[k][:, 0], r0[k][:, s]), ("alone", N, k, s)


def check_weights(be, N=7):
    """weights=None = all-ones weights bit for bit; a second run the same bits; zero weights an exact 0; `want` subsets the same
    bits; a row of only empty slots sums to 0; random weights against the reference."""
    ctrl = gc.philox_ctrl(N, C=C_ROWS)
    a, b = pairs(N)[0]
    full = Full(ctrl, K_DRAWS, N, a, b, offset=7)
    rng = np.random.default_rng(4400 + N)
    L = 130
    listed = random_list(rng, C_ROWS, L, K_DRAWS)
    ok = ~full.nan
    r_none = run(be, full, listed)
    r_ones = run(be, full, listed, np.ones((C_ROWS, L)))
    gc.assert_same_bits(r_ones, r_none, ("ones = None", N), OUTPUTS)
    weights = rng.uniform(-1.0, 2.0, (C_ROWS, L))
    r_w = run(be, full, listed, weights)
    gc.assert_same_bits(run(be, full, listed, weights), r_w, ("second run", N), OUTPUTS)
    compare(r_w, full, listed, weights, ("weights", N))
    # the weights must matter on the reference, or a kernel that ignores them would pass
    gap = np.abs(full.gather(listed, weights)[2][ok] - full.gather(listed)[2][ok])
    assert float(np.median(gap)) >= 1e-2, ("the weights do not change the reference sums enough to be missed", float(np.median(gap)))
    only = run(be, full, listed, weights, want=("sum",))
    assert set(only) == {"sum"}
    gc.assert_same_bits(only, r_w, ("want = sum", N), ("sum",))
    r_zero = run(be, full, listed, np.zeros((C_ROWS, L)), want=("sum",))
    assert (r_zero["sum"][ok] == 0.0).all() and np.isnan(r_zero["sum"][full.nan]).all(), ("zero weights", N)
    empty = listed.copy()
    empty[0] = -1
    r_empty = run(be, full, empty, weights)
    assert (r_empty["sum"][0] == 0.0).all() and np.isnan(r_empty["fid"][0]).all() and np.isnan(r_empty["grad"][0]).all(), "empty row"
    gc.assert_same_bits({"sum": r_empty["sum"][2:]}, {"sum": r_w["sum"][2:]}, ("other rows beside an empty one", N), ("sum",))


def check_long_rows(be, L, N=5, report=None):
    """Rows of 64 / 65 tiles in the second pass (L = 4096: one tile per lane; 4097: a second step of the strided loop),
    want = ("sum",): within the sum bar of the host sum of the reference."""
    ctrl = gc.philox_ctrl(N, C=C_ROWS)
    a, b = pairs(N)[0]
    full = Full(ctrl, K_DRAWS, N, a, b, offset=7)
    rng = np.random.default_rng(4500 + L)
    listed = random_list(rng, C_ROWS, L, K_DRAWS)
    listed[:, L - 1] = listed[:, 0]                                    # the last slot counts
    weights = rng.uniform(0.5, 1.5, (C_ROWS, L))
    got = run(be, full, listed, weights, want=("sum",))
    assert set(got) == {"sum"}
    last = full.gather(listed[:, L - 1:], weights[:, L - 1:])
    assert (np.abs(last[2][~full.nan][:, 0]) > 100 * full.gather(listed, weights)[4][~full.nan][:, 0]).all(), "the last slot has no teeth"
    worst = compare(got, full, listed, weights, ("long rows", L))
    if report is not None:
        report(f"long rows, L = {L}: worst error / bar = {worst:.2e}")


def check_modes(be, N=7, report=None):
    """Shared draws; per-row sigma with a sigma = 0 row, where every listed sample equals the nominal value; static terms (XXZ
    diagonal, non-unit couplings); one stream offset past 2^33 - each against the reference, L = 65."""
    rng = np.random.default_rng(4600 + N)
    a, b = pairs(N)[0]
    L = 65
    ctrl = gc.philox_ctrl(N, C=C_ROWS)
    h0d, h0o = gc.static_terms(N, "both")
    sig_rows = np.array([0.0, 0.05, 0.08])
    cases = (("shared", ctrl, dict(shared=True, offset=7)),
             ("sigma rows", gc.philox_ctrl(N, C=C_ROWS, nan_row=None), dict(sigma=sig_rows, offset=7)),
             ("sigma rows, shared", gc.philox_ctrl(N, C=C_ROWS, nan_row=None), dict(sigma=sig_rows, offset=7, shared=True)),
             ("static", gc.philox_ctrl(N, C=C_ROWS, seed=gc.STATIC_CTRL_SEED.get(N)), dict(h0d=h0d, h0o=h0o, offset=7)),
             ("far offset", ctrl, dict(offset=gc.FAR_OFFSET)),
             ("far offset, shared", ctrl, dict(offset=gc.FAR_OFFSET, shared=True)),
             ("wrap offset", ctrl, dict(offset=gc.wrap_offset(N))))
    assert gc.FAR_OFFSET > 2 ** 33
    for name, cx, kw in cases:
        full = Full(cx, K_DRAWS, N, a, b, **kw)
        full.teeth((name, N))
        listed = random_list(rng, C_ROWS, L, K_DRAWS)
        if name == "wrap offset":
            listed[0, :40] = np.arange(40)                                         # the samples around the carry
        weights = rng.uniform(-1.0, 2.0, (C_ROWS, L))
        got = run(be, full, listed, weights)
        worst = compare(got, full, listed, weights, (name, N))
        if name == "static":
            gc.assert_static_teeth(full.F, gc.grad_eigh(cx, full.draws, N, a, b)[0], (name, N))
        if name == "shared":
            # the rows really share the draws on the reference, and differ from the per-row stream
            assert np.array_equal(full.draws[0], full.draws[2]) and not np.array_equal(full.draws[2], Full(cx, K_DRAWS, N, a, b, offset=7).draws[2])
        if name.startswith("sigma rows"):
            nominal = gc.grad_eigh(cx[:1], np.zeros((1, 1, N, 3)), N, a, b)
            okc = (listed[0] >= 0) & (listed[0] < K_DRAWS)
            assert np.abs(got["fid"][0, okc] - nominal[0][0, 0]).max() < TOL and np.ptp(got["fid"][0, okc]) == 0.0, (name, "sigma = 0 row")
            assert np.ptp(got["grad"][0, okc], axis=0).max() == 0.0, (name, "sigma = 0 row: gradient")
        if report is not None:
            report(f"{name}, N = {N}: worst error / bar = {worst:.2e}")


def hard_listed_cases(N, rng):
    """the controllers of grad_checks.hard_inputs for an entry that generates its draws: (name, ctrl, sigma, h0_offdiag) - the
    draw-free inputs at sigma = 0, the cut chain as a static coupling of exactly 0 under random draws"""
    hard = {name: ctrl for name, ctrl, _ in gc.hard_inputs(N, rng)}
    cut = np.ones(N - 1)
    cut[max(1, N // 2) - 1] = 0.0
    return (("uniform", hard["uniform"], 0.0, None), ("mirror", hard["mirror"], 0.0, None), ("clustered", hard["clustered"], 0.0, None),
            ("cut", hard["cut"], 0.05, cut), ("T=0", hard["T=0"], 0.05, None), ("bias 1e3", hard["bias 1e3"], 0.05, None))


def check_hard_inputs(be, N):
    """finite results inside the bars on the inputs a spectral route is most likely to get wrong, every pair of grad_pairs"""
    rng = np.random.default_rng(7700 + N)
    K = 70
    listed = np.concatenate([np.arange(66), [-1, 3, 3, 69]]).astype(np.int32)[None, :]
    for name, ctrl, sigma, h0o in hard_listed_cases(N, rng):
        for (a, b) in gc.grad_pairs(N):
            full = Full(ctrl, K, N, a, b, offset=3, sigma=sigma, h0o=h0o)
            got = run(be, full, listed)
            okc = listed[0] >= 0
            assert np.isfinite(got["fid"][0, okc]).all() and np.isfinite(got["grad"][0, okc]).all() and np.isfinite(got["sum"]).all(), (name, N, a, b)
            compare(got, full, listed, None, ("hard", name, N, a, b))


# ------------------------------------------------------------------------------------------------------------------------
# CVaR: the reference tail, its boundary gap, and what a mean gradient would miss
# ------------------------------------------------------------------------------------------------------------------------


def tail_reference(F, alpha):
    """(listed (C, m), weights (C, m), gap (C,)) of the lower tail of every row of F by a NumPy sort, written independently of
    noise.tail_weights; gap = the distance between the m-th and the (m + 1)-th smallest value (inf when m = K) and, when the m-th
    carries a fractional weight, also between the (m - 1)-th and the m-th: the smaller of the two.  While every value moves by less
    than half of it, list and weights stay what they are."""
    C, K = F.shape
    ak = alpha * K
    m = min(K, int(np.ceil(ak)))
    listed, weights, gap = np.empty((C, m), dtype=np.int32), np.empty((C, m)), np.empty(C)
    for c in range(C):
        order = sorted(range(K), key=lambda k: (F[c, k], k))
        tail = sorted(order[:m])
        listed[c] = tail
        weights[c] = [((ak - (m - 1)) / ak if k == order[m - 1] else 1.0 / ak) for k in tail]
        gap[c] = F[c, order[m]] - F[c, order[m - 1]] if m < K else np.inf
        if m > 1 and ak != m:
            gap[c] = min(gap[c], F[c, order[m - 1]] - F[c, order[m - 2]])
    return listed, weights, gap


def cvar_reference(F, G, alpha):
    """(cvar (C,), grad_cvar (C, N+1), var (C,), gap (C,)) of the empirical distribution of every row"""
    listed, weights, gap = tail_reference(F, alpha)
    Fl = np.take_along_axis(F, listed.astype(np.int64), 1)
    Gl = np.take_along_axis(G, listed.astype(np.int64)[..., None], 1)
    return (weights * Fl).sum(axis=1), (weights[..., None] * Gl).sum(axis=1), Fl.max(axis=1), gap
