"""Checks of the fidelity on a grid of readout times (`backend.mc_fidelity_times`, `backend.readout_times`), the references they
are held to, and a NumPy stand-in of the entry.

The `check_*` functions take a backend object (anything with `mc_fidelity_times`, `readout_times` and `mc_fidelity` like
`code-robchar_amd.backend`): tests/test_gpu_times.py runs them on the device, tests/test_times_checks.py on the stand-in built
on `orc.fidelity_eigh`, where they must pass, and on deliberately broken stand-ins, where they must fail.

Definition under test.  For controller row c with time entry T_c and a grid (tscale, tshift) of M times,
    t_cj = |T_c tscale_j + tshift_j|        (product rounded, then sum, then absolute value: NumPy's own),
    "fid" [M][C][K]: slab j = the ordinary fidelity tensor of the controllers with T replaced by t_cj,
    "wsum" [C][K]:  acc = w_0 F_0; acc = fma(w_j, F_j, acc), j = 1 .. M - 1,
    "min"  [C][K]:  min_j F_j;      a NaN controller row is NaN in every output."""
from fractions import Fraction

import numpy as np

import chain_checks as cc
from oracle import philox_host
from oracle import robchar_oracle as orc

# the grid of the oracle comparison: early and late readout, both signs of the shift
TSCALE = np.array([0.8, 0.9, 1.0, 1.1, 1.2])
TSHIFT = np.array([0.0, -0.25, 0.0, 0.25, 0.5])
# (N, in, out) of the first oracle comparison: the pairs whose guard margins tests/test_times_checks.py records and on whose
# controllers the teeth guards of grad_times_checks.py were measured
PAIRS = ((2, 0, 1), (3, 0, 2), (7, 0, 6), (7, 2, 4), (7, 3, 3), (12, 0, 11), (12, 1, 7), (16, 0, 15), (16, 4, 9))
# every instantiation of the kernels (N = 2 ... 16) with an end-to-end and an interior pair, then the further pairs of PAIRS; the
# residency of the tensor kernel steps at N = 8 / 9 and 12 / 13 (`times_min_waves`), that of the kernel that generates its draws
# drops to one wave at N = 14 (`times_philox_min_waves`)
SIZES = tuple(range(2, 17))
EVERY_SIZE = tuple(dict.fromkeys([(N, a, b) for N in SIZES for (a, b) in ((0, N - 1), (N // 2, max(N // 2 - 1, 0)))] + list(PAIRS)))
STEP_SIZES = (3, 7, 8, 9, 12, 13, 14, 16)     # both sides of each residency step, and the one-wave sizes
MIN_SPREAD = 0.05          # median over the samples of max_j F - min_j F on the reference: a kernel that ignores the grid fails


def times_of(T, tscale=None, tshift=None):
    """the definition of t_cj, independent of the code under test"""
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    M = max([len(v) for v in (tscale, tshift) if v is not None] + [1])
    a = np.ones(M) if tscale is None else np.asarray(tscale, dtype=np.float64)
    b = np.zeros(M) if tshift is None else np.asarray(tshift, dtype=np.float64)
    return np.abs(T[:, None] * a[None, :] + b[None, :])


def with_time(ctrl, t):
    """the controllers with their time entry replaced by t (a NaN row stays a NaN row)"""
    c = np.array(ctrl, dtype=np.float64)
    nan = np.isnan(c).any(axis=1)
    c[:, -1] = t
    c[nan] = np.nan
    return c


def _fma(a, b, c):
    """fma(a, b, c) correctly rounded (Fraction arithmetic is exact and its conversion to float rounds once); NaN passes through"""
    if a != a or b != b or c != c:
        return float("nan")
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def weighted_sum(weights, slabs):
    """the defined fma sequence over the slabs [M][...], element by element"""
    slabs = np.asarray(slabs, dtype=np.float64)
    w = [float(v) for v in weights]
    out = np.empty(slabs.shape[1:])
    flat, res = slabs.reshape(len(w), -1), out.reshape(-1)
    for i in range(flat.shape[1]):
        acc = w[0] * float(flat[0, i])
        for j in range(1, len(w)):
            acc = _fma(w[j], float(flat[j, i]), acc)
        res[i] = acc
    return out


def reference_slabs(ctrl, draws, N, a, b, tscale=None, tshift=None, h0_diag=None, h0_offdiag=None, fidelity=orc.fidelity_eigh):
    """[M][C][K] from one oracle evaluation per grid time (the line the kernel is built to beat)"""
    ctrl = np.asarray(ctrl, dtype=np.float64)
    draws = np.asarray(draws, dtype=np.float64)
    if draws.shape[0] == 1 and ctrl.shape[0] > 1:
        draws = np.broadcast_to(draws, (ctrl.shape[0],) + draws.shape[1:])
    t = times_of(ctrl[:, N], tscale, tshift)
    return np.stack([fidelity(with_time(ctrl, t[:, j]), draws, N, a, b, h0_diag=h0_diag, h0_offdiag=h0_offdiag)
                     for j in range(t.shape[1])])


# ------------------------------------------------------------------------------------------------------------------------
# the stand-in (and its broken variants)
# ------------------------------------------------------------------------------------------------------------------------


class StandIn:
    """`backend.mc_fidelity_times` / `readout_times` / `mc_fidelity` on the CPU oracle.  `broken`: one of BROKEN, a stand-in
    that gets exactly that part of the definition wrong."""

    BROKEN = ("ignores tscale", "ignores tshift", "no absolute value", "slabs reversed", "slab layout [C][K][M]",
              "unweighted wsum", "max instead of min", "NaN row not propagated")

    def __init__(self, broken=None):
        assert broken is None or broken in self.BROKEN
        self.broken = broken

    def readout_times(self, T, tscale=None, tshift=None):
        t = times_of(T, tscale, tshift)
        if self.broken == "no absolute value":
            T = np.asarray(T, dtype=np.float64).reshape(-1)
            a = 1.0 if tscale is None else np.asarray(tscale, dtype=np.float64)[None, :]
            b = 0.0 if tshift is None else np.asarray(tshift, dtype=np.float64)[None, :]
            t = np.broadcast_to(T[:, None] * a + b, t.shape)
        return t

    def mc_fidelity(self, controllers, draws, nspin, inspin, outspin, h0_diag=None, h0_offdiag=None, kernel="auto", **kw):
        c = np.asarray(controllers, dtype=np.float64)
        d = np.asarray(draws, dtype=np.float64)
        if d.shape[0] == 1 and c.shape[0] > 1:
            d = np.broadcast_to(d, (c.shape[0],) + d.shape[1:])
        return orc.fidelity_eigh(c, d, nspin, inspin, outspin, h0_diag=h0_diag, h0_offdiag=h0_offdiag)

    def mc_fidelity_times(self, controllers, draws, nspin, inspin, outspin, tscale=None, tshift=None, weights=None, want=("fid",),
                          h0_diag=None, h0_offdiag=None, device=None):
        ctrl = np.asarray(controllers, dtype=np.float64)
        if "wsum" in want and weights is None:
            raise ValueError("want 'wsum' needs weights")
        M = max([len(v) for v in (tscale, tshift, weights) if v is not None] + [1])
        sc = None if tscale is None or self.broken == "ignores tscale" else tscale
        sh = None if tshift is None or self.broken == "ignores tshift" else tshift
        sc = np.ones(M) if sc is None else sc
        sh = np.zeros(M) if sh is None else sh
        slabs = reference_slabs(ctrl, draws, nspin, inspin, outspin, sc, sh, h0_diag, h0_offdiag)
        res = {}
        if "wsum" in want:
            res["wsum"] = weighted_sum(np.ones(M) if self.broken == "unweighted wsum" else weights, slabs)
        if "min" in want:
            res["min"] = slabs.max(axis=0) if self.broken == "max instead of min" else slabs.min(axis=0)
        if self.broken == "NaN row not propagated":
            nan = np.isnan(ctrl).any(axis=1)
            for k in res:
                res[k][nan] = 0.0
        if "fid" in want:
            fid = slabs
            if self.broken == "slabs reversed":
                fid = slabs[::-1].copy()
            if self.broken == "slab layout [C][K][M]":
                fid = np.ascontiguousarray(np.moveaxis(slabs, 0, -1)).reshape(slabs.shape)
            res["fid"] = fid
        return res


def standin_times_philox(controllers, n_draws, nspin, inspin, outspin, seed, offset=0, sigma=0.05, tscale=None, tshift=None,
                         weights=None, want=("fid",), h0_diag=None, h0_offdiag=None):
    """`backend.mc_fidelity_times_philox` on the CPU: the documented stream elements (row c, draw k, site i, slot s is element
    offset + ((c K + k) N + i) 3 + s, scaled by the row's sigma) through the stand-in"""
    ctrl = np.asarray(controllers, dtype=np.float64)
    rows = ctrl.shape[0]
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (rows,))
    z = philox_host.philox_normal(seed, offset, rows * n_draws * nspin * 3, 1.0).reshape(rows, n_draws, nspin, 3)
    return StandIn().mc_fidelity_times(ctrl, sig[:, None, None, None] * z, nspin, inspin, outspin, tscale, tshift, weights, want,
                                       h0_diag, h0_offdiag)


# ------------------------------------------------------------------------------------------------------------------------
# checks (backend in, assertion out)
# ------------------------------------------------------------------------------------------------------------------------

_ORACLE_CACHE = {}


def oracle_workload(N, a, b):
    """the workload of the oracle comparison and its reference, computed once per (N, a, b) and never modified"""
    if (N, a, b) not in _ORACLE_CACHE:
        rng = np.random.default_rng(5)
        ctrl = cc.deloc_ctrl(rng, 3, N, 0.5)
        draws = 0.05 * rng.standard_normal((3, 70, N, 3))                # one full tile and a tail of 6
        want = reference_slabs(ctrl, draws, N, a, b, TSCALE, TSHIFT)
        for v in (ctrl, draws, want):
            v.setflags(write=False)
        _ORACLE_CACHE[N, a, b] = (ctrl, draws, want)
    return _ORACLE_CACHE[N, a, b]


def check_reference_guards(want, what):
    """the two guards of the oracle comparison: the reference has teeth, and it moves over the grid"""
    cc.assert_has_teeth(want, what=what)
    spread = float(np.median(want.max(axis=0) - want.min(axis=0)))
    assert spread >= MIN_SPREAD, ("the reference hardly changes over the grid", what, spread)
    return spread


def check_oracle(be, N, a, b, worst=None):
    ctrl, draws, want = oracle_workload(N, a, b)
    check_reference_guards(want, (N, a, b))
    got = be.mc_fidelity_times(ctrl, draws, N, a, b, tscale=TSCALE, tshift=TSHIFT, want=("fid",))["fid"]
    res = cc.compare(got, want, (N, a, b, "times vs oracle"))
    if worst is not None:
        worst.add("times", res)
    return res


def closed_form_workload(N):
    ctrl = cc.closed_form_ctrl(N, cc.CF_GS, [1.3])
    return ctrl, np.zeros((ctrl.shape[0], 2, N, 3)), cc.CF_TS - 1.3, cc.closed_form_offdiag(N)


def check_closed_form(be, N, worst=None):
    """the spin-j chain: no eigensolver in the reference.  One row per g, T = 1.3, the grid shifts it over CF_TS."""
    ctrl, draws, tshift, off = closed_form_workload(N)
    t = times_of(ctrl[:, N], None, tshift)
    lo, hi = 1.0, 0.0
    for out in (0, N // 2, N - 1):
        want = np.stack([np.repeat(cc.closed_form_fid(N, with_time(ctrl, t[:, j]), 0, out)[:, None], 2, axis=1)
                         for j in range(t.shape[1])])
        lo, hi = min(lo, float(want.min())), max(hi, float(want.max()))
        got = be.mc_fidelity_times(ctrl, draws, N, 0, out, tshift=tshift, h0_offdiag=off, want=("fid",))["fid"]
        res = cc.compare(got, want, (N, out, "times vs closed form"))
        if worst is not None:
            worst.add("closed form", res)
    assert lo < 1e-3 and hi > 0.9, (N, lo, hi)                            # the grid runs from ~0 to the full transfer


def check_readout_times(be):
    """`readout_times` is NumPy's |T a + b| bit for bit, negative arguments, absent arrays and NaN included"""
    T = np.array([3.7, -2.2, 0.0, 1e-3, 41.123456789, np.nan])
    a = np.array([1.0, 0.3, -1.7, 1.1, 0.0])
    b = np.array([0.0, -5.0, 0.25, 1e-9, -0.5])
    want = np.abs(T[:, None] * a[None, :] + b[None, :])
    assert (T[:, None] * a + b < 0).any()
    for (sa, sb, w) in ((a, b, want), (a, None, np.abs(T[:, None] * a)), (None, b, np.abs(T[:, None] + b)), (None, None, np.abs(T)[:, None])):
        got = np.asarray(be.readout_times(T, sa, sb))
        assert got.shape == w.shape and np.array_equal(got, w, equal_nan=True), (sa is None, sb is None)


def semantics_workload():
    """C = 3 (a NaN row in the middle), K = 5, M = 4; one grid time with T a + b < 0; weights that are not all equal"""
    rng = np.random.default_rng(11)
    N = 4
    ctrl = cc.deloc_ctrl(rng, 3, N, 0.5)
    ctrl[1, 2] = np.nan
    draws = 0.05 * rng.standard_normal((3, 5, N, 3))
    return N, ctrl, draws, np.array([1.0, 0.6, 1.4, -1.0]), np.array([0.0, 0.3, -0.4, -0.5]), np.array([0.4, 0.3, 0.2, -0.1])


def check_outputs(be, N, ctrl, draws, a, b, tscale, tshift, weights, h0_offdiag=None):
    """All three outputs of one call, and each alone: the slabs against the oracle, "wsum" and "min" against their definition
    evaluated on the backend's OWN slabs (exact), NaN rows everywhere."""
    want = reference_slabs(ctrl, draws, N, a, b, tscale, tshift, h0_offdiag=h0_offdiag)
    res = be.mc_fidelity_times(ctrl, draws, N, a, b, tscale=tscale, tshift=tshift, weights=weights, want=("fid", "wsum", "min"),
                               h0_offdiag=h0_offdiag)
    res = {k: np.asarray(v) for k, v in res.items()}
    assert sorted(res) == ["fid", "min", "wsum"]
    fid = res["fid"]
    cc.compare(fid, want, "slabs")
    nan = np.isnan(np.asarray(ctrl)).any(axis=1)
    assert res["min"].shape == want.shape[1:] and res["wsum"].shape == want.shape[1:]
    assert np.isnan(res["min"][nan]).all() and np.isnan(res["wsum"][nan]).all() and np.isnan(fid[:, nan]).all()
    assert not np.isnan(res["min"][~nan]).any() and not np.isnan(res["wsum"][~nan]).any()
    assert np.array_equal(res["min"], fid.min(axis=0), equal_nan=True), "min"
    assert np.array_equal(res["wsum"], weighted_sum(weights, fid), equal_nan=True), "wsum"
    # the order of the slabs and the weighting must matter on this workload, or the two lines above prove nothing
    ok = ~nan
    assert np.abs(fid[0][ok] - fid[-1][ok]).max() > 1e-2
    assert np.abs(res["wsum"][ok] - fid[:, ok].sum(axis=0)).max() > 1e-2 and np.abs(fid[:, ok].max(axis=0) - res["min"][ok]).max() > 1e-2
    for k in ("fid", "wsum", "min"):                                     # each output requested alone: the same bits
        one = be.mc_fidelity_times(ctrl, draws, N, a, b, tscale=tscale, tshift=tshift, weights=weights if k == "wsum" else None,
                                   want=(k,), h0_offdiag=h0_offdiag)
        assert list(one) == [k] and np.array_equal(np.asarray(one[k]), res[k], equal_nan=True), k
    return res


def check_semantics(be):
    N, ctrl, draws, tscale, tshift, weights = semantics_workload()
    check_readout_times(be)
    t = np.asarray(be.readout_times(ctrl[:, N], tscale, tshift))
    assert (ctrl[[0, 2], N][:, None] * tscale + tshift < 0).any()
    res = check_outputs(be, N, ctrl, draws, 0, N - 1, tscale, tshift, weights)
    # a grid time with T a + b < 0 equals the slab of a grid that asks for |t| directly (tscale = 0, tshift = t: per row)
    for c in (0, 2):
        direct = be.mc_fidelity_times(ctrl[c:c + 1], draws[c:c + 1], N, 0, N - 1, tscale=np.zeros(4), tshift=t[c], want=("fid",))["fid"]
        assert np.array_equal(np.asarray(direct)[:, 0], res["fid"][:, c]), c
    # absent arrays: all 1 / all 0
    one = be.mc_fidelity_times(ctrl, draws, N, 0, N - 1, tshift=tshift, want=("fid",))["fid"]
    two = be.mc_fidelity_times(ctrl, draws, N, 0, N - 1, tscale=np.ones(4), tshift=tshift, want=("fid",))["fid"]
    assert np.array_equal(np.asarray(one), np.asarray(two), equal_nan=True)
    one = be.mc_fidelity_times(ctrl, draws, N, 0, N - 1, tscale=tscale, want=("fid",))["fid"]
    two = be.mc_fidelity_times(ctrl, draws, N, 0, N - 1, tscale=tscale, tshift=np.zeros(4), want=("fid",))["fid"]
    assert np.array_equal(np.asarray(one), np.asarray(two), equal_nan=True)


def check_against_rows_kernel(be, N, a, b, exact=True):
    """slab j against `mc_fidelity(kernel="tridiag_ql")` on controllers with T replaced by `readout_times(...)`: the same
    operations, so the same bits"""
    ctrl, draws, _ = oracle_workload(N, a, b)
    t = np.asarray(be.readout_times(ctrl[:, N], TSCALE, TSHIFT))
    got = np.asarray(be.mc_fidelity_times(ctrl, draws, N, a, b, tscale=TSCALE, tshift=TSHIFT, want=("fid",))["fid"])
    worst = 0.0
    for j in range(len(TSCALE)):
        rows = np.asarray(be.mc_fidelity(with_time(ctrl, t[:, j]), draws, N, a, b, kernel="tridiag_ql"))
        worst = max(worst, float(np.abs(got[j] - rows).max()))
        if exact:
            assert np.array_equal(got[j], rows), (N, a, b, j, worst)
    return worst


def check_edges(be):
    """K = 64 and 65, M = 1 and M = 64, shared draws"""
    rng = np.random.default_rng(23)
    N = 5
    for K in (64, 65):
        ctrl = cc.deloc_ctrl(rng, 2, N, 0.5)
        draws = 0.05 * rng.standard_normal((2, K, N, 3))
        check_outputs(be, N, ctrl, draws, 0, N - 1, TSCALE, TSHIFT, np.array([0.1, 0.2, 0.4, 0.2, 0.1]))
    ctrl = cc.deloc_ctrl(rng, 2, N, 0.5)
    draws = 0.05 * rng.standard_normal((2, 9, N, 3))
    # M = 1: the grid is the row's own time - the plain fidelity, and wsum = w F, min = F
    res = be.mc_fidelity_times(ctrl, draws, N, 1, 3, weights=np.array([0.7]), want=("fid", "wsum", "min"))
    res = {k: np.asarray(v) for k, v in res.items()}
    cc.compare(res["fid"][0], orc.fidelity_eigh(ctrl, draws, N, 1, 3), "M = 1")
    assert res["fid"].shape == (1, 2, 9) and np.array_equal(res["min"], res["fid"][0]) and np.array_equal(res["wsum"], 0.7 * res["fid"][0])
    # M = 64: the largest grid
    tshift = np.linspace(-1.0, 1.0, 64)
    w64 = np.linspace(0.5, 1.5, 64) / 64
    got = be.mc_fidelity_times(ctrl, draws, N, 0, N - 1, tshift=tshift, weights=w64, want=("fid", "wsum", "min"))
    got = {k: np.asarray(v) for k, v in got.items()}
    cc.compare(got["fid"], reference_slabs(ctrl, draws, N, 0, N - 1, None, tshift), "M = 64")
    assert np.array_equal(got["min"], got["fid"].min(axis=0)) and np.array_equal(got["wsum"], weighted_sum(w64, got["fid"]))
    # one draw set for every controller
    shared = 0.05 * rng.standard_normal((1, 65, N, 3))
    c3 = cc.deloc_ctrl(rng, 3, N, 0.5)
    got = np.asarray(be.mc_fidelity_times(c3, shared, N, 0, N - 1, tscale=TSCALE, tshift=TSHIFT, want=("fid",))["fid"])
    want = reference_slabs(c3, shared, N, 0, N - 1, TSCALE, TSHIFT)
    cc.assert_has_teeth(want, what="shared draws")
    cc.compare(got, want, "shared draws")


# ------------------------------------------------------------------------------------------------------------------------
# a toy experiment for `MCDataSim.get_readout_dict`
# ------------------------------------------------------------------------------------------------------------------------
TOY = dict(N=4, A=0, B=3, C=4, TN=0.05, SEED=77, K=16, NOISES=np.array([0.02, 0.05]),
           TSCALE=np.array([0.7, 1.0, 1.3]), TSHIFT=np.array([0.1, 0.0, -0.2]))


def write_toy_experiment(name):
    """two algorithms with three delocalised controller rows each under ./experiments/<name> (the fourth slot stays empty);
    returns the controller table"""
    import json
    import os
    N, rng = TOY["N"], np.random.default_rng(3)

    def rows(n):
        x = np.empty((n, N + 1))
        x[:, :N] = rng.uniform(-0.5, 0.5, (n, N))
        x[:, N] = rng.uniform(0.5 * N, 0.7 * N, n)
        return x.tolist()
    le = {"ppo": {str(TOY["TN"]): {"controller": rows(3)}}, "lbfgs": {str(N): {"controller": rows(3)}}}
    os.makedirs(f"experiments/{name}")
    with open(f"experiments/{name}/ppo_spin_{N}_{TOY['A']}-{TOY['B']}_c_{TOY['C']}.le", "w") as fh:
        json.dump(le, fh)
    return le


def readout_level_reference(ctrl, j, sigma, nvalid, samples, seed, tscale, tshift):
    """level j of an algorithm on its own (its elements start at j * nvalid * K * 3 N): (rim [M][C'], std, worst, window_rim [C'])"""
    N = TOY["N"]
    off = j * nvalid * samples * N * 3
    draws = sigma * philox_host.philox_normal(seed, off, nvalid * samples * N * 3, 1.0).reshape(nvalid, samples, N, 3)
    slabs = reference_slabs(ctrl, draws, N, TOY["A"], TOY["B"], tscale, tshift)
    rim = np.array([[orc.wd_from_ideal(r.copy()) for r in s] for s in slabs])
    window = np.array([orc.wd_from_ideal(r.copy()) for r in slabs.min(axis=0)])
    return rim, slabs.std(axis=2), slabs.min(axis=2), window
