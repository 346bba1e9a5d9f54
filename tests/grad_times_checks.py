"""Checks of the fidelity gradient on a grid of readout times (`backend.mc_fidelity_grad_times_philox`), the references they are
held to, and a NumPy stand-in of the entry.  The `check_*` functions take a backend object: tests/test_gpu_grad_times.py runs
them on the device, tests/test_grad_times_checks.py on the stand-in, where they must pass, and on broken stand-ins, where they
must fail.

Definition under test.  Controller row c, time entry T_c (signed), grid (tscale, tshift, w) of M times:
    u_cj = T_c tscale_j + tshift_j                     (product rounded, then the sum: NumPy's own)
    W = sum_j w_j F(u_cj),   dW/dx_l = sum_j w_j dF/dx_l(u_cj),   dW/dx_N = sum_j w_j tscale_j sgn(u_cj) F'(|u_cj|),
every sum taken as acc = w_0 v_0; acc = fma(w_j, v_j, acc); "mean" / "moment" the row means of (W, dW/dx) and (W^2, W dW/dx).

References.  Independent: `grad_checks.grad_eigh` at each grid time on `times_checks.with_time(ctrl, u_j)` (its time entry
carries sgn(u_j)), the time entry multiplied by tscale_j, combined in float64.  Bound: sum_j |w_j| grad_bars(row at time u_j),
the time entry's bar multiplied by |tscale_j| - every term's own bar, weighted like the term.  Bit for bit: M calls of the
backend's own `mc_fidelity_grad_philox` on the same rows, combined by `times_checks.weighted_sum` (exact fma)."""
import numpy as np

import chain_checks as cc
import grad_checks as gc
import times_checks as tc

TSCALE, TSHIFT = tc.TSCALE, tc.TSHIFT
WEIGHTS = np.array([0.1, 0.2, 0.4, 0.2, 0.1])
SEED, SIGMA = gc.PHILOX_SEED, gc.PHILOX_SIGMA
EPS = 2.0 ** -52
OUTPUTS = ("fid", "grad", "mean", "moment")
# every instantiation: 2 ... 9 single pass (7 the residency edge); 10: the first multi-pass size; 11: the only size with five
# eigenvector rows per QL pass in three passes (`grad_batch_rows`, `grad_passes`); 12: the most passes
SIZES = tuple(range(2, 13))
MIN_BIAS_TEETH, MIN_TIME_TEETH = 0.01, 0.1


def pairs(N):
    """end to end, one interior pair, one with in == out"""
    return tuple(dict.fromkeys(((0, N - 1), (min(1, N - 1), N // 2), (N // 2, N // 2))))


def signed_times(T, tscale=None, tshift=None):
    """u_cj [C][M], the definition (NumPy rounds the product, then the sum)"""
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    M = max([len(v) for v in (tscale, tshift) if v is not None] + [1])
    a = np.ones(M) if tscale is None else np.asarray(tscale, dtype=np.float64)
    b = np.zeros(M) if tshift is None else np.asarray(tshift, dtype=np.float64)
    return T[:, None] * a[None, :] + b[None, :]


def grid_of(tscale, tshift, weights):
    M = len(weights)
    return (np.ones(M) if tscale is None else np.asarray(tscale, dtype=np.float64),
            np.zeros(M) if tshift is None else np.asarray(tshift, dtype=np.float64), np.asarray(weights, dtype=np.float64))


def draws_of(ctrl, K, N, offset=0, shared=False, sigma=SIGMA):
    """the draws the entry generates, regenerated on the host: [C][K][N][3]"""
    C = ctrl.shape[0]
    if shared:
        z = gc.host_draws(SEED, offset, (1, K, N, 3), 1.0)
        return z * np.broadcast_to(np.asarray(sigma, dtype=np.float64), (C,))[:, None, None, None]
    return gc.host_draws(SEED, offset, (C, K, N, 3), sigma)


def reference(ctrl, draws, N, a, b, tscale, tshift, weights, h0_diag=None, h0_offdiag=None):
    """(W [C][K], dW [C][K][N+1], bars [C][K][N+1], F at the row's own T, dF at the row's own T) from grad_eigh per grid time"""
    ctrl = np.asarray(ctrl, dtype=np.float64)
    sc, sh, w = grid_of(tscale, tshift, weights)
    u = signed_times(ctrl[:, N], sc, sh)
    W = G = bars = None
    for j in range(len(w)):
        cj = tc.with_time(ctrl, u[:, j])
        Fj, Gj = gc.grad_eigh(cj, draws, N, a, b, h0_diag, h0_offdiag)
        bj = gc.grad_bars(cj, draws, N, h0_diag, h0_offdiag)
        Gj[..., N] *= sc[j]
        bj[..., N] *= abs(sc[j])
        W = w[j] * Fj if W is None else W + w[j] * Fj
        G = w[j] * Gj if G is None else G + w[j] * Gj
        bars = abs(w[j]) * bj if bars is None else bars + abs(w[j]) * bj
    F0, G0 = gc.grad_eigh(ctrl, draws, N, a, b, h0_diag, h0_offdiag)
    return W, G, bars, F0, G0


def teeth(G, G0, weights):
    """(bias, time): the medians over the samples of max_l |dW/dx_l - (sum w) dF/dx_l(T)| over the biases, and of the same
    difference of the time entry - what a kernel that ignores the grid gets wrong"""
    ok = ~np.isnan(G).any(axis=(-1, -2))
    d = np.abs(G[ok] - float(np.sum(weights)) * G0[ok])
    return float(np.median(d[..., :-1].max(axis=-1))), float(np.median(d[..., -1]))


def assert_teeth(G, G0, weights, what):
    tb, tt = teeth(G, G0, weights)
    assert tb >= MIN_BIAS_TEETH and tt >= MIN_TIME_TEETH, ("the reference hardly feels the grid", what, tb, tt)
    return tb, tt


def host_means(res):
    return np.concatenate([res["fid"].mean(axis=1)[:, None], res["grad"].mean(axis=1)], axis=1)


def host_moments(res):
    return np.concatenate([(res["fid"] ** 2).mean(axis=1)[:, None], (res["fid"][..., None] * res["grad"]).mean(axis=1)], axis=1)


# ------------------------------------------------------------------------------------------------------------------------
# the stand-in (and its broken variants)
# ------------------------------------------------------------------------------------------------------------------------


class StandIn(gc.StandIn):
    """`backend.mc_fidelity_grad_times_philox` (and, inherited, `mc_fidelity_grad_philox`) on the CPU: the single-time stand-in
    per grid time, combined by the defined fma sequence.  `broken`: one of BROKEN."""

    BROKEN = ("grid ignored", "omega dropped from the gradient", "no tscale in the time entry", "no sgn(u)",
              "moments with F(T)", "W summed over the passes")

    def __init__(self, broken=None):
        assert broken is None or broken in self.BROKEN
        gc.StandIn.__init__(self, None)
        self.times_broken = broken
        self.calls = []

    def mc_fidelity_times_philox(self, ctrl, K, N, a, b, seed, offset=0, sigma=0.05, tscale=None, tshift=None, weights=None,
                                 want=("fid",), h0_diag=None, h0_offdiag=None):
        return tc.standin_times_philox(ctrl, K, N, a, b, seed, offset, sigma, tscale, tshift, weights, want, h0_diag, h0_offdiag)

    def readout_times(self, T, tscale=None, tshift=None):
        return tc.times_of(T, tscale, tshift)

    def mc_fidelity_grad_times_philox(self, ctrl, K, N, a, b, seed, offset=0, sigma=0.05, shared=False, tscale=None, tshift=None,
                                      weights=None, h0_diag=None, h0_offdiag=None, want=OUTPUTS):
        if weights is None:
            raise ValueError("weights: required")
        self.calls.append(dict(tscale=tscale, tshift=tshift, weights=weights, K=K, seed=seed, offset=offset, sigma=sigma,
                               shared=shared, want=tuple(want)))
        br = self.times_broken
        ctrl = np.asarray(ctrl, dtype=np.float64)
        sc, sh, w = grid_of(tscale, tshift, weights)
        if br == "grid ignored":
            sc, sh = np.ones(len(w)), np.zeros(len(w))
        u = signed_times(ctrl[:, N], sc, sh)
        Fs, Gs = [], []
        for j in range(len(w)):
            r = self.mc_fidelity_grad_philox(tc.with_time(ctrl, u[:, j]), K, N, a, b, seed, offset=offset, sigma=sigma, shared=shared,
                                             h0_diag=h0_diag, h0_offdiag=h0_offdiag, want=("fid", "grad"))
            g = np.array(r["grad"])
            if br == "no sgn(u)":
                g[..., N] *= np.where(u[:, j] < 0, -1.0, 1.0)[:, None]
            if br != "no tscale in the time entry":
                g[..., N] = sc[j] * g[..., N]
            Fs.append(r["fid"])
            Gs.append(g)
        W = tc.weighted_sum(w, np.stack(Fs))
        G = tc.weighted_sum(np.ones(len(w)) if br == "omega dropped from the gradient" else w, np.stack(Gs))
        Wm = W
        if br == "moments with F(T)":
            Wm = self.mc_fidelity_grad_philox(ctrl, K, N, a, b, seed, offset=offset, sigma=sigma, shared=shared, h0_diag=h0_diag,
                                              h0_offdiag=h0_offdiag, want=("fid",))["fid"]
        if br == "W summed over the passes":
            W = W * (1 if N <= 9 else {10: 2, 11: 3, 12: 5}[N])
        full = {"fid": W, "grad": G}
        res = {k: full[k] for k in ("fid", "grad") if k in want}
        if "mean" in want:
            res["mean"] = host_means(full) if K else np.zeros((ctrl.shape[0], N + 2))
        if "moment" in want:
            res["moment"] = host_moments({"fid": Wm, "grad": G}) if K else np.zeros((ctrl.shape[0], N + 2))
        return res


# ------------------------------------------------------------------------------------------------------------------------
# checks (backend in, assertion out)
# ------------------------------------------------------------------------------------------------------------------------


def _call(be, ctrl, K, N, a, b, offset=0, shared=False, sigma=SIGMA, tscale=TSCALE, tshift=TSHIFT, weights=WEIGHTS, want=OUTPUTS,
          h0d=None, h0o=None):
    return gc.to_host(be.mc_fidelity_grad_times_philox(ctrl, K, N, a, b, SEED, offset=offset, sigma=sigma, shared=shared, tscale=tscale,
                                                       tshift=tshift, weights=weights, h0_diag=h0d, h0_offdiag=h0o, want=want))


def single_time_yardstick(be, ctrl, K, N, a, b, offset=0, shared=False, sigma=SIGMA, tscale=TSCALE, tshift=TSHIFT, weights=WEIGHTS):
    """M calls of the backend's `mc_fidelity_grad_philox` on with_time(ctrl, u_j), the time column multiplied by tscale_j (rounded
    once), the slabs combined by the exact fma sequence: {"fid", "grad"}"""
    sc, sh, w = grid_of(tscale, tshift, weights)
    u = signed_times(ctrl[:, N], sc, sh)
    Fs, Gs = [], []
    for j in range(len(w)):
        r = gc.to_host(be.mc_fidelity_grad_philox(tc.with_time(ctrl, u[:, j]), K, N, a, b, SEED, offset=offset, sigma=sigma, shared=shared,
                                                  want=("fid", "grad")))
        g = np.array(r["grad"])
        g[..., N] = sc[j] * g[..., N]
        Fs.append(r["fid"])
        Gs.append(g)
    return {"fid": tc.weighted_sum(w, np.stack(Fs)), "grad": tc.weighted_sum(w, np.stack(Gs))}


def check_bits_against_single_time(be, N, a, b, K=70, offset=0, shared=False, sigma=SIGMA, exact=True, ctrl=None, grid=None):
    """check 1: fid and grad equal the yardstick bit for bit (`exact`), else inside the bars of the independent reference"""
    ctrl = gc.philox_ctrl(N) if ctrl is None else ctrl
    tscale, tshift, weights = grid if grid is not None else (TSCALE, TSHIFT, WEIGHTS)
    what = ("bits", N, a, b, K, offset, "shared" if shared else "per row")
    got = _call(be, ctrl, K, N, a, b, offset, shared, sigma, tscale, tshift, weights, want=("fid", "grad"))
    want = single_time_yardstick(be, ctrl, K, N, a, b, offset, shared, sigma, tscale, tshift, weights)
    nan = np.isnan(ctrl).any(axis=1)
    assert np.isnan(got["fid"][nan]).all() and np.isnan(got["grad"][nan]).all() and np.isfinite(got["grad"][~nan]).all(), what
    assert np.abs(want["grad"][~nan]).max() > 1e-2, what
    if exact:
        gc.assert_same_bits(got, want, what, ("fid", "grad"))
    else:
        draws = draws_of(ctrl, K, N, offset, shared, sigma)
        bars = reference(ctrl, draws, N, a, b, tscale, tshift, weights)[2]
        gc.compare_grad(got["grad"], want["grad"], 2.0 * bars, what)
    return got


def check_unit_grid(be, N, a, b, K=70, shared=False):
    """check 2: M = 1, tscale = 1, tshift = 0, w = 1: all four outputs are `mc_fidelity_grad_philox`'s bits"""
    ctrl = gc.philox_ctrl(N)
    want = gc.to_host(be.mc_fidelity_grad_philox(ctrl, K, N, a, b, SEED, offset=3, sigma=SIGMA, shared=shared))
    for (sc, sh) in ((np.ones(1), np.zeros(1)), (None, None)):
        got = _call(be, ctrl, K, N, a, b, 3, shared, SIGMA, sc, sh, np.ones(1))
        gc.assert_same_bits(got, want, ("unit grid", N, a, b, shared, sc is None), OUTPUTS)
    assert np.abs(want["moment"][[0, 2]]).max() > 1e-3


def check_means_and_moments(be, N, a, b, K=70, shared=False):
    """check 3: mean and moment against float64 NumPy means of the per-sample outputs of the same call, K 2^-52 max|entry| per
    row (the summation order only); NaN row NaN everywhere; each output alone gives the same bits"""
    ctrl = gc.philox_ctrl(N)
    full = _call(be, ctrl, K, N, a, b, 7, shared)
    assert all(np.isnan(full[k][1]).all() for k in OUTPUTS), (N, a, b)
    ok = [0, 2]
    hm, hq = host_means(full), host_moments(full)
    for c in ok:
        bm = K * EPS * max(float(np.abs(full["grad"][c]).max()), float(np.abs(full["fid"][c]).max()))
        bq = K * EPS * float(np.abs(np.concatenate([full["fid"][c][:, None] ** 2, full["fid"][c][:, None] * full["grad"][c]], axis=1)).max())
        em, eq = float(np.abs(full["mean"][c] - hm[c]).max()), float(np.abs(full["moment"][c] - hq[c]).max())
        assert em <= bm, ("mean against host sums", N, a, b, c, em, bm)
        assert eq <= bq, ("moment against host sums", N, a, b, c, eq, bq)
    # the moments must differ from what F W would give (mean W^2 != (mean W)^2 is not enough: that holds for any spread)
    assert np.abs(hq[ok, 1:]).max() > 1e-3 and hq[ok, 0].min() > 1e-3
    for sub in (("mean",), ("moment",), ("mean", "moment"), ("fid",)):
        only = _call(be, ctrl, K, N, a, b, 7, shared, want=sub)
        assert set(only) == set(sub)
        gc.assert_same_bits(only, full, ("subset", N, sub), sub)
    return full


def guarded_ctrl(N, a, b):
    """the controllers on which the teeth guards were measured: those of the oracle workload of times_checks.py ((N, a, b) one of
    times_checks.PAIRS, N <= 12), under N(0, 0.05^2) draws"""
    assert (N, a, b) in tc.PAIRS and N <= 12
    return np.array(tc.oracle_workload(N, a, b)[0])


def check_reference(be, N, a, b, K=70, shared=False, worst=None, guard=True, ctrl=None):
    """check 4: inside the bars of grad_eigh per grid time; `guard`: with the teeth guards asserted on the reference (they hold on
    the controllers of `guarded_ctrl`)"""
    ctrl = gc.philox_ctrl(N) if ctrl is None else ctrl
    draws = draws_of(ctrl, K, N, 0, shared)
    W, G, bars, F0, G0 = reference(ctrl, draws, N, a, b, TSCALE, TSHIFT, WEIGHTS)
    what = ("reference", N, a, b, "shared" if shared else "per row")
    if guard:
        assert_teeth(G, G0, WEIGHTS, what)
    got = _call(be, ctrl, K, N, a, b, 0, shared)
    cc.compare(got["fid"], W, (what, "fid"))
    out = gc.compare_grad(got["grad"], G, bars, (what, "grad"))
    mw = np.concatenate([W.mean(axis=1)[:, None], G.mean(axis=1)], axis=1)
    mb = np.concatenate([np.full((bars.shape[0], 1), gc.TOL), bars.max(axis=1)], axis=1)
    gc.compare_grad(got["mean"], mw, mb, (what, "mean"))
    # moment: |W| <= sum |w| and |err W| <= TOL, so |err (W dW)| <= sum|w| bars + TOL |dW|
    sw = float(np.abs(WEIGHTS).sum())
    qw = np.concatenate([(W * W).mean(axis=1)[:, None], (W[..., None] * G).mean(axis=1)], axis=1)
    qb = np.concatenate([np.full((bars.shape[0], 1), 2 * sw * gc.TOL), (sw * bars + gc.TOL * np.abs(np.nan_to_num(G))).max(axis=1)], axis=1)
    gc.compare_grad(got["moment"], qw, qb, (what, "moment"))
    if worst is not None:
        worst.add(("times", N), out)
    return out


def cross_bound(ctrl, draws, N, tscale, tshift, weights):
    """sum |w| 64 N 2^-52 max(1, t ||H||) per sample: the project's bound between two fp64 eigen routes, at the largest grid time"""
    cz = np.nan_to_num(np.asarray(ctrl, dtype=np.float64))
    d = cz[:, None, :N] + draws[..., 0]
    e = np.hypot(1.0 + draws[:, :, 1:, 1], draws[:, :, 1:, 2])
    norm = np.abs(d).max(-1) + 2.0 * e.max(-1)
    t = np.abs(signed_times(cz[:, N], tscale, tshift)).max(axis=1)
    return float(np.abs(weights).sum()) * 64 * N * EPS * np.maximum(1.0, t[:, None] * norm)


def check_cross_times_kernel(be, N, a, b, K=70):
    """check 5: W against the weighted sum of the readout-time kernel (another kernel, another eigen route)"""
    ctrl = gc.philox_ctrl(N)
    got = _call(be, ctrl, K, N, a, b, 0, False, want=("fid",))["fid"]
    ws = gc.to_host(be.mc_fidelity_times_philox(ctrl, K, N, a, b, SEED, offset=0, sigma=SIGMA, tscale=TSCALE, tshift=TSHIFT,
                                                weights=WEIGHTS, want=("wsum",)))["wsum"]
    bound = cross_bound(ctrl, draws_of(ctrl, K, N), N, TSCALE, TSHIFT, WEIGHTS)
    ok = [0, 2]
    assert np.isnan(got[1]).all() and np.isnan(ws[1]).all()
    err = np.abs(got[ok] - ws[ok])
    assert (err <= bound[ok]).all(), ("W against the times kernel", N, a, b, float(err.max()), float(bound[ok].min()))
    assert np.ptp(ws[ok]) > 1e-3
    return float(err.max())


def check_semantics(be, N=7, K=70):
    """check 6: every u < 0 (tshift = -2 |T|: F is even, so W is that of the mirrored grid and the time entry that of
    tscale -> -tscale); u = 0 exactly; M = 64"""
    ctrl = gc.philox_ctrl(N, nan_row=None, neg_row=None)[:1]
    a, b, T = 0, N - 1, float(ctrl[0, N])
    assert T > 0
    # u_j = T - 2 T = -T against u_j = T: the same W and bias entries, the time entry with the sign of tscale flipped
    neg = _call(be, ctrl, K, N, a, b, 0, False, SIGMA, np.ones(1), np.array([-2.0 * T]), np.ones(1), want=("fid", "grad"))
    pos = _call(be, ctrl, K, N, a, b, 0, False, SIGMA, -np.ones(1), np.array([2.0 * T]), np.ones(1), want=("fid", "grad"))
    own = gc.to_host(be.mc_fidelity_grad_philox(ctrl, K, N, a, b, SEED, sigma=SIGMA, want=("fid", "grad")))
    assert np.array_equal(neg["fid"], own["fid"]) and np.array_equal(pos["fid"], own["fid"])
    assert np.array_equal(neg["grad"][..., :N], own["grad"][..., :N]) and np.array_equal(pos["grad"][..., :N], own["grad"][..., :N])
    assert np.array_equal(neg["grad"][..., N], -own["grad"][..., N]) and np.array_equal(pos["grad"][..., N], -own["grad"][..., N])
    assert np.abs(own["grad"][..., N]).max() > 1e-2
    # u = 0 exactly: F = [in == out] (to the orthonormality of the rows: the fidelity bar), every derivative exactly 0
    for (ai, bi) in ((0, N - 1), (N // 2, N // 2)):
        z = _call(be, ctrl, K, N, ai, bi, 0, False, SIGMA, np.zeros(1), np.zeros(1), np.array([0.7]), want=("fid", "grad"))
        assert np.abs(z["fid"] - 0.7 * (ai == bi)).max() < gc.TOL, (ai, bi)
        assert (z["grad"] == 0.0).all(), (ai, bi)
    # M = 64 against the single-time yardstick
    grid = (np.linspace(0.7, 1.3, 64), np.linspace(-1.0, 1.0, 64), np.linspace(0.5, 1.5, 64) / 64)
    return check_bits_against_single_time(be, N, a, b, K=K, ctrl=ctrl, grid=grid)


def check_hard_inputs(be, N):
    """the controller rows of `grad_checks.hard_inputs` (uniform, mirror-symmetric, clustered, T = 0, biases of 1e3; the cut bond as
    a zero static coupling) on the grid, without draws (sigma = 0) and with them: finite, inside the bars of the reference"""
    rng = np.random.default_rng(7700 + N)
    K = 3
    for name, ctrl, _ in gc.hard_inputs(N, rng):
        h0o = None
        if name == "cut":
            h0o = np.ones(N - 1)
            h0o[max(1, N // 2) - 1] = 0.0
        for sigma in (0.0, SIGMA):
            for (a, b) in pairs(N):
                what = ("hard", name, N, a, b, sigma)
                draws = draws_of(ctrl, K, N, 0, False, sigma)
                W, G, bars, _, _ = reference(ctrl, draws, N, a, b, TSCALE, TSHIFT, WEIGHTS, None, h0o)
                got = _call(be, ctrl, K, N, a, b, 0, False, sigma, want=("fid", "grad"), h0o=h0o)
                assert np.isfinite(got["fid"]).all() and np.isfinite(got["grad"]).all(), what
                assert np.abs(got["fid"] - W).max() < gc.TOL * float(np.abs(WEIGHTS).sum()), what
                gc.compare_grad(got["grad"], G, bars, what)
