"""The argument tuples `backend.py` hands to the C entries of include/robchar_hip.h, pinned on the NumPy (blocking) path with a
recording stand-in for the loaded library - runs without a GPU and without a built library.  The expected tuples are written
out from the prototypes in the header, argument by argument; nothing here is derived from backend.py."""
import ctypes
import importlib

import numpy as np
import pytest

N, C, K, M = 3, 2, 3, 2
TAIL_LEN, FUSED_PAYS = 2, 1


class Recorder:
    """Stands in for the loaded library: every `rc_*` attribute records (name, args) and returns 0.  `peek[(name, i)] = n` keeps
    the n doubles behind pointer argument i as they are DURING the call (for arrays the wrapper makes and drops)."""

    def __init__(self):
        self.calls, self.peek, self.peeked = [], {}, {}

    def __getattr__(self, name):
        if not name.startswith("rc_"):
            raise AttributeError(name)
        fixed = {"rc_device_count": 1, "rc_last_error": b"", "rc_tail_select_len": TAIL_LEN, "rc_philox_fused_pays": FUSED_PAYS}
        if name in fixed:
            return lambda *args: fixed[name]

        def entry(*args):
            self.calls.append((name, args))
            for (which, i), n in self.peek.items():
                if which == name:
                    self.peeked[(name, i)] = list(ctypes.cast(args[i], ctypes.POINTER(ctypes.c_double))[:n])
            return 0
        return entry


@pytest.fixture
def rec(monkeypatch):
    lib = importlib.import_module("code-robchar_amd._lib")
    r = Recorder()
    monkeypatch.setattr(lib, "load", lambda: r)
    return r


@pytest.fixture
def backend():
    return importlib.import_module("code-robchar_amd.backend")


def P(a):
    """What a pointer to the first element of the NumPy array `a` looks like after `seen`."""
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return ("ptr", a.ctypes.data)


def seen(rec, name):
    """The arguments of the ONE recorded call, which must be to `name`: pointers as ("ptr", address), NULL as None."""
    assert [c[0] for c in rec.calls] == [name], rec.calls
    return tuple(("ptr", a.value) if isinstance(a, ctypes.c_void_p) else a for a in rec.calls[0][1])


def out_ptr(res, key, shape):
    assert isinstance(res[key], np.ndarray) and res[key].shape == shape and res[key].dtype == np.float64
    return P(res[key])


def inputs(h0=False):
    rng = np.random.RandomState(3)
    ctrl, draws = rng.rand(C, N + 1), rng.rand(C, K, N, 3)
    return ctrl, draws, (rng.rand(N) if h0 else None), (rng.rand(N - 1) if h0 else None)


# ---------------------------------------------------------------------------------------------------------------- the calls
# int rc_mc_fidelity_kernel_f64(device, kernel, N, in, out, h0_diag, h0_offdiag, ring, controllers, draws, C, K, fid_out)
def test_mc_fidelity(rec, backend):
    ctrl, draws, h0d, h0o = inputs(h0=True)
    res = backend.mc_fidelity(ctrl, draws, N, 0, 2, h0_diag=h0d, h0_offdiag=h0o, ring=True, device=0, kernel="tridiag_ql")
    assert isinstance(res, np.ndarray) and res.shape == (C, K) and res.dtype == np.float64
    assert seen(rec, "rc_mc_fidelity_kernel_f64") == (0, 1, N, 0, 2, P(h0d), P(h0o), 1, P(ctrl), P(draws), C, K, P(res))


def test_mc_fidelity_without_static_terms_into_out(rec, backend):
    ctrl, draws, _, _ = inputs()
    out = np.empty((C, K))
    res = backend.mc_fidelity(ctrl, draws, N, 1, 0, out=out)
    assert res is out
    assert seen(rec, "rc_mc_fidelity_kernel_f64") == (0, 0, N, 1, 0, None, None, 0, P(ctrl), P(draws), C, K, P(out))


# int rc_mc_fidelity_grad_f64(device, N, in, out, h0_diag, h0_offdiag, controllers, draws, draws_ctrl_stride, C, K,
#                             fid_out, grad_out, mean_out);   rc_mc_fidelity_sens_f64: the same, sens_out for grad_out
@pytest.mark.parametrize("which, second, second_shape, mean_len", [("grad", "grad", (C, K, N + 1), N + 2),
                                                                   ("sens", "sens", (C, K, N, 3), 3 * N + 2)])
def test_derivatives(rec, backend, which, second, second_shape, mean_len):
    fn = getattr(backend, f"mc_fidelity_{which}")
    ctrl, draws, h0d, h0o = inputs(h0=True)
    res = fn(ctrl, draws, N, 0, 2, h0_diag=h0d, h0_offdiag=h0o, device=0)
    assert sorted(res) == sorted(("fid", second, "mean"))
    assert seen(rec, f"rc_mc_fidelity_{which}_f64") == (
        0, N, 0, 2, P(h0d), P(h0o), P(ctrl), P(draws), K * N * 3, C, K,
        out_ptr(res, "fid", (C, K)), out_ptr(res, second, second_shape), out_ptr(res, "mean", (C, mean_len)))


@pytest.mark.parametrize("which, second, second_shape, mean_len", [("grad", "grad", (C, K, N + 1), N + 2),
                                                                   ("sens", "sens", (C, K, N, 3), 3 * N + 2)])
def test_derivatives_one_output(rec, backend, which, second, second_shape, mean_len):
    fn = getattr(backend, f"mc_fidelity_{which}")
    ctrl, draws, _, _ = inputs()
    res = fn(ctrl, draws, N, 2, 1, want=("mean",))
    assert list(res) == ["mean"]
    assert seen(rec, f"rc_mc_fidelity_{which}_f64") == (
        0, N, 2, 1, None, None, P(ctrl), P(draws), K * N * 3, C, K, None, None, out_ptr(res, "mean", (C, mean_len)))
    rec.calls.clear()
    res = fn(ctrl, draws, N, 2, 1, want=(second,))
    assert seen(rec, f"rc_mc_fidelity_{which}_f64") == (
        0, N, 2, 1, None, None, P(ctrl), P(draws), K * N * 3, C, K, None, out_ptr(res, second, second_shape), None)


@pytest.mark.parametrize("which", ["grad", "sens"])
def test_derivatives_shared_draw_set(rec, backend, which):
    """one (1, K, N, 3) draw set for both controllers: stride 0, on the blocking entry"""
    ctrl, draws, _, _ = inputs()
    one = np.ascontiguousarray(draws[:1])
    res = getattr(backend, f"mc_fidelity_{which}")(ctrl, one, N, 0, 2, want=("fid",))
    assert seen(rec, f"rc_mc_fidelity_{which}_f64") == (
        0, N, 0, 2, None, None, P(ctrl), P(one), 0, C, K, out_ptr(res, "fid", (C, K)), None, None)


# int rc_mc_fidelity_times_f64(device, N, in, out, h0_diag, h0_offdiag, ring, controllers, draws, draws_ctrl_stride, C, K, M,
#                              tscale, tshift, weights, fid_out, wsum_out, fmin_out)
def test_times(rec, backend):
    ctrl, draws, h0d, h0o = inputs(h0=True)
    a, b, w = np.array([1.0, 0.5]), np.array([0.0, 0.25]), np.array([0.75, 0.25])
    res = backend.mc_fidelity_times(ctrl, draws, N, 0, 2, tscale=a, tshift=b, weights=w, want=("fid", "wsum", "min"),
                                    h0_diag=h0d, h0_offdiag=h0o, device=0)
    assert sorted(res) == ["fid", "min", "wsum"]
    assert seen(rec, "rc_mc_fidelity_times_f64") == (
        0, N, 0, 2, P(h0d), P(h0o), 0, P(ctrl), P(draws), K * N * 3, C, K, M, P(a), P(b), P(w),
        out_ptr(res, "fid", (M, C, K)), out_ptr(res, "wsum", (C, K)), out_ptr(res, "min", (C, K)))


def test_times_without_weights_one_output(rec, backend):
    ctrl, draws, _, _ = inputs()
    b = np.array([0.0, 0.25])
    rec.peek[("rc_mc_fidelity_times_f64", 13)] = M          # the absent tscale: all 1, made inside the call
    res = backend.mc_fidelity_times(ctrl, draws, N, 1, 1, tshift=b, want=("min",))
    assert list(res) == ["min"]
    got = seen(rec, "rc_mc_fidelity_times_f64")
    assert got[:13] == (0, N, 1, 1, None, None, 0, P(ctrl), P(draws), K * N * 3, C, K, M)
    assert rec.peeked[("rc_mc_fidelity_times_f64", 13)] == [1.0, 1.0]
    assert got[14:] == (P(b), None, None, None, out_ptr(res, "min", (C, K)))
    rec.calls.clear()
    rec.peek = {("rc_mc_fidelity_times_f64", 13): 1, ("rc_mc_fidelity_times_f64", 14): 1}
    res = backend.mc_fidelity_times(ctrl, draws, N, 1, 1)       # no grid at all: M = 1, t = |T|, want = ("fid",)
    got = seen(rec, "rc_mc_fidelity_times_f64")
    assert got[:13] == (0, N, 1, 1, None, None, 0, P(ctrl), P(draws), K * N * 3, C, K, 1)
    assert rec.peeked == {("rc_mc_fidelity_times_f64", 13): [1.0], ("rc_mc_fidelity_times_f64", 14): [0.0]}
    assert got[15:] == (None, out_ptr(res, "fid", (1, C, K)), None, None)


# int rc_reduce_f64(device, fid, C, K, q_thresholds, nq, dkw_eps, rim1, std_, minf, q, sorted_out)
def test_reduce_metrics(rec, backend):
    fid, thr = np.random.RandomState(5).rand(C, K), np.array([0.95, 0.98])
    res = backend.reduce_metrics(fid, q_thresholds=thr, dkw_eps=0.01, want_sorted=True, device=0)
    assert sorted(res) == ["min", "q", "rim1", "sorted", "std"]
    assert seen(rec, "rc_reduce_f64") == (
        0, P(fid), C, K, P(thr), 2, 0.01, out_ptr(res, "rim1", (3, C)), out_ptr(res, "std", (3, C)), out_ptr(res, "min", (3, C)),
        out_ptr(res, "q", (3, 2, C)), out_ptr(res, "sorted", (C, K)))


def test_reduce_metrics_without_thresholds(rec, backend):
    fid, thr = np.random.RandomState(5).rand(C, K), np.empty(0)
    res = backend.reduce_metrics(fid, q_thresholds=thr)
    assert sorted(res) == ["min", "q", "rim1", "std"] and res["q"].shape == (3, 0, C)
    assert seen(rec, "rc_reduce_f64") == (
        0, P(fid), C, K, P(thr), 0, 0.0, out_ptr(res, "rim1", (3, C)), out_ptr(res, "std", (3, C)), out_ptr(res, "min", (3, C)),
        None, None)


# int rc_rim_p_f64(device, fid, C, K, p, out)
def test_rim_p(rec, backend):
    fid = np.random.RandomState(5).rand(C, K)
    res = backend.rim_p(fid, 2.5, device=0)
    assert isinstance(res, np.ndarray) and res.shape == (C,) and res.dtype == np.float64
    assert seen(rec, "rc_rim_p_f64") == (0, P(fid), C, K, 2.5, P(res))


# int rc_draws_philox_f64(device, seed, offset, n, scale, out)
def test_philox_normal(rec, backend):
    res = backend.philox_normal((C, K, N, 3), seed=2 ** 63 + 5, scale=0.05, offset=7, device=0)
    assert isinstance(res, np.ndarray) and res.shape == (C, K, N, 3) and res.dtype == np.float64
    assert seen(rec, "rc_draws_philox_f64") == (0, 2 ** 63 + 5, 7, C * K * N * 3, 0.05, P(res))


# int rc_bootstrap_metrics_f64(device, fid, C, K, B, seed, offset, q_thresholds, nq, rank_lo, rank_hi, route, rep_out, summary_out)
def test_bootstrap_metrics(rec, backend):
    boot = importlib.import_module("code-robchar_amd.bootstrap")
    fid, thr, B = np.random.RandomState(5).rand(C, K), np.array([0.95, 0.98]), 40
    lo, hi = boot.ranks(B, 0.9)
    res = backend.bootstrap_metrics(fid, B, seed=11, offset=3, q_thresholds=thr, conf=0.9, route="global", device=0)
    assert sorted(res) == ["names", "replicates", "summary"] and list(res["names"]) == list(boot.metric_names(2))
    assert seen(rec, "rc_bootstrap_metrics_f64") == (
        0, P(fid), C, K, B, 11, 3, P(thr), 2, lo, hi, 2, out_ptr(res, "replicates", (5, C, B)), out_ptr(res, "summary", (5, 4, C)))


def test_bootstrap_metrics_without_thresholds_one_output(rec, backend):
    boot = importlib.import_module("code-robchar_amd.bootstrap")
    fid, B = np.random.RandomState(5).rand(C, K), 8
    lo, hi = boot.ranks(B, 0.95)
    res = backend.bootstrap_metrics(fid, B, seed=0, q_thresholds=(), want=("summary",))
    assert sorted(res) == ["names", "summary"]
    assert seen(rec, "rc_bootstrap_metrics_f64") == (
        0, P(fid), C, K, B, 0, 0, None, 0, lo, hi, 0, None, out_ptr(res, "summary", (3, 4, C)))
    rec.calls.clear()
    res = backend.bootstrap_metrics(fid, B, seed=0, q_thresholds=(), want=("replicates",), route="lds")
    assert seen(rec, "rc_bootstrap_metrics_f64") == (
        0, P(fid), C, K, B, 0, 0, None, 0, lo, hi, 1, out_ptr(res, "replicates", (3, C, B)), None)


# ------------------------------------------------------------------------------------------------------------- the refusals
def refused(rec, argument, call, *args, **kwargs):
    with pytest.raises(ValueError, match=argument):
        call(*args, **kwargs)
    assert rec.calls == []


def test_refusals_of_the_draw_tensor_entries(rec, backend):
    ctrl, draws, _, _ = inputs()
    families = [(backend.mc_fidelity, "out"), (backend.mc_fidelity_grad, "want"), (backend.mc_fidelity_sens, "want"),
                (backend.mc_fidelity_times, "want")]
    for fn, _ in families:
        refused(rec, "Nspin", fn, np.ones((C, 2)), np.zeros((C, K, 1, 3)), 1, 0, 0)
        refused(rec, "Nspin", fn, np.ones((C, 34)), np.zeros((C, K, 33, 3)), 33, 0, 0)
        refused(rec, "outspin", fn, ctrl, draws, N, 0, N)
        refused(rec, "inspin", fn, ctrl, draws, N, -1, 0)
        refused(rec, "draws", fn, ctrl, np.zeros((C, K, N + 1, 3)), N, 0, 2)
        refused(rec, "draws", fn, ctrl, np.zeros((C, K, N, 2)), N, 0, 2)
        refused(rec, "controllers", fn, np.ones((C, N + 2)), draws, N, 0, 2)
        refused(rec, "h0_diag", fn, ctrl, draws, N, 0, 2, h0_diag=np.zeros(N + 1))
        refused(rec, "h0_offdiag", fn, ctrl, draws, N, 0, 2, h0_offdiag=np.zeros(N))
    for fn, kw in families[1:]:
        refused(rec, "want", fn, ctrl, draws, N, 0, 2, **{kw: ()})
        refused(rec, "want", fn, ctrl, draws, N, 0, 2, **{kw: ("fid", "hessian")})


def test_refusals_of_the_readout_time_grid(rec, backend):
    ctrl, draws, _, _ = inputs()
    for fn, second in ((backend.mc_fidelity_times, draws), (backend.mc_fidelity_times_philox, K)):
        kw = {} if fn is backend.mc_fidelity_times else {"seed": 1}
        refused(rec, "needs weights", fn, ctrl, second, N, 0, 2, tshift=np.zeros(M), want=("wsum",), **kw)
        refused(rec, "tscale, tshift and weights must have one length", fn, ctrl, second, N, 0, 2, tscale=np.ones(2), tshift=np.zeros(3), **kw)
        refused(rec, "tscale, tshift and weights must have one length", fn, ctrl, second, N, 0, 2, tscale=np.ones(2), weights=np.zeros(3), **kw)
        refused(rec, "grid must hold 1 .. 64", fn, ctrl, second, N, 0, 2, tshift=np.zeros(0), **kw)
        refused(rec, "grid must hold 1 .. 64", fn, ctrl, second, N, 0, 2, tshift=np.zeros(65), **kw)
        refused(rec, "N <= 16", fn, np.ones((C, 18)), (np.zeros((C, K, 17, 3)) if second is draws else K), 17, 0, 16, **kw)


def test_refusals_of_the_generated_draws_entries(rec, backend):
    """every one of them before the library is touched: nothing may have been loaded, nothing called"""
    ctrl = np.ones((C, N + 1))
    listed = lambda c, k, *a, **kw: backend.mc_fidelity_grad_listed(c, k, np.zeros((len(c), 2), dtype=np.int32), None, *a, **kw)
    positional = lambda fn: (lambda c, k, n, i, o, **kw: fn(c, k, n, i, o, **kw))
    by_name = lambda c, k, n, i, o, **kw: listed(c, k, nspin=n, inspin=i, outspin=o, **kw)
    for fn in (positional(backend.mc_fidelity_sens_philox), positional(backend.mc_fidelity_grad_philox),
               positional(backend.mc_fidelity_times_philox), by_name):
        refused(rec, "Nspin", fn, np.ones((C, 2)), K, 1, 0, 0, seed=1)
        refused(rec, "outspin", fn, ctrl, K, N, 0, N, seed=1)
        refused(rec, "want", fn, ctrl, K, N, 0, 2, seed=1, want=())
        refused(rec, "want", fn, ctrl, K, N, 0, 2, seed=1, want=("fid", "hessian"))
        refused(rec, "controllers", fn, np.ones((C, N + 2)), K, N, 0, 2, seed=1)
        refused(rec, "controllers", fn, np.ones(N + 1), K, N, 0, 2, seed=1)
        refused(rec, "n_draws", fn, ctrl, -1, N, 0, 2, seed=1)
        refused(rec, "sigma", fn, ctrl, K, N, 0, 2, seed=1, sigma=np.ones(C + 1))
        refused(rec, "sigma", fn, ctrl, K, N, 0, 2, seed=1, sigma=np.ones((C, 1)))
        refused(rec, "h0_diag", fn, ctrl, K, N, 0, 2, seed=1, h0_diag=np.zeros(N + 1))
        refused(rec, "h0_offdiag", fn, ctrl, K, N, 0, 2, seed=1, h0_offdiag=np.zeros(N))


def test_refusals_of_the_metric_entries(rec, backend):
    fid = np.zeros((C, K))
    refused(rec, "fid", backend.reduce_metrics, np.zeros(K))
    refused(rec, "want", backend.bootstrap_metrics, fid, 8, seed=1, want=())
    refused(rec, "want", backend.bootstrap_metrics, fid, 8, seed=1, want=("summary", "mean"))
    refused(rec, "route", backend.bootstrap_metrics, fid, 8, seed=1, route="fast")
    refused(rec, "fid", backend.bootstrap_metrics, np.zeros(K), 8, seed=1)
    refused(rec, "K must be positive", backend.bootstrap_metrics, np.zeros((C, 0)), 8, seed=1)
    refused(rec, "n_boot", backend.bootstrap_metrics, fid, 0, seed=1)
    refused(rec, "seed", backend.bootstrap_metrics, fid, 8, seed=-1)
    refused(rec, "offset", backend.bootstrap_metrics, fid, 8, seed=1, offset=2 ** 64)
    refused(rec, "want", backend.tail_select, fid, 0.5, want=("list", "mean"))
    refused(rec, "alpha", backend.tail_select, fid, 0.0)
    refused(rec, "fid", backend.tail_select, np.zeros(K), 0.5)
    refused(rec, "want", backend.lbfgs_result, None, None, want=())
    refused(rec, "want", backend.lbfgs_result, None, None, want=("x", "hessian"))
