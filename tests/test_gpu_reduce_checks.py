"""`backend.reduce_metrics` and `backend.rim_p` on the device against the known answers of tests/reduce_checks.py: every check through
the blocking entry (NumPy in) and through the enqueue entry on CUDA tensors with both overlap hints - the exact outputs hold for
every hint -, the input tensor untouched by the out-of-place sort, the hint changing nothing outside 8192 < K <= 10240, and
`rc_reduce_f64` with every output pointer alone (the others NULL)."""
import ctypes
import importlib

import numpy as np
import pytest

import reduce_checks as rc

pytestmark = pytest.mark.gpu


def blocking(be):
    return lambda F, **kw: be.reduce_metrics(F, **kw)


def on_tensors(be, overlapped):
    def reduce(F, **kw):
        import torch
        Ft = torch.from_numpy(F).cuda()
        keep = Ft.clone()
        res = be.reduce_metrics(Ft, overlapped=overlapped, **kw)
        res = {k: v.cpu().numpy() for k, v in res.items()}
        assert keep.cpu().numpy().tobytes() == Ft.cpu().numpy().tobytes()          # NaN included: the bytes
        return res
    return reduce


def reducers(be):
    return (blocking(be), on_tensors(be, True), on_tensors(be, False))


def rim_ps(be):
    def on_tensor(F, p):
        import torch
        Ft = torch.from_numpy(F).cuda()
        keep = Ft.clone()
        out = be.rim_p(Ft, p).cpu().numpy()
        assert keep.cpu().numpy().tobytes() == Ft.cpu().numpy().tobytes()
        return out
    return (lambda F, p: be.rim_p(F, p), on_tensor)


@pytest.mark.parametrize("nq", [0, 2, 3, 8])
def test_grid_rows_every_route(be, nq):
    for reduce in reducers(be):
        rc.check_grid(reduce, nqs=(nq,))


@pytest.mark.parametrize("check", [rc.check_nan_rows, rc.check_alone, rc.check_highfid, rc.check_sort_nan], ids=lambda c: c.__name__)
def test_checks(be, check):
    for reduce in reducers(be):
        check(reduce)


@pytest.mark.parametrize("K", rc.SORT_K)
def test_sort(be, K):
    for reduce in reducers(be):
        rc.check_sort(reduce, ks=(K,))


@pytest.mark.parametrize("K", rc.RIMP_K)
def test_rim_p(be, K):
    for rim_p in rim_ps(be):
        rc.check_rim_p(rim_p, ks=(K,))


@pytest.mark.parametrize("nq", [2, 8])
def test_the_hint_matters_for_one_row_length_only(be, nq):
    """the standalone hint IS the blocking entry's route, and outside 8192 < K <= 10240 both hints give the same bytes, std included"""
    thr = rc.THRESHOLDS[nq][0]
    for K in rc.ks_of(nq):
        F, t, _ = rc.case(("grid", K, 3, nq, 0, 0), lambda: rc.grid_slab(K, 3, thr, 0), rc.GRID, 16, thr)
        host, ov, alone = (r(F.copy(), q_thresholds=t, dkw_eps=rc.EPS) for r in reducers(be))
        for name in ("rim1", "std", "min", "q"):
            assert np.ascontiguousarray(alone[name]).tobytes() == host[name].tobytes(), (K, name)
            if name != "std" or not (8192 < K <= 10240):
                assert np.ascontiguousarray(ov[name]).tobytes() == host[name].tobytes(), (K, name)


@pytest.mark.parametrize("K", [100, 5000, 20000])
def test_any_output_pointer_may_be_null(be, K):
    """include/robchar_hip.h: "Any output pointer may be NULL to skip it" - each output alone gives the bytes of the call with all
    of them (std_ = NULL skips the kernel's second pass; q = NULL with nq = 2; sorted_out alone launches no reduction at all)"""
    lib = importlib.import_module("code-robchar_amd._lib").load()
    thr = rc.THRESHOLDS[2][0]
    F, t, ref = rc.case(("grid", K, 3, 2, 0, 0), lambda: rc.grid_slab(K, 3, thr, 0), rc.GRID, 16, thr)
    C = F.shape[0]
    shapes = {"rim1": (3, C), "std": (3, C), "min": (3, C), "q": (3, 2, C), "sorted": (C, K)}

    def call(want):
        out = {name: np.full(shapes[name], -7.0) for name in want}
        ptr = lambda name: ctypes.c_void_p(out[name].ctypes.data) if name in out else None
        src = F.copy()
        assert lib.rc_reduce_f64(0, ctypes.c_void_p(src.ctypes.data), C, K, ctypes.c_void_p(t.ctypes.data), 2, rc.EPS,
                                 *(ptr(name) for name in shapes)) == 0
        assert src.tobytes() == F.tobytes()
        return out

    full = call(tuple(shapes))
    rc.compare(full, ref, ("all outputs", K))
    assert np.array_equal(full["sorted"], np.sort(F, axis=1))
    for wanted in [(name,) for name in shapes] + [("rim1", "min", "q", "sorted"), ("rim1", "std", "min", "sorted"), ("std", "q")]:
        got = call(wanted)
        for name in wanted:
            assert got[name].tobytes() == full[name].tobytes(), (K, wanted, name)
