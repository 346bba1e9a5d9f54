"""The blocking entries `rc_mc_fidelity_grad_f64` and `rc_mc_fidelity_sens_f64` take host or device pointers for either input and
any output (one routine stages whatever is on the host through the device's workspace).  Every mix must give the all-host-pointer
call's results bit for bit.  N = 3: the smallest N with two staging phases; K = 65: two tiles per row, the second with one sample,
so that a wrong size or offset in the carving of the workspace shows.

The other blocking entries that stage through the same workspace plan - `rc_mc_fidelity_kernel_f64`, `rc_reduce_f64`,
`rc_rim_p_f64`, `rc_draws_philox_f64` - are held to the same rule below, on the same shape."""
import ctypes
import importlib
import itertools

import numpy as np
import pytest

import chain_checks as cc

pytestmark = pytest.mark.gpu
N, C, K, A, B = 3, 2, 65, 0, 2
# entry -> doubles per sample of the second output, doubles per row of the mean (include/robchar_hip.h)
ENTRIES = {"grad": (N + 1, N + 2), "sens": (3 * N, 3 * N + 2)}


@pytest.fixture(scope="module")
def inputs(be):
    ctrl = cc.deloc_ctrl(np.random.default_rng(5), C, N, 0.5)
    draws = be.philox_normal((C, K, N, 3), seed=2024, scale=0.05)
    return np.ascontiguousarray(ctrl), np.ascontiguousarray(draws)


def run(which, ctrl, draws, stride, ctrl_dev, draws_dev, outs_dev, want=(True, True, True)):
    """One blocking call; the inputs and the requested outputs on the device (torch owns the memory) or on the host.
    Returns the requested outputs as NumPy arrays (None where not requested)."""
    import torch
    lib = importlib.import_module("code-robchar_amd._lib").load()
    per_sample, per_row = ENTRIES[which]
    dev = torch.device("cuda", torch.cuda.current_device())
    sizes = (C * K, C * K * per_sample, C * per_row)
    keep, args = [], []
    for a, on_dev in ((ctrl, ctrl_dev), (draws, draws_dev)):
        t = torch.from_numpy(a).to(dev) if on_dev else a
        keep.append(t)
        args.append(ctypes.c_void_p(t.data_ptr() if on_dev else t.ctypes.data))
    outs = []
    for n, w in zip(sizes, want):
        o = None
        if w:               # (a sentinel that no result equals: an element the call did not write fails the comparison)
            o = torch.full((n,), -7.0, dtype=torch.float64, device=dev) if outs_dev else np.full(n, -7.0)
        outs.append(o)
        args.append(None if o is None else ctypes.c_void_p(o.data_ptr() if outs_dev else o.ctypes.data))
    torch.cuda.synchronize()                      # the entry runs on the library's own stream
    rc = getattr(lib, f"rc_mc_fidelity_{which}_f64")(dev.index or 0, N, A, B, None, None, args[0], args[1], stride, C, K, *args[2:])
    assert rc == 0, lib.rc_last_error()
    return [None if o is None else (o.cpu().numpy() if outs_dev else o) for o in outs]


@pytest.fixture(scope="module")
def reference(be, inputs):
    """the all-host-pointer calls: private draws per controller row"""
    ref = {w: run(w, *inputs, K * N * 3, False, False, False) for w in ENTRIES}
    for w, outs in ref.items():
        for o in outs:
            assert np.isfinite(o).all() and np.abs(o).max() > 1e-3 and not (o == -7.0).any(), w
    return ref


@pytest.mark.parametrize("which", list(ENTRIES))
def test_every_mix_of_host_and_device_pointers(be, inputs, reference, which):
    for ctrl_dev, draws_dev, outs_dev in itertools.product((False, True), repeat=3):
        got = run(which, *inputs, K * N * 3, ctrl_dev, draws_dev, outs_dev)
        for name, g, r in zip(("fid", which, "mean"), got, reference[which]):
            assert np.array_equal(g, r), (which, name, ctrl_dev, draws_dev, outs_dev)


@pytest.mark.parametrize("which", list(ENTRIES))
def test_shared_draw_set(be, inputs, which):
    """draws_ctrl_stride = 0: one set of K draws for both rows"""
    ctrl, draws = inputs[0], np.ascontiguousarray(inputs[1][:1])
    ref = run(which, ctrl, draws, 0, False, False, False)
    assert all(np.isfinite(r).all() and not (r == -7.0).any() for r in ref)
    assert not np.array_equal(ref[0][:K], ref[0][K:])                     # (two different controller rows)
    for ctrl_dev, draws_dev, outs_dev in ((False, True, False), (True, False, True), (True, True, True)):
        got = run(which, ctrl, draws, 0, ctrl_dev, draws_dev, outs_dev)
        for g, r in zip(got, ref):
            assert np.array_equal(g, r), (which, ctrl_dev, draws_dev, outs_dev)


@pytest.mark.parametrize("which", list(ENTRIES))
def test_mean_only(be, inputs, reference, which):
    """only mean_out requested: the workspace then holds the inputs and the mean rows alone"""
    ref = run(which, *inputs, K * N * 3, False, False, False, want=(False, False, True))
    assert ref[0] is None and ref[1] is None and np.isfinite(ref[2]).all() and not (ref[2] == -7.0).any()
    assert np.array_equal(ref[2], reference[which][2])                    # (the row means do not depend on what else is stored)
    for ctrl_dev, draws_dev, outs_dev in ((True, False, False), (False, True, True), (True, True, True)):
        got = run(which, *inputs, K * N * 3, ctrl_dev, draws_dev, outs_dev, want=(False, False, True))
        assert np.array_equal(got[2], ref[2]), (which, ctrl_dev, draws_dev, outs_dev)


# ----------------------------------------------------------------------------------------------------------------
# the other blocking entries: same shape, same sentinel, every mix against the all-host call
# ----------------------------------------------------------------------------------------------------------------
THR, EPS = np.array([0.9, 0.99]), 0.05                   # rc_reduce_f64: two thresholds, a DKW band
SMALL = {"rim1": 3 * C, "std": 3 * C, "min": 3 * C, "q": 3 * len(THR) * C}      # its four small outputs, in argument order
NDRAWS = 2 * 65 * 3 * 3 + 1                              # rc_draws_philox_f64: odd, so the last Box-Muller pair is half used


def place(a, on_dev):
    """an input array on the host or on the device: (owner, pointer)"""
    import torch
    t = torch.from_numpy(a).cuda() if on_dev else a
    return t, ctypes.c_void_p(t.data_ptr() if on_dev else t.ctypes.data)


def sentinel(n, where):
    """an output of n doubles that no result equals; where: None (not requested), "host" or "dev": (owner, pointer)"""
    import torch
    if where is None:
        return None, None
    o = torch.full((n,), -7.0, dtype=torch.float64, device="cuda") if where == "dev" else np.full(n, -7.0)
    return o, ctypes.c_void_p(o.data_ptr() if where == "dev" else o.ctypes.data)


def call(name, *args):
    """one blocking call on the current device; returns nothing: the outputs are the owners `sentinel` gave"""
    import torch
    lib = importlib.import_module("code-robchar_amd._lib").load()
    torch.cuda.synchronize()                      # the entry runs on the library's own stream
    rc = getattr(lib, name)(torch.cuda.current_device(), *args)
    assert rc == 0, lib.rc_last_error()


def host(o):
    return None if o is None else (o if isinstance(o, np.ndarray) else o.cpu().numpy())


def run_fidelity(ctrl, draws, ctrl_dev, draws_dev, fid_dev):
    (kc, pc), (kd, pd) = place(ctrl, ctrl_dev), place(draws, draws_dev)
    o, po = sentinel(C * K, "dev" if fid_dev else "host")
    call("rc_mc_fidelity_kernel_f64", 0, N, A, B, None, None, 0, pc, pd, C, K, po)
    return host(o)


def run_reduce(fid, fid_dev, small, sorted_where, want=tuple(SMALL)):
    """`small`: where the requested ones of the four small outputs live; returns {name: array} of what was requested"""
    kf, pf = place(fid, fid_dev)
    outs = {k: sentinel(n, small if k in want else None) for k, n in SMALL.items()}
    outs["sorted"] = sentinel(C * K, sorted_where)
    thr = np.ascontiguousarray(THR)
    call("rc_reduce_f64", pf, C, K, ctypes.c_void_p(thr.ctypes.data), len(THR), EPS, *(p for _, p in outs.values()))
    return {k: host(o) for k, (o, _) in outs.items() if o is not None}


def run_rim_p(fid, fid_dev, out_dev):
    kf, pf = place(fid, fid_dev)
    o, po = sentinel(C, "dev" if out_dev else "host")
    call("rc_rim_p_f64", pf, C, K, 2.0, po)
    return host(o)


def run_draws(out_dev):
    o, po = sentinel(NDRAWS, "dev" if out_dev else "host")
    call("rc_draws_philox_f64", 2024, 12345, NDRAWS, 0.05, po)
    return host(o)


def written(o):
    return np.isfinite(o).all() and not (o == -7.0).any()


@pytest.fixture(scope="module")
def fid_reference(be, inputs):
    """the all-host-pointer fidelity call; the reductions below take its result as their input"""
    ref = run_fidelity(*inputs, False, False, False)
    assert written(ref) and ref.min() > 0.0 and ref.max() < 1.0 + 1e-12 and np.ptp(ref) > 1e-3
    return ref


@pytest.fixture(scope="module")
def reduce_reference(be, fid_reference):
    ref = run_reduce(fid_reference, False, "host", "host")
    assert all(written(v) for v in ref.values()) and set(ref) == set(SMALL) | {"sorted"}
    assert np.array_equal(ref["sorted"].reshape(C, K), np.sort(fid_reference.reshape(C, K), axis=1))
    assert np.abs(ref["rim1"][:C] - (1.0 - fid_reference.reshape(C, K)).mean(axis=1)).max() < 1e-12
    return ref


def test_fidelity_every_mix(be, inputs, fid_reference):
    for mix in itertools.product((False, True), repeat=3):
        assert np.array_equal(run_fidelity(*inputs, *mix), fid_reference), mix


def test_reduce_every_mix(be, fid_reference, reduce_reference):
    for fid_dev, sorted_where, small in itertools.product((False, True), (None, "host", "dev"), ("host", "dev")):
        got = run_reduce(fid_reference, fid_dev, small, sorted_where)
        assert set(got) == set(SMALL) | ({"sorted"} if sorted_where else set())
        for k, g in got.items():
            assert np.array_equal(g, reduce_reference[k]), (k, fid_dev, sorted_where, small)


@pytest.mark.parametrize("only", list(SMALL))
def test_reduce_one_small_output_alone(be, fid_reference, reduce_reference, only):
    """one of the four small outputs requested: the others take no workspace and the kernel gets NULL for them"""
    for small in ("host", "dev"):
        got = run_reduce(fid_reference, True, small, None, want=(only,))
        assert list(got) == [only] and np.array_equal(got[only], reduce_reference[only]), (only, small)


def test_rim_p_every_mix(be, fid_reference):
    ref = run_rim_p(fid_reference, False, False)
    assert written(ref) and (ref > 0.0).all() and ref[0] != ref[1]
    for mix in itertools.product((False, True), repeat=2):
        assert np.array_equal(run_rim_p(fid_reference, *mix), ref), mix


def test_draws_philox_host_and_device(be):
    ref = run_draws(False)
    assert written(ref) and 0.03 < ref.std() < 0.07 and len(np.unique(ref)) == NDRAWS
    assert np.array_equal(run_draws(True), ref)
