"""The blocking entries `rc_mc_fidelity_grad_f64` and `rc_mc_fidelity_sens_f64` take host or device pointers for either input and
any output (one routine stages whatever is on the host through the device's workspace).  Every mix must give the all-host-pointer
call's results bit for bit.  N = 3: the smallest N with two staging phases; K = 65: two tiles per row, the second with one sample,
so that a wrong size or offset in the carving of the workspace shows."""
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
