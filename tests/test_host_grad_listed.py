"""grad_eigensystem_fast<N, R, FREEZE = true> - the QL of mc_fid_grad_listed_kernel - gives every lane the bits it gets alone in
a wave, whatever the other lanes hold; FREEZE = false (every other kernel) does not, and both are inside the bars of each other
and of the reference.  64 lanes in lock step on the CPU (tests/host/host_grad_listed.cpp, the harness of host_wave.cpp).  The
same property on inputs of its own is what the stand-alone build of that file checks - the one a sanitizer can be put on."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import chain_checks as cc
import grad_checks as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "host_grad_listed.cpp")
FLAGS = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread"]
P = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def wave(tmp_path_factory):
    """wave(ctrl_row, draws (n, N, 3), lanes, N, a, b, freeze) -> (fid (n,), grad (n, N+1), votes (n,), ok (n,)); only the entries
    of `lanes` are written"""
    out = tmp_path_factory.mktemp("hostgradlisted") / "librc_hostgradlisted.so"
    subprocess.run(FLAGS + ["-shared", "-fPIC", "-o", str(out), SRC], check=True)
    lib = ctypes.CDLL(str(out))

    def run(ctrl, draws, lanes, N, a, b, freeze):
        ctrl = np.ascontiguousarray(ctrl, dtype=np.float64).reshape(-1)
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        lanes = np.ascontiguousarray(lanes, dtype=np.int32)
        n = draws.shape[0]
        h0d, h0o = np.zeros(32), np.ones(32)
        fid, grad = np.full(n, np.nan), np.full((n, N + 1), np.nan)
        votes, ok = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
        rc = lib.rc_host_wave_grad(N, ctrl.ctypes.data_as(P), h0d.ctypes.data_as(P), h0o.ctypes.data_as(P), draws.ctypes.data_as(P),
                                   lanes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(lanes), a, b, int(freeze),
                                   fid.ctypes.data_as(P), grad.ctypes.data_as(P), votes.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                                   ok.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        assert rc == 0
        return fid, grad, votes, ok
    return run


def mixed_samples(N, seed):
    """one delocalised controller row and 64 samples: two in three with sigma = 0.05 draws (delocalised: the QL needs its
    sweeps), one in three with biases of +-40 on top (localised: the couplings are negligible after a sweep or two)"""
    rng = np.random.default_rng(seed)
    ctrl = cc.deloc_ctrl(rng, 1, N, 0.5)[0]
    draws = 0.05 * rng.standard_normal((64, N, 3))
    draws[::3, :, 0] += rng.uniform(-40.0, 40.0, (22, N))
    return ctrl, draws


@pytest.mark.parametrize("N", [3, 7, 10])
def test_frozen_lanes_do_not_see_their_mates(wave, N):
    ctrl, draws = mixed_samples(N, 8800 + N)
    a, b = 0, N - 1
    rng = np.random.default_rng(N)
    every = np.arange(64)
    alone_f, alone_g, alone_v = np.empty(64), np.empty((64, N + 1)), np.empty(64, dtype=np.int64)
    loose_f, loose_g = np.empty(64), np.empty((64, N + 1))
    for l in every:
        f, g, v, ok = wave(ctrl, draws, [l], N, a, b, True)
        assert ok[l] == 1
        alone_f[l], alone_g[l], alone_v[l] = f[l], g[l], v[l]
        f, g, _, _ = wave(ctrl, draws, [l], N, a, b, False)
        loose_f[l], loose_g[l] = f[l], g[l]
    # the sweep counts within the wave really differ: alone, the samples take part in different numbers of votes
    print(f"N = {N}: votes of a sample alone {alone_v.min()} .. {alone_v.max()} (localised {np.median(alone_v[::3])}, "
          f"delocalised {np.median(alone_v[1::3])})")
    assert alone_v.max() > alone_v.min() and np.median(alone_v[::3]) < np.median(alone_v[1::3])
    # FREEZE: the same bits among all 64, among another set of mates, and in other lanes' company in reversed order
    full_f, full_g, _, ok = wave(ctrl, draws, every, N, a, b, True)
    assert ok.all()
    assert np.array_equal(full_f, alone_f) and np.array_equal(full_g, alone_g)
    some = np.sort(rng.permutation(64)[:23])
    part_f, part_g, _, _ = wave(ctrl, draws, some[::-1], N, a, b, True)
    assert np.array_equal(part_f[some], alone_f[some]) and np.array_equal(part_g[some], alone_g[some])
    # without it the wave's vote shows in the bits of some lane (or this test would have no teeth) ...
    vote_f, vote_g, _, ok = wave(ctrl, draws, every, N, a, b, False)
    assert ok.all()
    changed = int((vote_f != loose_f).sum() + (vote_g != loose_g).any(axis=1).sum())
    print(f"N = {N}: FREEZE = false, lanes whose bits change with their mates: {changed}")
    assert changed > 0
    # ... and both are inside the bars of each other and of the reference
    Fw, Gw = gc.grad_eigh(ctrl[None, :], draws[None], N, a, b)
    bars = gc.grad_bars(ctrl[None, :], draws[None], N)[0]
    for f, g in ((full_f, full_g), (vote_f, vote_g), (loose_f, loose_g)):
        assert np.abs(f - Fw[0]).max() < gc.TOL and (np.abs(g - Gw[0]) < bars).all()
    assert np.abs(full_f - vote_f).max() < gc.TOL and (np.abs(full_g - vote_g) < bars).all()


def test_stand_alone_program(tmp_path):
    exe = tmp_path / "host_grad_listed"
    subprocess.run(FLAGS + ["-DRC_HOST_GRAD_LISTED_MAIN", "-o", str(exe), SRC], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
