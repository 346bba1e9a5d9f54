"""The per-sample arithmetic of the readout-time kernels (code-robchar_amd/csrc/times_core.h) compiled for the host with g++
(tests/host/host_times.cpp) and held to the checks of times_checks.py - runs without a GPU.  Two routes on every input: the
kernels' order (register-resident QL with the rows `in` and `out`; the textbook routine only for a sample whose QL hits the
sweep cap) and the textbook routine forced for every sample (the kernels' fallback).  And the claim the GPU suite repeats on the
device: at one time the new pieces give the bits of chain_fidelity_fast<N, kWeightsRows>."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import chain_checks as cc
import times_checks as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.POINTER(ctypes.c_double)
LL = ctypes.c_longlong


def _p(a):
    return a.ctypes.data_as(P) if a is not None else None


class HostBackend:
    """`mc_fidelity_times`, `readout_times` and the rows-mode `mc_fidelity` of the backend through the host build"""

    def __init__(self, lib, force_general):
        self.lib, self.force_general = lib, force_general

    readout_times = staticmethod(tc.times_of)          # (the backend's is NumPy too; the kernel's own rounding is what the slabs test)

    def _common(self, ctrl, draws, N, h0_diag, h0_offdiag):
        ctrl = np.ascontiguousarray(ctrl, dtype=np.float64)
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        C, K = ctrl.shape[0], draws.shape[1]
        stride = 0 if (draws.shape[0] == 1 and C > 1) else K * N * 3
        h0d = np.zeros(N) if h0_diag is None else np.ascontiguousarray(h0_diag, dtype=np.float64)
        h0o = np.ones(max(N - 1, 1)) if h0_offdiag is None else np.ascontiguousarray(h0_offdiag, dtype=np.float64)
        return ctrl, draws, C, K, stride, h0d, h0o

    def mc_fidelity_times(self, ctrl, draws, N, a, b, tscale=None, tshift=None, weights=None, want=("fid",), h0_diag=None,
                          h0_offdiag=None, device=None):
        ctrl, draws, C, K, stride, h0d, h0o = self._common(ctrl, draws, N, h0_diag, h0_offdiag)
        vec = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
        ts, th, w = vec(tscale), vec(tshift), vec(weights)
        M = max([len(v) for v in (ts, th, w) if v is not None] + [1])
        F, W, Fm = np.empty((M, C, K)), np.empty((C, K)), np.empty((C, K))
        rc = self.lib.rc_host_chain_fidelity_times(N, _p(np.nan_to_num(ctrl)), _p(h0d), _p(h0o), _p(draws), LL(stride), LL(C), LL(K), a, b,
                                                   self.force_general, M, _p(ts), _p(th), _p(w), _p(F), _p(W), _p(Fm))
        assert rc == 0
        nan = np.isnan(ctrl).any(axis=1)              # (the kernels' rule for a padded row; the per-sample arithmetic never sees one)
        F[:, nan] = np.nan
        W[nan] = np.nan
        Fm[nan] = np.nan
        res = {"fid": F, "wsum": W, "min": Fm}
        return {k: res[k] for k in want}

    def mc_fidelity(self, ctrl, draws, N, a, b, h0_diag=None, h0_offdiag=None, kernel="tridiag_ql", **kw):
        assert kernel == "tridiag_ql"
        ctrl, draws, C, K, stride, h0d, h0o = self._common(ctrl, draws, N, h0_diag, h0_offdiag)
        F = np.empty((C, K))
        assert self.lib.rc_host_chain_fidelity_rows(N, _p(ctrl), _p(h0d), _p(h0o), _p(draws), LL(stride), LL(C), LL(K), a, b, _p(F)) == 0
        return F


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    out = tmp_path_factory.mktemp("hosttimes") / "librc_hosttimes.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                    os.path.join(ROOT, "tests", "host", "host_times.cpp")], check=True)
    lib = ctypes.CDLL(str(out))
    lib.rc_host_times_general_calls.restype = ctypes.c_longlong
    return lib


@pytest.fixture(params=[0, 1], ids=["kernel-order", "textbook-forced"])
def host(request, hostlib):
    return HostBackend(hostlib, request.param)


@pytest.mark.parametrize("N", range(2, 17))
def test_every_size_end_to_end_vs_oracle(host, N):
    worst = cc.Worst()
    tc.check_oracle(host, N, 0, N - 1, worst)
    print("host times:", worst)


@pytest.mark.parametrize("N,a,b", [p for p in tc.PAIRS if p[1:] != (0, p[0] - 1)])
def test_interior_pairs_vs_oracle(host, N, a, b):
    tc.check_oracle(host, N, a, b)


@pytest.mark.parametrize("N", [3, 7, 16])
def test_closed_form(host, N):
    tc.check_closed_form(host, N)


def test_semantics_and_edges(host):
    tc.check_semantics(host)
    tc.check_edges(host)


@pytest.mark.parametrize("N", range(2, 17))
def test_one_time_is_the_rows_mode_bit_for_bit(hostlib, N):
    """times_eigen_fast + times_phase_fid at t against chain_fidelity_fast<N, kWeightsRows> with x[N] = t: the same operations"""
    host = HostBackend(hostlib, 0)
    n0 = hostlib.rc_host_times_general_calls()
    for (a, b) in ((0, N - 1), (N // 2, max(0, N // 2 - 1)), (N - 1, N - 1)):
        assert tc.check_against_rows_kernel(host, N, a, b) == 0.0
    assert hostlib.rc_host_times_general_calls() == n0                   # the fast route needed no fallback


def test_textbook_route_is_exercised(hostlib):
    n0 = hostlib.rc_host_times_general_calls()
    tc.check_oracle(HostBackend(hostlib, 0), 7, 0, 6)
    n1 = hostlib.rc_host_times_general_calls()
    tc.check_oracle(HostBackend(hostlib, 1), 7, 0, 6)
    n2 = hostlib.rc_host_times_general_calls()
    assert n1 - n0 == 0 and n2 - n1 == 3 * 70


def test_a_null_matrix_takes_the_textbook_routine_in_kernel_order(hostlib):
    """every bond cut and every bias zero: H = 0, no coupling is ever negligible against |d_l| + |d_l+1| = 0, the fast QL runs
    into its sweep cap and the sample takes the textbook routine - the one input known to; the same chain at a bias of 0.25 (a
    global phase away) stays on the fast path"""
    host = HostBackend(hostlib, 0)
    N, K = 7, 5
    ctrl = np.zeros((2, N + 1))
    ctrl[:, N] = (3.0, 2.0)
    ctrl[0, :N] = 0.25
    draws = np.zeros((2, K, N, 3))
    draws[:, :, 1:, 1] = -1.0
    n0 = hostlib.rc_host_times_general_calls()
    res = host.mc_fidelity_times(ctrl, draws, N, 0, 2, tscale=tc.TSCALE, tshift=tc.TSHIFT, weights=np.ones(5), want=("fid", "wsum", "min"))
    same = host.mc_fidelity_times(ctrl, draws, N, 3, 3, tscale=tc.TSCALE, tshift=tc.TSHIFT, want=("fid", "min"))
    assert hostlib.rc_host_times_general_calls() - n0 == 2 * K           # row 1 only, in both calls
    assert all(np.abs(v).max() < 1e-200 for v in res.values())
    assert np.abs(same["fid"] - 1.0).max() < 1e-14 and np.abs(same["min"] - 1.0).max() < 1e-14
