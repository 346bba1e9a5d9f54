"""The per-sample arithmetic of the fidelity-gradient kernel (code-robchar_amd/csrc/grad_core.h) compiled for the host with
g++ (tests/host/host_grad.cpp) and held to the bars of grad_checks.py - runs without a GPU.  Two routes are exercised on
every input: the kernel's order (register-resident QL with all eigenvector rows; the textbook routine only for a sample
whose QL hits the sweep cap) and the textbook routine forced for every sample (the kernel's fallback)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import chain_checks as cc
import grad_checks as gc
from oracle import robchar_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.POINTER(ctypes.c_double)


class HostBackend:
    """`mc_fidelity_grad` of the backend through the host build"""

    def __init__(self, lib, force_general):
        self.lib, self.force_general = lib, force_general

    def mc_fidelity_grad(self, ctrl, draws, N, a, b, h0_diag=None, h0_offdiag=None, device=None, want=("fid", "grad", "mean")):
        ctrl = np.ascontiguousarray(ctrl, dtype=np.float64)
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        C, K = ctrl.shape[0], draws.shape[1]
        stride = 0 if (draws.shape[0] == 1 and C > 1) else K * N * 3
        h0d = np.zeros(N) if h0_diag is None else np.ascontiguousarray(h0_diag, dtype=np.float64)
        h0o = np.ones(max(N - 1, 1)) if h0_offdiag is None else np.ascontiguousarray(h0_offdiag, dtype=np.float64)
        F, G = np.empty((C, K)), np.empty((C, K, N + 1))
        rc = self.lib.rc_host_chain_fidelity_grad(N, ctrl.ctypes.data_as(P), h0d.ctypes.data_as(P), h0o.ctypes.data_as(P),
                                                  draws.ctypes.data_as(P), ctypes.c_longlong(stride), ctypes.c_longlong(C),
                                                  ctypes.c_longlong(K), a, b, self.force_general, F.ctypes.data_as(P),
                                                  G.ctypes.data_as(P))
        assert rc == 0
        nan = np.isnan(ctrl).any(axis=1)              # (the kernel's rule for a padded row; the per-sample arithmetic never sees one)
        F[nan] = np.nan
        G[nan] = np.nan
        res = {"fid": F, "grad": G, "mean": np.concatenate([F.mean(axis=1)[:, None], G.mean(axis=1)], axis=1)}
        return {k: v for k, v in res.items() if k in want}


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    out = tmp_path_factory.mktemp("hostgrad") / "librc_hostgrad.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                    os.path.join(ROOT, "tests", "host", "host_grad.cpp")], check=True)
    lib = ctypes.CDLL(str(out))
    lib.rc_host_grad_general_calls.restype = ctypes.c_longlong
    return lib


@pytest.fixture(params=[0, 1], ids=["kernel-order", "textbook-forced"])
def host(request, hostlib):
    return HostBackend(hostlib, request.param)


def test_golden_kernel_cases(host, kernel_cases):
    """the golden chain / xxz cases: fidelity against the stored values, gradient against the eigh formulas"""
    worst = gc.Worst()
    for case in kernel_cases:
        if case["mode"] == "ring" or case["N"] > 12:
            continue
        N, a, b = case["N"], case["inspin"], case["outspin"]
        h0 = orc.xxz_delta(N) if case["mode"] == "xxz" else None
        for s in range(case["draws"].shape[0]):
            draws = case["draws"][s]
            res = host.mc_fidelity_grad(case["ctrl"], draws, N, a, b, h0_diag=h0, want=("fid", "grad"))
            assert np.abs(res["fid"] - case["fid"][s]).max() < 1e-11
            _, Gw = gc.grad_eigh(case["ctrl"], draws, N, a, b, h0)
            worst.add(case["mode"], gc.compare_grad(res["grad"], Gw, gc.grad_bars(case["ctrl"], draws, N, h0), case["name"]))
    print("host gradient, golden cases:", worst)


@pytest.mark.parametrize("N", [2, 3, 5, 7, 10, 12])
def test_deloc(host, N):
    worst = gc.Worst()
    gc.check_deloc_grad(host, N, worst)
    print("host gradient:", worst)


@pytest.mark.parametrize("N", [2, 3, 5, 7, 10, 12])
def test_hard_inputs(host, N):
    worst = gc.Worst()
    gc.check_hard_inputs(host, N, worst)
    print("host gradient:", worst)


@pytest.mark.parametrize("N", [3, 7, 12])
def test_hard_inputs_vs_frechet(host, N):
    """the same hard inputs against expm_frechet (shares neither gauge nor eigensolver with the code under test)"""
    gc.check_hard_inputs(host, N, ref=gc.grad_frechet)


@pytest.mark.parametrize("N", [3, 7, 12])
def test_closed_form(host, N):
    gc.check_closed_form_grad(host, N)


def test_textbook_route_is_exercised(hostlib):
    """The kernel-order route must not need the textbook routine on the hard inputs (its QL has no condition on gaps or
    cut bonds), and the forced route must run it for every sample: both counts are exposed."""
    rng = np.random.default_rng(1)
    n0 = hostlib.rc_host_grad_general_calls()
    gc.check_hard_inputs(HostBackend(hostlib, 0), 7)
    n1 = hostlib.rc_host_grad_general_calls()
    gc.check_hard_inputs(HostBackend(hostlib, 1), 7)
    n2 = hostlib.rc_host_grad_general_calls()
    nsamples = sum(d.shape[1] for _, _, d in gc.hard_inputs(7, rng)) * len(gc.grad_pairs(7))
    assert n1 - n0 == 0
    assert n2 - n1 == nsamples > 0
