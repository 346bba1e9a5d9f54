"""The per-sample time loop of the gradient kernel on a grid of readout times (code-robchar_amd/csrc/grad_times_core.h) compiled
for the host with g++ -ffp-contract=off (tests/host/host_grad_times.cpp) - runs without a GPU.  Both eigen routes (the kernel's
order; the textbook routine forced for every sample), N = 2 .. 12: inside the bars of the independent reference, and BIT FOR BIT
the existing single-time host arithmetic evaluated per grid time and combined by the exact fma sequence."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import grad_checks as gc
import grad_times_checks as gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.POINTER(ctypes.c_double)


def _p(a):
    return None if a is None else a.ctypes.data_as(P)


class HostBackend:
    """`mc_fidelity_grad_philox` and `mc_fidelity_grad_times_philox` of the backend through the host build, on draws regenerated
    on the host"""

    def __init__(self, lib, force_general):
        self.lib, self.force_general = lib, force_general

    def _run(self, ctrl, K, N, a, b, seed, offset, sigma, shared, grid, want):
        assert seed == gt.SEED
        ctrl = np.ascontiguousarray(ctrl, dtype=np.float64)
        C = ctrl.shape[0]
        draws = np.ascontiguousarray(gt.draws_of(ctrl, K, N, offset, shared, sigma))
        h0d, h0o = np.zeros(N), np.ones(max(N - 1, 1))
        F, G = np.empty((C, K)), np.empty((C, K, N + 1))
        head = (N, _p(np.nan_to_num(ctrl)), _p(h0d), _p(h0o), _p(draws), ctypes.c_longlong(K * N * 3), ctypes.c_longlong(C),
                ctypes.c_longlong(K), a, b, self.force_general)
        if grid is None:
            rc = self.lib.rc_host_chain_fidelity_grad(*head, _p(F), _p(G))
        else:
            sc, sh, w = (None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in grid)
            rc = self.lib.rc_host_chain_fidelity_grad_times(*head, len(w), _p(sc), _p(sh), _p(w), _p(F), _p(G))
        assert rc == 0
        nan = np.isnan(ctrl).any(axis=1)              # (the kernel's rule for a padded row; the per-sample arithmetic never sees one)
        F[nan] = np.nan
        G[nan] = np.nan
        res = {"fid": F, "grad": G}
        res["mean"], res["moment"] = gt.host_means(res), gt.host_moments(res)
        return {k: v for k, v in res.items() if k in want}

    def mc_fidelity_grad_philox(self, ctrl, K, N, a, b, seed, offset=0, sigma=0.05, shared=False, h0_diag=None, h0_offdiag=None,
                                want=gt.OUTPUTS):
        return self._run(ctrl, K, N, a, b, seed, offset, sigma, shared, None, want)

    def mc_fidelity_grad_times_philox(self, ctrl, K, N, a, b, seed, offset=0, sigma=0.05, shared=False, tscale=None, tshift=None,
                                      weights=None, h0_diag=None, h0_offdiag=None, want=gt.OUTPUTS):
        return self._run(ctrl, K, N, a, b, seed, offset, sigma, shared, (tscale, tshift, weights), want)


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    out = tmp_path_factory.mktemp("hostgradtimes") / "librc_hostgradtimes.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                    os.path.join(ROOT, "tests", "host", "host_grad_times.cpp")], check=True)
    return ctypes.CDLL(str(out))


@pytest.fixture(params=[0, 1], ids=["kernel-order", "textbook-forced"])
def host(request, hostlib):
    return HostBackend(hostlib, request.param)


@pytest.mark.parametrize("N", range(2, 13))
def test_reference_and_bits(host, N):
    """inside the bars of grad_eigh per grid time (with the teeth guards where the pair has them), and the bits of the
    single-time arithmetic per u_j combined by the exact fma sequence"""
    worst = gc.Worst()
    for (a, b) in gt.pairs(N):
        gt.check_reference(host, N, a, b, K=20, worst=worst, guard=False)
        gt.check_bits_against_single_time(host, N, a, b, K=20)
    print("host gradient on the grid:", worst)


@pytest.mark.parametrize("N", range(2, 13))
def test_unit_grid_gives_the_single_time_bits(host, N):
    gt.check_unit_grid(host, N, 0, N - 1, K=10)


@pytest.mark.parametrize("N", range(2, 13))
def test_negative_u_zero_u_and_the_largest_grid(host, N):
    """u < 0 flips only the time entry's sign; u = 0 exactly (tscale = tshift = 0) gives F = [in == out], gradient 0 and time
    entry 0; M = 64"""
    gt.check_semantics(host, N, K=6)
