"""Placement of the two Sobol device entries (rc_draws_sobol_f64_async, rc_mc_fidelity_sobol_f64_async) inside guarded arenas
(tests/arena.py, the procedure of tests/test_gpu_placement.py): every input and output at 0 and at 8 mod 16 bytes - the uint32
tables, carried as int32 tensors, at 0 and at 4 mod 8 -, no guard word changed, no output element left unwritten, and the bits
those of the plain call."""
import importlib

import numpy as np
import pytest

import chain_checks as cc
from test_gpu_placement import placement, plain_call

pytestmark = pytest.mark.gpu
sobol = importlib.import_module("code-robchar_amd.sobol")


@pytest.fixture(scope="module")
def dev(be):
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def tables(D, R, C, seed):
    dirnum, shift = sobol.scramble(D, R, seed, C=C)
    return dirnum.view(np.int32), shift.view(np.int32)


@pytest.mark.parametrize("D,R,P,K,skip", ((21, 3, 64, 192, 320), (96, 1, 100, 100, 0), (6, 2, 128, 130, 2 ** 32 - 128)))
def test_sobol_generator(be, dev, D, R, P, K, skip):
    C = 3
    dirnum, shift = tables(D, R, C, seed=D)
    inputs = dict(dirnum=dirnum, shift=shift, sigma=np.array([0.05, 0.0, 0.3]))

    def call(arena, dirnum, shift, sigma):
        return be._sobol_generate(("draws", "bits"), dirnum, shift, P, K, skip, sigma, C, dev, True)

    plain = plain_call(dev, call, inputs)
    assert np.array_equal(plain["bits"].view(np.uint32), sobol.points(dirnum.view(np.uint32), shift.view(np.uint32), P, K, skip))
    placement(dev, call, inputs, plain, ("sobol generator", D, R, P, K, skip))


@pytest.mark.parametrize("N", (2, 7, 13))
def test_mc_fidelity_sobol(be, dev, N):
    C, R, P, K, skip = 3, 2, 128, 130, 64
    rng = np.random.default_rng(8800 + N)
    ctrl = cc.deloc_ctrl(rng, C, N, 0.5)
    ctrl[1, N // 2] = np.nan
    dirnum, shift = tables(3 * N, R, C, seed=N)
    inputs = dict(controllers=ctrl, dirnum=dirnum, shift=shift, sigma=np.array([0.05, 0.05, 0.0]))

    def call(arena, controllers, dirnum, shift, sigma, out=False):
        import torch
        o = torch.empty((C, K), dtype=torch.float64, device=dev) if out else None
        return be.mc_fidelity_sobol(controllers, K, N, 0, N - 1, dirnum, shift, P, skip=skip, sigma=sigma, out=o)

    plain = plain_call(dev, call, inputs)
    assert np.isnan(plain["out"][1]).all() and np.nanmax(plain["out"]) > 1e-3
    placement(dev, call, inputs, plain, ("mc_fidelity_sobol", N), outs=(False, True))
