"""Placement of the pick-freeze entry (rc_mc_fidelity_pickfreeze_philox_f64_async) inside guarded arenas (tests/arena.py, the
procedure of tests/test_gpu_placement.py): the controllers, the per-row scales and both outputs at 0 and at 8 mod 16 bytes, no
guard word changed, no output element left unwritten - tail tiles and the NaN row included -, and the bits those of the plain
call."""
import numpy as np
import pytest

import grad_checks as gc
import variance_checks as vc
from test_gpu_placement import placement, plain_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(be):
    import torch
    return torch.device("cuda", torch.cuda.current_device())


@pytest.mark.parametrize("N,K", ((2, 1), (7, 130), (10, 65), (13, 63)))
def test_mc_fidelity_pickfreeze_philox(be, dev, N, K):
    ctrl = gc.philox_ctrl(N)
    masks, *_ = vc.groups_under_test(N)
    inputs = dict(controllers=ctrl, sigma=np.array([0.05, 0.05, 0.0]))

    def call(arena, controllers, sigma):
        return be.mc_fidelity_pickfreeze_philox(controllers, K, N, 0, N - 1, vc.SEED, masks, offset=9, sigma=sigma, want=("fid", "mean"))

    plain = plain_call(dev, call, inputs)
    assert np.isnan(plain["fid"][:, 1]).all() and np.isnan(plain["mean"][1]).all() and np.nanmax(plain["fid"]) > 1e-3
    assert not np.isnan(plain["fid"][:, [0, 2]]).any() and not np.isnan(plain["mean"][[0, 2]]).any()
    placement(dev, call, inputs, plain, ("mc_fidelity_pickfreeze_philox", N, K))
