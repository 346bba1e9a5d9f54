"""Placement test of `backend.mc_fidelity_grad_times_philox` with tests/arena.py, on the protocol of tests/test_gpu_placement.py:
the controllers, the per-row sigma, the three grid arrays and all four outputs sit inside guarded arenas, the float64 bodies at 0
and at 8 mod 16 bytes, the guards around the inputs poisoned with a NaN sentinel or with 1e300.  After the call no guard word has
changed, no output element is left unwritten, and every output has the bits of the plain call - which is first held against the
independent reference of grad_times_checks.py."""
import numpy as np
import pytest

import grad_checks as gc
import grad_times_checks as gt
from arena import FILLS, Arena

pytestmark = pytest.mark.gpu
COMBOS = [(shift, fill) for shift in (0, 1) for fill in FILLS]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("N", (7, 12))
def test_mc_fidelity_grad_times_philox(be, N):
    import torch
    dev = be.compute_device()
    K, offset = 65, 7                                                    # a one-sample tail behind a full tile
    ctrl = gc.philox_ctrl(N)                                             # C = 3: row 1 NaN, row 2 with a negative time entry
    sig = np.array([0.05, 0.03, 0.08])
    for shared in (False, True):
        tag = ("grad times philox", N, "shared" if shared else "per row")

        def call(ctrl_t, sigma_t):
            return be.mc_fidelity_grad_times_philox(ctrl_t, K, N, 0, N - 1, gt.SEED, offset=offset, sigma=sigma_t, shared=shared,
                                                    tscale=gt.TSCALE, tshift=gt.TSHIFT, weights=gt.WEIGHTS)
        plain = gc.to_host(call(torch.from_numpy(ctrl).to(dev), torch.from_numpy(sig).to(dev)))
        draws = gt.draws_of(ctrl, K, N, offset, shared, sig)
        W, G, bars, _, _ = gt.reference(ctrl, draws, N, 0, N - 1, gt.TSCALE, gt.TSHIFT, gt.WEIGHTS)
        assert np.abs(np.nan_to_num(plain["fid"] - W)).max() < gc.TOL and np.isnan(plain["fid"][1]).all(), tag
        gc.compare_grad(plain["grad"], G, bars, tag)
        for shift, fill in COMBOS:
            ar = Arena(shift=shift, device=dev)
            where = (tag, "shift", shift, "poison", fill)
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(torch, "empty", ar.empty)
                # the grid's device copy: one guarded block per array instead of the cached (3, M) tensor
                mp.setattr(be, "_times_grid_on_device", lambda a, b, w, d: [ar.place(a, fill), ar.place(b, fill), ar.place(w, fill)])
                res = call(ar.place(ctrl, fill), ar.place(sig, fill))
            assert sum(" empty " in b.name for b in ar.blocks) == 4 and sum(" place" in b.name for b in ar.blocks) == 5, where
            try:
                ar.check_guards()
                for k, t in res.items():
                    ar.assert_written(t, k)
            except AssertionError as e:
                raise AssertionError(f"{where}: {e}") from None
            got = gc.to_host(res)
            assert sorted(got) == sorted(plain) == sorted(gt.OUTPUTS)
            for k in got:
                assert got[k].shape == plain[k].shape and np.array_equal(bits(got[k]), bits(plain[k])), (
                    where, k, "depends on where its tensors sit")
