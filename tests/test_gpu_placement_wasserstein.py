"""Placement test of `backend.wasserstein_matrix` with tests/arena.py, on the protocol of tests/test_gpu_placement.py: the two
inputs and the output sit inside guarded arenas, the float64 bodies at 0 and at 8 mod 16 bytes, the guards around the inputs
poisoned with a NaN sentinel or with 1e300.  After the call no guard word has changed, no output element is left unwritten, and
the output has the bits of the plain call - which is first held against the fsum reference.  Shapes: partial tiles on both sides
of more than one tile; K below a chunk (the tile kernel writes the result) and above (partial sums and the finishing pass)."""
import numpy as np
import pytest

import wasserstein_checks as wc
from arena import FILLS, Arena

pytestmark = pytest.mark.gpu
COMBOS = [(shift, fill) for shift in (0, 1) for fill in FILLS]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("K", (100, wc.CHUNK + 45), ids=("direct", "split"))
@pytest.mark.parametrize("symmetric", (False, True), ids=("general", "symmetric"))
def test_wasserstein_matrix(be, K, symmetric):
    import torch
    dev = be.compute_device()
    A = np.sort(wc.beta_rows(wc.TILE + 6, K, 141) * np.linspace(0.3, 1.0, wc.TILE + 6)[:, None], axis=1)    # rows of different spread
    B = None if symmetric else np.sort(wc.beta_rows(5, K, 142, (2.0, 2.0)), axis=1)
    up = lambda x: None if x is None else torch.from_numpy(x).to(dev)
    for p in (1, 2):
        tag = ("wasserstein", "symmetric" if symmetric else "general", K, p)
        plain = be.wasserstein_matrix(up(A), up(B), p=p, assume_sorted=True).cpu().numpy()
        want = wc.reference(("placement", symmetric, K, p), A, B, p)
        assert np.median(wc.off_diagonal(want, symmetric)) >= 1e-2
        wc.assert_within_bar(plain, want, K, str(tag))
        for shift, fill in COMBOS:
            ar = Arena(shift=shift, device=dev)
            where = (tag, "shift", shift, "poison", fill)
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(torch, "empty", ar.empty)
                res = be.wasserstein_matrix(ar.place(A, fill), None if symmetric else ar.place(B, fill), p=p, assume_sorted=True)
            assert sum(" empty " in b.name for b in ar.blocks) == 1 and sum(" place" in b.name for b in ar.blocks) == (1 if symmetric else 2), where
            try:
                ar.check_guards()
                ar.assert_written(res, "out")
            except AssertionError as e:
                raise AssertionError(f"{where}: {e}") from None
            got = res.cpu().numpy()
            assert got.shape == plain.shape and np.array_equal(bits(got), bits(plain)), (where, "depends on where its tensors sit")
