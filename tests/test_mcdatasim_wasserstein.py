"""`MCDataSim.get_wasserstein_dict` around NumPy stand-ins for `backend.sort_rows` and `backend.wasserstein_matrix` (built on
`wasserstein.matrix_reference`) - runs without a GPU.  What is under test is everything around the kernel: one sort per algorithm
over the L * C rows, one launch per level, shapes, the NaN padding, the cache policy and the unsupported configurations."""
import importlib
import json
import os

import numpy as np
import pytest

import test_mcdatasim_sensitivity as ms
import wasserstein_checks as wc

mcmod = importlib.import_module("code-robchar_amd.mc_data_sim")
be = importlib.import_module("code-robchar_amd.backend")

K = 24
L, C = len(ms.NOISES), ms.C


class StandIn:
    def __init__(self):
        self.sorts, self.launches = [], []

    def sort_rows(self, fid, device=None):
        self.sorts.append(tuple(fid.shape))
        return np.sort(np.asarray(fid, dtype=np.float64), axis=1)

    def wasserstein_matrix(self, a, b=None, p=1, assume_sorted=False, device=None, out=None):
        assert assume_sorted and b is None
        a = np.asarray(a)
        fin = a[~np.isnan(a).any(axis=1)]
        assert np.all(np.diff(fin, axis=1) >= 0)                     # the rows arrive sorted
        self.launches.append((tuple(a.shape), p))
        return wc.wd.matrix_reference(a, None, p)


def fidelities(seed):
    """(L, C, K) per algorithm: three real controllers, the fourth padded with NaN; the distributions widen with the level"""
    rng = np.random.default_rng(seed)
    out = {}
    for n, name in enumerate(("ppo", "lbfgs")):
        F = np.full((L, C, K), np.nan)
        for j in range(L):
            for c in range(3):
                F[j, c] = rng.beta(5.0 - c, 1.5 + 0.5 * j + n, K)
        out[name] = F
    return out


@pytest.fixture
def sim(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    os.makedirs("experiments/sens")
    json.dump(ms.controllers(np.random.default_rng(3)), open(f"experiments/sens/ppo_spin_{ms.N}_{ms.A}-{ms.B}_c_{C}.le", "w"))
    stand = StandIn()
    monkeypatch.setattr(be, "sort_rows", stand.sort_rows)
    monkeypatch.setattr(be, "wasserstein_matrix", stand.wasserstein_matrix)
    s = mcmod.MCDataSim(experiment_name="sens", Nspin=ms.N, inspin=ms.A, outspin=ms.B, noises=ms.NOISES, bootreps=K, training_noise=ms.TN,
                        numcontrollers=C, filemarker=".le", verbose=False, seed=ms.SEED)
    s.stand, s.fids, s.fid_calls = stand, fidelities(5), []
    monkeypatch.setattr(s, "get_fid_dists", lambda *a, **k: (s.fid_calls.append(a), s.fids)[1])
    return s


def same(x, y):
    return list(x) == list(y) and all(np.array_equal(x[a], y[a], equal_nan=True) for a in x)


@pytest.mark.parametrize("p", (1, 2))
def test_table_shapes_padding_and_values(sim, p):
    table = sim.get_wasserstein_dict(p=p)
    assert list(table) == ["ppo", "lbfgs"]
    assert sim.stand.sorts == [(L * C, K)] * 2                        # one sort per algorithm over the L * C rows
    assert sim.stand.launches == [((C, K), p)] * (2 * L)              # then one launch per level
    for name, W in table.items():
        assert isinstance(W, np.ndarray) and W.shape == (L, C, C) and W.dtype == np.float64
        assert np.isnan(W[:, 3, :]).all() and np.isnan(W[:, :, 3]).all() and np.isfinite(W[:, :3, :3]).all()     # the padded controller
        for j in range(L):
            want = wc.wd.matrix_reference(sim.fids[name][j, :3], None, p)
            assert np.median(wc.off_diagonal(want, True)) >= 1e-2
            assert np.array_equal(W[j, :3, :3], want)
            assert np.array_equal(W[j, :3, :3], W[j, :3, :3].T) and np.all(np.diag(W[j])[:3] == 0)
    one = sim.get_wasserstein_dict(algoname="lbfgs", p=p)
    assert list(one) == ["lbfgs"] and np.array_equal(one["lbfgs"], table["lbfgs"], equal_nan=True)


def test_cache_reuse_and_refusal(sim):
    path = sim.get_mcname(ms.TN, ms.NOISES) + "w"
    table = sim.get_wasserstein_dict(p=1)
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    with np.load(path) as z:
        assert int(z["p"]) == 1 and sorted(z.files) == ["algo:lbfgs", "algo:ppo", "p"] and z["algo:ppo"].shape == (L, C, C)
    n = len(sim.stand.launches)
    assert same(sim.get_wasserstein_dict(p=1), table) and len(sim.stand.launches) == n and len(sim.fid_calls) == 1     # served from the file
    assert same(sim.get_wasserstein_dict(p=1, algoname="ppo"), {"ppo": table["ppo"]}) and len(sim.stand.launches) == n
    other = sim.get_wasserstein_dict(p=2)                             # another p: the file is refused, recomputed and replaced
    assert len(sim.stand.launches) == n + 2 * L and not same(other, table)
    with np.load(path) as z:
        assert int(z["p"]) == 2
    sim.get_wasserstein_dict(p=1)
    assert len(sim.stand.launches) == n + 4 * L
    # another shape: a file of a run with more controllers is not reused
    with open(path, "wb") as fh:
        np.savez(fh, p=np.int64(1), **{"algo:ppo": np.zeros((L, C + 1, C + 1)), "algo:lbfgs": table["lbfgs"]})
    again = sim.get_wasserstein_dict(p=1)
    assert len(sim.stand.launches) == n + 5 * L and same(again, table)
    with pytest.raises(ValueError, match="p must be 1 or 2"):
        sim.get_wasserstein_dict(p=3)


def test_cache_format_none_writes_nothing(sim):
    sim.cache_format = "none"
    table = sim.get_wasserstein_dict()
    assert table["ppo"].shape == (L, C, C) and not os.path.exists(sim.get_mcname(ms.TN, ms.NOISES) + "w")
    sim.get_wasserstein_dict()
    assert len(sim.stand.launches) == 4 * L                           # nothing to reuse


def test_unsupported_configurations(sim, monkeypatch):
    sim.devices = [0]
    with pytest.raises(NotImplementedError, match="one GPU"):
        sim.get_wasserstein_dict()
    sim.devices = None
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError, match="process group"):
        sim.get_wasserstein_dict()
    assert not hasattr(sim, "get_wd_data_c")
