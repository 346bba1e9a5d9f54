"""`MCDataSim.get_qmc_dict` around a NumPy stand-in for `backend.mc_fidelity_sobol` (sobol.py's normals + the oracle) and the oracle
stand-in for `backend.reduce_metrics` - runs without a GPU.  What is under test is everything around the kernel: the tiling of the
controller rows over the levels with one sigma per row, the scramble shared by all rows, the replicate statistics, the NaN padding,
the cache policy and that no other random stream is touched."""
import importlib
import json
import os

import numpy as np
import pytest

import stand_in
import times_checks as tc
from oracle import robchar_oracle as orc

mcmod = importlib.import_module("code-robchar_amd.mc_data_sim")
noise = importlib.import_module("code-robchar_amd.noise")
be = importlib.import_module("code-robchar_amd.backend")
sobol = importlib.import_module("code-robchar_amd.sobol")

T = tc.TOY
N, C, SEED, NOISES, TN = T["N"], T["C"], T["SEED"], T["NOISES"], T["TN"]
R, P, L = 4, 64, 2


class Counted:
    def __init__(self):
        self.calls = []

    def __call__(self, controllers, n_draws, nspin, inspin, outspin, dirnum, shift, P, skip=0, sigma=0.05, h0_diag=None, h0_offdiag=None):
        ctrl = np.asarray(controllers)
        rows = ctrl.shape[0]
        sig = np.broadcast_to(sigma, (rows,)).copy()
        self.calls.append(dict(rows=rows, K=n_draws, P=P, sigma=sig, dirnum=dirnum.copy(), shift=shift.copy()))
        draws = sobol.normals(dirnum, shift, P, n_draws, skip, sigma=sig, C=rows).reshape(rows, n_draws, nspin, 3)
        return orc.fidelity_eigh(ctrl, draws, nspin, inspin, outspin, h0_diag=h0_diag, h0_offdiag=h0_offdiag)


@pytest.fixture
def sim(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    le = tc.write_toy_experiment("qmc")
    stand = Counted()
    monkeypatch.setattr(be, "mc_fidelity_sobol", stand)
    monkeypatch.setattr(be, "reduce_metrics", stand_in.reduce_metrics)
    s = mcmod.MCDataSim(experiment_name="qmc", Nspin=N, inspin=T["A"], outspin=T["B"], noises=NOISES, bootreps=5,
                        training_noise=TN, numcontrollers=C, filemarker=".le", verbose=False, seed=SEED)
    s.stand, s.le = stand, le
    return s


def test_table_keys_shapes_padding_and_values(sim):
    state, off0 = np.random.get_state(), sim._philox_offset
    table = sim.get_qmc_dict(replicates=R, points=P)
    assert sim._philox_offset == off0
    assert all(np.array_equal(x, y) for x, y in zip(state, np.random.get_state()))
    assert list(table) == ["ppo", "lbfgs"]
    assert len(sim.stand.calls) == 2 and all(c["rows"] == L * 3 and c["K"] == R * P and c["P"] == P for c in sim.stand.calls)
    assert np.array_equal(sim.stand.calls[0]["sigma"], np.repeat(NOISES, 3))          # one launch per algorithm, a sigma per row
    dirnum, shift = sobol.scramble(3 * N, R, SEED)
    for c in sim.stand.calls:                                                         # the scramble is shared by all rows and algorithms
        assert np.array_equal(c["dirnum"], dirnum) and np.array_equal(c["shift"], shift) and c["shift"].shape[0] == 1
    for algo, key in (("ppo", str(TN)), ("lbfgs", str(N))):
        t = table[algo]
        assert sorted(t) == sorted(("noises", "rim", "rim_se", "std", "std_se", "worst"))
        assert all(isinstance(v, list) for v in t.values()) and t["noises"] == NOISES.tolist()
        tabs = {k: np.array(t[k], dtype=np.float64) for k in ("rim", "rim_se", "std", "std_se", "worst")}
        assert all(v.shape == (L, C) for v in tabs.values())
        assert all(np.isnan(v[:, 3]).all() and not np.isnan(v[:, :3]).any() for v in tabs.values())     # the padded controller
        ctrl = np.array(sim.le[algo][key]["controller"])
        for j, sigma in enumerate(NOISES):
            draws = sobol.normals(dirnum, shift, P, R * P, sigma=float(sigma), C=3).reshape(3, R * P, N, 3)
            fid = orc.fidelity_eigh(ctrl, draws, N, T["A"], T["B"]).reshape(3, R, P)
            rim = 1.0 - fid.mean(axis=2)
            assert np.allclose(tabs["rim"][j, :3], rim.mean(axis=1), rtol=0, atol=1e-14)
            assert np.allclose(tabs["rim_se"][j, :3], rim.std(axis=1, ddof=1) / np.sqrt(R), rtol=0, atol=1e-14)
            sd = fid.std(axis=2)
            assert np.allclose(tabs["std"][j, :3], sd.mean(axis=1), rtol=0, atol=1e-14)
            assert np.allclose(tabs["std_se"][j, :3], sd.std(axis=1, ddof=1) / np.sqrt(R), rtol=0, atol=1e-14)
            assert np.array_equal(tabs["worst"][j, :3], fid.min(axis=(1, 2)))
        assert (tabs["rim_se"][:, :3] > 0).all() and (tabs["rim_se"][:, :3] < 0.2 * tabs["rim"][:, :3]).all()


def same_table(x, y):
    return list(x) == list(y) and all(
        list(x[a]) == list(y[a]) and all(np.array_equal(np.array(x[a][k], dtype=np.float64), np.array(y[a][k], dtype=np.float64),
                                                        equal_nan=True) for k in x[a]) for a in x)


def test_cache_reuse_and_refusal_on_changed_parameters(sim):
    first = sim.get_qmc_dict(replicates=R, points=P)
    path = sim.get_mcname(TN, NOISES) + "q"
    assert os.path.exists(path)
    stored = json.load(open(path))
    assert stored["replicates"] == R and stored["points"] == P and stored["seed"] == SEED
    ncalls = len(sim.stand.calls)
    assert same_table(sim.get_qmc_dict(replicates=R, points=P), first) and len(sim.stand.calls) == ncalls            # served from the file
    assert same_table(sim.get_qmc_dict(replicates=R, points=P, algoname="lbfgs"), {"lbfgs": first["lbfgs"]}) and len(sim.stand.calls) == ncalls
    sim.get_qmc_dict(replicates=R, points=P, seed=SEED + 1)                                                # another seed recomputes
    assert len(sim.stand.calls) == 2 * ncalls
    sim.get_qmc_dict(replicates=R + 1, points=P, seed=SEED + 1)                                            # other replicates too
    assert len(sim.stand.calls) == 3 * ncalls and sim.stand.calls[-1]["K"] == (R + 1) * P
    sim.get_qmc_dict(replicates=R + 1, points=2 * P, seed=SEED + 1)                                        # and other points
    assert len(sim.stand.calls) == 4 * ncalls and json.load(open(path))["points"] == 2 * P
    os.remove(path)
    sim.cache_format = "none"
    sim.get_qmc_dict(replicates=R, points=P)
    assert not os.path.exists(path)


def test_unsupported_configurations(sim, monkeypatch):
    with pytest.raises(ValueError, match="multiple of 64"):
        sim.get_qmc_dict(replicates=R, points=100)
    with pytest.raises(ValueError, match="at least 2"):
        sim.get_qmc_dict(replicates=1, points=P)
    sim.devices = [0]
    with pytest.raises(NotImplementedError, match="one GPU"):
        sim.get_qmc_dict(replicates=R, points=P)
    sim.devices = None
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError, match="process group"):
        sim.get_qmc_dict(replicates=R, points=P)
    assert not sim.stand.calls
