"""`MCDataSim.get_sensitivity_dict` around a NumPy stand-in for `backend.mc_fidelity_sens_philox` - runs without a GPU.  The
stand-in regenerates the stream elements the entry documents (oracle/philox_host.py: row c, draw k, site i, slot s is element
offset + ((c K + k) N + i) 3 + s, scaled by the row's sigma) and differentiates with sens_checks.sens_eigh; what is under
test is everything around the kernel: the tiling of the controller rows over the levels, the offsets, the NaN padding, the
cache policy and that no other random stream is touched."""
import importlib
import json
import os

import numpy as np
import pytest

import sens_checks as sc
from oracle import philox_host

mcmod = importlib.import_module("code-robchar_amd.mc_data_sim")
noise = importlib.import_module("code-robchar_amd.noise")
be = importlib.import_module("code-robchar_amd.backend")

N, A, B, C, K, SEED = 4, 0, 3, 4, 16, 77
NOISES = np.array([0.0, 0.05, 0.1])
TN = 0.05


class StandIn:
    """`backend.mc_fidelity_sens_philox` on the CPU; counts its calls"""

    def __init__(self):
        self.calls = []

    def __call__(self, controllers, n_draws, nspin, inspin, outspin, seed, offset=0, sigma=0.05, h0_diag=None, h0_offdiag=None,
                 want=("fid", "sens", "mean")):
        ctrl = np.asarray(controllers, dtype=np.float64)
        rows = ctrl.shape[0]
        sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (rows,))
        self.calls.append(dict(rows=rows, K=n_draws, seed=seed, offset=offset, sigma=sig.copy()))
        z = philox_host.philox_normal(seed, offset, rows * n_draws * nspin * 3, 1.0).reshape(rows, n_draws, nspin, 3)
        draws = sig[:, None, None, None] * z
        F, S = sc.sens_eigh(ctrl, draws, nspin, inspin, outspin, h0_diag, h0_offdiag)
        res = {"fid": F, "sens": S, "mean": sc.mean_of(F, draws, S)}
        return {k: res[k] for k in want}


def controllers(rng):
    """three real rows per algorithm (delocalised: the sensitivities are of order 0.1 - 1), the fourth slot stays empty"""
    def rows(n):
        x = np.empty((n, N + 1))
        x[:, :N] = rng.uniform(-0.5, 0.5, (n, N))
        x[:, N] = rng.uniform(0.5 * N, 0.7 * N, n)
        return x.tolist()
    return {"ppo": {str(TN): {"controller": rows(3)}}, "lbfgs": {str(N): {"controller": rows(3)}}}


@pytest.fixture
def sim(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    os.makedirs("experiments/sens")
    le = controllers(np.random.default_rng(3))
    json.dump(le, open(f"experiments/sens/ppo_spin_{N}_{A}-{B}_c_{C}.le", "w"))
    stand = StandIn()
    monkeypatch.setattr(be, "mc_fidelity_sens_philox", stand)
    s = mcmod.MCDataSim(experiment_name="sens", Nspin=N, inspin=A, outspin=B, noises=NOISES, bootreps=5, training_noise=TN,
                        numcontrollers=C, filemarker=".le", verbose=False, seed=SEED)
    s.stand, s.le = stand, le
    return s


def same_table(x, y):
    """equality of two results, NaN padding included"""
    return list(x) == list(y) and all(
        list(x[a]) == list(y[a]) and all(np.array_equal(np.array(x[a][k], dtype=np.float64), np.array(y[a][k], dtype=np.float64),
                                                        equal_nan=True) for k in x[a]) for a in x)


def level_reference(ctrl, j, sigma, nvalid, samples=K, seed=SEED):
    """level j of an algorithm on its own: its elements start at j * nvalid * K * 3 N"""
    off = j * nvalid * samples * N * 3
    draws = sigma * philox_host.philox_normal(seed, off, nvalid * samples * N * 3, 1.0).reshape(nvalid, samples, N, 3)
    F, S = sc.sens_eigh(ctrl, draws, N, A, B)
    return sc.mean_of(F, draws, S)


def test_table_against_the_level_by_level_reference(sim):
    state, off0 = np.random.get_state(), sim._philox_offset
    table = sim.get_sensitivity_dict(samples=K)
    assert sim._philox_offset == off0
    assert all(np.array_equal(x, y) for x, y in zip(state, np.random.get_state()))
    assert list(table) == ["ppo", "lbfgs"]
    assert len(sim.stand.calls) == 2 and all(c["rows"] == 3 * 3 and c["offset"] == 0 and c["K"] == K for c in sim.stand.calls)
    assert np.array_equal(sim.stand.calls[0]["sigma"], np.repeat(NOISES, 3))            # one launch per algorithm, a sigma per row
    for algo, key in (("ppo", str(TN)), ("lbfgs", str(N))):
        t = table[algo]
        assert all(isinstance(t[k], list) for k in ("noises", "fav", "dfav_dlogsigma", "direction"))
        fav, slope, direction = (np.array(t[k], dtype=np.float64) for k in ("fav", "dfav_dlogsigma", "direction"))
        assert t["noises"] == NOISES.tolist()
        assert fav.shape == (3, C) and slope.shape == (3, C) and direction.shape == (3, C, N, 3)
        ctrl = np.array(sim.le[algo][key]["controller"])
        for j, sigma in enumerate(NOISES):
            want = level_reference(ctrl, j, sigma, 3)
            assert np.array_equal(fav[j, :3], want[:, 0]), (algo, j)
            assert np.array_equal(slope[j, :3], want[:, 1]), (algo, j)
            assert np.array_equal(direction[j, :3], want[:, 2:].reshape(3, N, 3)), (algo, j)
        assert np.abs(slope[1:, :3]).max() > 1e-3 and np.abs(direction[:, :3, :, :2]).max() > 1e-2      # teeth
        # sigma = 0: slope exactly 0, direction = the nominal sensitivity's reference
        assert (slope[0, :3] == 0.0).all()
        # (inside the reference's own bars, not bit for bit: the stand-in's zero draws are 0 * z = +-0, and eigh of a matrix with
        # -0 imaginary parts may pick other eigenvector phases than eigh of the real one)
        zero = np.zeros((3, 1, N, 3))
        _, S0 = sc.sens_eigh(ctrl, zero, N, A, B)
        sc.compare_sens(direction[0, :3], S0[:, 0], sc.sens_bars(ctrl, zero, N)[0][:, 0], (algo, "nominal"))
        # the padded controller
        assert np.isnan(fav[:, 3]).all() and np.isnan(slope[:, 3]).all() and np.isnan(direction[:, 3]).all()
        assert not np.isnan(fav[:, :3]).any() and not np.isnan(direction[:, :3]).any()


def test_cache_policy(sim):
    first = sim.get_sensitivity_dict(samples=K)
    path = sim.get_mcname(TN, NOISES) + "s"
    assert os.path.exists(path)
    stored = json.load(open(path))
    assert stored["samples"] == K and stored["seed"] == SEED
    ncalls = len(sim.stand.calls)
    assert same_table(sim.get_sensitivity_dict(samples=K), first) and len(sim.stand.calls) == ncalls        # served from the file
    assert same_table(sim.get_sensitivity_dict(samples=K, algoname="lbfgs"), {"lbfgs": first["lbfgs"]}) and len(sim.stand.calls) == ncalls
    other = sim.get_sensitivity_dict(samples=K, seed=SEED + 1)                                   # another seed recomputes
    assert len(sim.stand.calls) == 2 * ncalls and sim.stand.calls[-1]["seed"] == SEED + 1
    assert other["ppo"]["fav"][1][:3] != first["ppo"]["fav"][1][:3] and other["ppo"]["fav"][0][:3] == first["ppo"]["fav"][0][:3]
    sim.get_sensitivity_dict(samples=K + 1)                                                      # another K too
    assert len(sim.stand.calls) == 3 * ncalls and sim.stand.calls[-1]["K"] == K + 1
    assert json.load(open(path))["samples"] == K + 1
    # cache_format="none": nothing is written
    os.remove(path)
    sim.cache_format = "none"
    sim.get_sensitivity_dict(samples=K)
    assert not os.path.exists(path)


def test_default_samples_and_split_by_level(sim, monkeypatch):
    """K defaults to bootreps; a launch that would exceed the tile limit is split by level, with each part's offset"""
    whole = sim.get_sensitivity_dict(algoname="ppo")
    assert sim.stand.calls[-1]["K"] == sim.bootreps
    os.remove(sim.get_mcname(TN, NOISES) + "s")
    monkeypatch.setattr(mcmod.MCDataSim, "_SENS_MAX_TILES", 2 * 3)                # two levels of three rows (one tile each)
    n0 = len(sim.stand.calls)
    parts = sim.get_sensitivity_dict(algoname="ppo")
    calls = sim.stand.calls[n0:]
    assert [c["rows"] for c in calls] == [6, 3] and [c["offset"] for c in calls] == [0, 2 * 3 * sim.bootreps * N * 3]
    assert same_table(parts, whole)


def test_unsupported_configurations(sim, monkeypatch):
    sim.noise_model = noise.structured_perturbation(Nspin=N, inspin=A, outspin=B, topo="ring")
    with pytest.raises(NotImplementedError):
        sim.get_sensitivity_dict(samples=K)
    sim.noise_model = noise.structured_perturbation(Nspin=N, inspin=A, outspin=B)
    sim.devices = [0]
    with pytest.raises(NotImplementedError, match="one GPU"):
        sim.get_sensitivity_dict(samples=K)
    sim.devices = None
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError, match="process group"):
        sim.get_sensitivity_dict(samples=K)
    assert not sim.stand.calls
