"""`MCDataSim.get_variance_dict` around the NumPy stand-in for `backend.mc_fidelity_pickfreeze_philox` (tests/variance_checks.py) -
runs without a GPU.  Under test is everything around the kernel: the tiling of the controller rows over the levels and the
replicates, the two stream blocks, the NaN padding, the sigma = 0 level, the cache policy, the one-GPU refusals, and that no
other random stream is touched."""
import importlib
import json
import os

import numpy as np
import pytest

import variance_checks as vc

mcmod = importlib.import_module("code-robchar_amd.mc_data_sim")
noise = importlib.import_module("code-robchar_amd.noise")
be = importlib.import_module("code-robchar_amd.backend")
vi = importlib.import_module("code-robchar_amd.variance_indices")

N, A, B, C, K, SEED = 4, 0, 3, 4, 48, 77
NOISES = np.array([0.0, 0.05, 0.1])
TN = 0.05


class Counting(vc.StandIn):
    def __init__(self):
        super().__init__()
        self.calls = []

    def __call__(self, controllers, n_draws, nspin, inspin, outspin, seed, groups, **kw):
        self.calls.append(dict(rows=np.asarray(controllers).shape[0], K=n_draws, seed=seed, groups=np.array(groups), **kw))
        return self.mc_fidelity_pickfreeze_philox(controllers, n_draws, nspin, inspin, outspin, seed, groups, **kw)


def controllers(rng):
    """three real rows per algorithm (delocalised), the fourth slot stays empty"""
    def rows(n):
        x = np.empty((n, N + 1))
        x[:, :N] = rng.uniform(-0.5, 0.5, (n, N))
        x[:, N] = rng.uniform(0.5 * N, 0.7 * N, n)
        return x.tolist()
    return {"ppo": {str(TN): {"controller": rows(3)}}, "lbfgs": {str(N): {"controller": rows(3)}}}


@pytest.fixture
def sim(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    os.makedirs("experiments/var")
    le = controllers(np.random.default_rng(3))
    json.dump(le, open(f"experiments/var/ppo_spin_{N}_{A}-{B}_c_{C}.le", "w"))
    stand = Counting()
    monkeypatch.setattr(be, "mc_fidelity_pickfreeze_philox", stand)
    s = mcmod.MCDataSim(experiment_name="var", Nspin=N, inspin=A, outspin=B, noises=NOISES, bootreps=5, training_noise=TN,
                        numcontrollers=C, filemarker=".le", verbose=False, seed=SEED)
    s.stand, s.le = stand, le
    return s


def same_table(x, y):
    def eq(u, v):
        return u == v if isinstance(u[0] if u else "", str) else np.array_equal(np.array(u, dtype=np.float64), np.array(v, dtype=np.float64),
                                                                                equal_nan=True)
    return list(x) == list(y) and all(list(x[a]) == list(y[a]) and all(eq(x[a][k], y[a][k]) for k in x[a]) for a in x)


def test_table_layout_padding_and_the_definition(sim):
    state, off0 = np.random.get_state(), sim._philox_offset
    table = sim.get_variance_dict(samples=K)
    assert sim._philox_offset == off0 and all(np.array_equal(x, y) for x, y in zip(state, np.random.get_state()))
    assert list(table) == ["ppo", "lbfgs"]
    masks, labels = vi.kind_groups(N)
    block = 3 * 3 * K * 3 * N                                                    # L C' K 3N: b lies one block behind a
    assert len(sim.stand.calls) == 2                                              # one launch per algorithm
    for c in sim.stand.calls:
        assert c["rows"] == 9 and c["K"] == K and c["seed"] == SEED and c["offset"] == 0 and c["offset_b"] == block
        assert np.array_equal(c["sigma"], np.repeat(NOISES, 3)) and np.array_equal(c["groups"], masks) and c["want"] == ("mean",)
    for algo, key in (("ppo", str(TN)), ("lbfgs", str(N))):
        t = table[algo]
        assert t["noises"] == NOISES.tolist() and t["groups"] == labels and "first_se" not in t
        fav, var, first, total = (np.array(t[k], dtype=np.float64) for k in ("fav", "var", "first", "total"))
        assert fav.shape == var.shape == (3, C) and first.shape == total.shape == (3, C, 3)
        ctrl = np.array(sim.le[algo][key]["controller"])
        for j, sigma in enumerate(NOISES):                                       # level j on its own, from the definition
            mean = vc.reference(ctrl, K, N, A, B, masks, j * 3 * K * 3 * N, block + j * 3 * K * 3 * N, sigma=float(sigma), seed=SEED)[1]
            want = vi.indices_from_means(mean)
            for k, got in (("fav", fav), ("var", var), ("first", first), ("total", total)):
                assert np.array_equal(got[j, :3], want[k], equal_nan=True), (algo, j, k)
        # sigma = 0: no variance, NaN indices; the padded controller: NaN everywhere
        assert (var[0, :3] == 0.0).all() and np.isnan(first[0]).all() and np.isnan(total[0]).all() and not np.isnan(fav[0, :3]).any()
        assert np.isnan(fav[:, 3]).all() and np.isnan(var[:, 3]).all() and np.isnan(first[:, 3]).all() and np.isnan(total[:, 3]).all()
        assert not np.isnan(first[1:, :3]).any() and (var[1:, :3] > 0).all() and (total[1:, :3] >= 0).all()
        assert total[1:, :3].max() > 0.3                                          # teeth: some group carries the variance


def test_replicates_and_groups(sim):
    R = 3
    table = sim.get_variance_dict(samples=K, groups="site", replicates=R, algoname="ppo")
    c = sim.stand.calls[-1]
    assert c["rows"] == R * 9 and c["offset_b"] == R * 9 * K * 3 * N and np.array_equal(c["sigma"], np.tile(np.repeat(NOISES, 3), R))
    t = table["ppo"]
    assert t["groups"] == [f"site_{i}" for i in range(N)] and np.array(t["first_se"]).shape == (3, C, N)
    assert np.array(t["var_se"]).shape == (3, C)
    # replicate r, level j on their own, from the definition
    masks, _ = vi.site_groups(N)
    ctrl = np.array(sim.le["ppo"][str(TN)]["controller"])
    per = 3 * K * 3 * N
    idx = [vi.indices_from_means(vc.reference(ctrl, K, N, A, B, masks, (r * 3 + 1) * per, (R * 3 + r * 3 + 1) * per, sigma=0.05,
                                              seed=SEED)[1]) for r in range(R)]
    for k in ("var", "first", "total"):
        m, se = vi.over_replicates(np.stack([i[k] for i in idx]))
        assert np.array_equal(np.array(t[k])[1, :3], m) and np.array_equal(np.array(t[k + "_se"])[1, :3], se), k
    masks_in = sim.get_variance_dict(samples=K, groups=[0b1, 0b1000000], algoname="ppo")["ppo"]
    assert masks_in["groups"] == ["0x1", "0x40"]


def test_cache_policy(sim):
    first = sim.get_variance_dict(samples=K)
    path = sim.get_mcname(TN, NOISES) + "v"
    assert os.path.exists(path)
    stored = json.load(open(path))
    assert stored["samples"] == K and stored["seed"] == SEED and stored["replicates"] == 1 and len(stored["masks"]) == 3
    ncalls = len(sim.stand.calls)
    assert same_table(sim.get_variance_dict(samples=K), first) and len(sim.stand.calls) == ncalls              # served from the file
    assert same_table(sim.get_variance_dict(samples=K, algoname="lbfgs"), {"lbfgs": first["lbfgs"]}) and len(sim.stand.calls) == ncalls
    for kw in (dict(seed=SEED + 1), dict(samples=K + 1), dict(groups="site"), dict(replicates=2)):             # any mismatch recomputes
        n0 = len(sim.stand.calls)
        sim.get_variance_dict(**{"samples": K, **kw})
        assert len(sim.stand.calls) == n0 + 2, kw
    assert json.load(open(path))["replicates"] == 2
    os.remove(path)
    sim.cache_format = "none"
    sim.get_variance_dict(samples=K)
    assert not os.path.exists(path)
    assert sim.get_variance_dict(algoname="ppo") and sim.stand.calls[-1]["K"] == sim.bootreps                  # K defaults to bootreps


def test_unsupported_configurations(sim, monkeypatch):
    sim.noise_model = noise.structured_perturbation(Nspin=N, inspin=A, outspin=B, topo="ring")
    with pytest.raises(NotImplementedError):
        sim.get_variance_dict(samples=K)
    sim.noise_model = noise.structured_perturbation(Nspin=N, inspin=A, outspin=B)
    with pytest.raises(ValueError):
        sim.get_variance_dict(samples=K, replicates=0)
    sim.devices = [0]
    with pytest.raises(NotImplementedError, match="one GPU"):
        sim.get_variance_dict(samples=K)
    sim.devices = None
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError, match="process group"):
        sim.get_variance_dict(samples=K)
    assert not sim.stand.calls
