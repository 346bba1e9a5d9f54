"""`backend.bootstrap_metrics` (bootstrap_replicates_kernel + row sort + bootstrap_summary_kernel behind
rc_bootstrap_metrics_f64*) on the device: every check of bootstrap_checks.py - exact known answers from the indices alone, ragged
shapes against fsum references, the counter layout, the two routes, the summary against NumPy, statistics with teeth -, torch
tensors on a side stream, the `rim_metrics` wrapper and `MCDataSim.get_bootstrap_dict`."""
import importlib
import json
import os

import numpy as np
import pytest

import bootstrap_checks as bc

pytestmark = pytest.mark.gpu


# ---- 1. exact known answers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check", (bc.check_exact_permutation_rows, bc.check_constant_row, bc.check_two_valued_row), ids=lambda c: c.__name__)
def test_exact_known_answers(be, check):
    check(be)


# ---- 2. ragged shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", bc.RAGGED_K)
@pytest.mark.parametrize("B", bc.RAGGED_B)
def test_ragged_shapes(be, K, B):
    bc.check_ragged(be, ks=(K,), bs=(B,))


# ---- 3. counter layout ---------------------------------------------------------------------------------------------------------------
def test_rows_are_one_row_calls_and_runs_repeat(be):
    bc.check_rows_are_one_row_calls(be)


def test_far_offsets(be):
    bc.check_far_offsets(be)


# ---- 4. routes -----------------------------------------------------------------------------------------------------------------------
def test_routes_agree_and_lds_cap(be):
    bc.check_routes(be)


def test_a_row_longer_than_the_lds_route_holds(be):
    """auto picks the global route above the cap: K = 18 433, against the fsum reference"""
    K, B = bc.boot.LDS_MAX_K + 1, 3
    F = np.random.default_rng(12).random((1, K))
    rep = be.bootstrap_metrics(F, B, 4, q_thresholds=bc.Q, want=("replicates",))["replicates"]
    f = F[0][bc.boot.indices(1, K, B, 4, 0)[0]]
    import math
    for b in range(B):
        assert rep[2, 0, b] == f[b].min() and rep[3, 0, b] == (f[b] >= bc.Q[0]).sum() / K
        assert abs((1.0 - rep[0, 0, b]) - math.fsum(f[b]) / K) <= K * bc.U


# ---- 5. summary ----------------------------------------------------------------------------------------------------------------------
def test_summary_against_numpy(be):
    bc.check_summary_against_numpy(be)


def test_summary_at_the_largest_replicate_count(be):
    """B = 16 384, the longest row the one-launch sort takes: picks, mean and SE against NumPy on the kernel's own replicates"""
    import math
    B = bc.boot.MAX_N_BOOT
    F = np.random.default_rng(14).random((2, 16))
    res = be.bootstrap_metrics(F, B, 2, q_thresholds=(0.5,), conf=0.9)
    rep, s = res["replicates"], res["summary"]
    lo, hi = bc.boot.ranks(B, 0.9)
    for j in range(4):
        for c in range(2):
            x = rep[j, c]
            srt = np.sort(x)
            assert s[j, 2, c] == srt[lo] and s[j, 3, c] == srt[hi], (j, c)
            assert abs(s[j, 0, c] - math.fsum(x) / B) <= B * bc.U * np.abs(x).max(), (j, c)
            var = math.fsum((x - math.fsum(x) / B) ** 2) / (B - 1)
            assert abs(s[j, 1, c] ** 2 - var) <= 4 * B * bc.U * max(1.0, np.abs(x).max() ** 2), (j, c)


# ---- 6. statistics -------------------------------------------------------------------------------------------------------------------
def test_statistics_with_teeth(be):
    """first the definition's own figures on these inputs, then the device's, then the bound"""
    F = bc.stat_fid()
    covered, lo, hi = bc.stat_figures(bc.StandIn(), F)
    print("definition:", covered, lo, hi)
    assert covered == 188 and round(lo, 3) == 0.913 and round(hi, 3) == 1.090
    covered, lo, hi = bc.stat_figures(be, F)
    print("device:", covered, lo, hi)
    assert covered >= 176 and 0.85 <= lo and hi <= 1.15
    bc.check_statistics(be)


# ---- 7. torch tensors on a side stream ---------------------------------------------------------------------------------------------
def test_side_stream_equals_the_numpy_path(be):
    import torch
    F = bc.ragged_fid(1000)
    want = be.bootstrap_metrics(F, 67, 5, offset=3, q_thresholds=bc.Q)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Ft = torch.from_numpy(F).to(be.compute_device(), non_blocking=False)
        got = be.bootstrap_metrics(Ft, 67, 5, offset=3, q_thresholds=bc.Q)
        only = be.bootstrap_metrics(Ft, 67, 5, offset=3, q_thresholds=bc.Q, want=("summary",))
    side.synchronize()
    assert got["replicates"].device == Ft.device and tuple(got["names"]) == tuple(want["names"]) and set(only) == {"summary", "names"}
    for k in ("replicates", "summary"):
        assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert only["summary"].cpu().numpy().tobytes() == want["summary"].tobytes()


def test_rim_metrics_wrapper(be):
    rm = importlib.import_module("code-robchar_amd.rim_metrics")
    F = np.random.default_rng(8).beta(8.0, 2.0, (3, 200))
    s = be.bootstrap_metrics(F, 100, 6, q_thresholds=be.Q_THRESHOLDS, want=("summary",))["summary"]
    rows = rm.bootstrap_metrics(F, n_boot=100, seed=6)
    assert list(rows) == list(rm.METRIC_NAMES)
    assert np.array_equal(rows[rm.METRIC_NAMES[0]]["lower"], s[0, 2]) and np.array_equal(rows[rm.METRIC_NAMES[3]]["se"], s[1, 1])
    assert np.array_equal(rows[rm.METRIC_NAMES[1]]["lower"], -s[3, 3]) and np.array_equal(rows[rm.METRIC_NAMES[1]]["upper"], -s[3, 2])
    assert np.array_equal(rows[rm.METRIC_NAMES[4]]["lower"], -s[2, 3]) and np.array_equal(rows[rm.METRIC_NAMES[4]]["se"], s[2, 1])
    one = rm.bootstrap_metrics(F[0], n_boot=100, seed=6)
    assert all(isinstance(one[m][k], float) and one[m][k] == rows[m][k][0] for m in rm.METRIC_NAMES for k in ("se", "lower", "upper"))


# ---- 8. MCDataSim.get_bootstrap_dict -----------------------------------------------------------------------------------------------
@pytest.fixture
def sim(be, tmp_path, monkeypatch):
    import test_mcdatasim_sensitivity as ms
    mcmod = importlib.import_module("code-robchar_amd.mc_data_sim")
    monkeypatch.chdir(tmp_path)
    os.makedirs("experiments/sens")
    le = ms.controllers(np.random.default_rng(3))
    json.dump(le, open(f"experiments/sens/ppo_spin_{ms.N}_{ms.A}-{ms.B}_c_{ms.C}.le", "w"))
    s = mcmod.MCDataSim(experiment_name="sens", Nspin=ms.N, inspin=ms.A, outspin=ms.B, noises=ms.NOISES, bootreps=40,
                        training_noise=ms.TN, numcontrollers=ms.C, filemarker=".le", verbose=False, seed=ms.SEED)
    s.ms = ms
    return s


def same_bootstrap(x, y):
    return list(x) == list(y) and all(np.array_equal(np.array(x[a][m][k], dtype=np.float64), np.array(y[a][m][k], dtype=np.float64),
                                                     equal_nan=True) for a in x for m in x[a] for k in ("se", "lower", "upper"))


def test_mcdatasim_bootstrap_dict(be, sim):
    rm = importlib.import_module("code-robchar_amd.rim_metrics")
    ms, L, C = sim.ms, len(sim.ms.NOISES), sim.ms.C
    before = {a: np.array(t) for a, t in sim.get_fid_dists().items()}
    state, off0 = np.random.get_state(), sim._philox_offset
    table = sim.get_bootstrap_dict(n_boot=200)
    assert sim._philox_offset == off0 and all(np.array_equal(x, y) for x, y in zip(state, np.random.get_state()))
    assert list(table) == ["ppo", "lbfgs"]
    for algo in table:
        fids = before[algo]
        assert fids.shape == (L, C, 40) and list(table[algo]) == list(rm.METRIC_NAMES)
        t = {m: {k: np.array(table[algo][m][k], dtype=np.float64) for k in ("se", "lower", "upper")} for m in rm.METRIC_NAMES}
        for m in rm.METRIC_NAMES:
            assert all(t[m][k].shape == (L, C) for k in t[m])
            assert all(np.isnan(t[m][k][:, 3]).all() and np.isfinite(t[m][k][:, :3]).all() for k in t[m])            # the padded controller
            assert np.all(t[m]["lower"][:, :3] <= t[m]["upper"][:, :3]) and np.all(t[m]["se"][:, :3] >= 0.0)
        rim = 1.0 - fids[:, :3].mean(axis=2)
        tol = 40 * bc.U                                   # two summation orders of the row's mean (sigma = 0: lower = upper = it)
        assert np.all(t[rm.METRIC_NAMES[0]]["lower"][:, :3] <= rim + tol) and np.all(rim - tol <= t[rm.METRIC_NAMES[0]]["upper"][:, :3])
        for m in (rm.METRIC_NAMES[1], rm.METRIC_NAMES[2], rm.METRIC_NAMES[4]):                                         # stored negated
            assert np.all(t[m]["upper"][:, :3] <= 0.0)
        assert np.all(t[rm.METRIC_NAMES[4]]["upper"][:, :3] <= -fids[:, :3].min(axis=2))       # no resample has a smaller minimum
        assert np.all(t[rm.METRIC_NAMES[0]]["se"][1:, :3] > 0.0)
        # the launch is over L * C rows, row j C + c, stream `seed` at offset 0
        direct = be.bootstrap_metrics(np.ascontiguousarray(fids.reshape(L * C, 40)), 200, ms.SEED, q_thresholds=be.Q_THRESHOLDS,
                                      want=("summary",))["summary"]
        assert np.array_equal(t[rm.METRIC_NAMES[0]]["se"], direct[0, 1].reshape(L, C), equal_nan=True)
        assert np.array_equal(t[rm.METRIC_NAMES[1]]["lower"], -direct[3, 3].reshape(L, C), equal_nan=True)
    after = {a: np.array(t) for a, t in sim.get_fid_dists().items()}
    assert all(np.array_equal(before[a], after[a], equal_nan=True) for a in before)

    # cache policy
    path = sim.get_mcname(ms.TN, ms.NOISES) + "b"
    stored = json.load(open(path))
    assert stored["n_boot"] == 200 and stored["conf"] == 0.95 and stored["seed"] == ms.SEED
    calls = []
    real = be.bootstrap_metrics
    import unittest.mock as mock
    with mock.patch.object(be, "bootstrap_metrics", side_effect=lambda *a, **k: (calls.append(1), real(*a, **k))[1]):
        assert same_bootstrap(sim.get_bootstrap_dict(n_boot=200), table) and not calls                   # served from the file
        assert same_bootstrap(sim.get_bootstrap_dict(n_boot=200, algoname="lbfgs"), {"lbfgs": table["lbfgs"]}) and not calls
        other = sim.get_bootstrap_dict(n_boot=200, seed=ms.SEED + 1)
        assert len(calls) == 2 and not same_bootstrap(other, table)
        sim.get_bootstrap_dict(n_boot=100, seed=ms.SEED + 1)
        assert len(calls) == 4 and json.load(open(path))["n_boot"] == 100
        sim.get_bootstrap_dict(n_boot=100, seed=ms.SEED + 1, conf=0.9)
        assert len(calls) == 6 and json.load(open(path))["conf"] == 0.9
        os.remove(path)
        sim.cache_format = "none"
        sim.get_bootstrap_dict(n_boot=100)
        assert not os.path.exists(path)


def test_mcdatasim_bootstrap_from_the_device_handle(be, sim, monkeypatch):
    """cache_format="none": the tensors are `DeviceFids` handles on the GPU (three rows per level, the fourth controller padded);
    the table equals the one of the NaN-padded host tensor, and no file is written"""
    mcmod = importlib.import_module("code-robchar_amd.mc_data_sim")
    rm = importlib.import_module("code-robchar_amd.rim_metrics")
    sim.cache_format = "none"
    dists = sim.get_fid_dists()
    assert all(isinstance(d, mcmod.DeviceFids) and d.tensor is not None and d.tensor.shape[1] == 3 for d in dists.values())
    monkeypatch.setattr(sim, "get_fid_dists", lambda *a, **k: dists)
    table = sim.get_bootstrap_dict(n_boot=50, conf=0.9)
    L, C = len(sim.ms.NOISES), sim.ms.C
    for algo, d in dists.items():
        host = np.array(d)
        assert host.shape == (L, C, 40) and np.isnan(host[:, 3]).all()
        want = rm.bootstrap_metrics(host.reshape(L * C, 40), n_boot=50, seed=sim.ms.SEED, conf=0.9)
        assert same_bootstrap({algo: table[algo]}, {algo: {m: {k: v.reshape(L, C) for k, v in t.items()} for m, t in want.items()}})
    assert not os.path.exists(sim.get_mcname(sim.ms.TN, sim.ms.NOISES) + "b")


def test_mcdatasim_unsupported_configurations(be, sim, monkeypatch):
    sim.devices = [0]
    with pytest.raises(NotImplementedError, match="one GPU"):
        sim.get_bootstrap_dict()
    sim.devices = None
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError, match="process group"):
        sim.get_bootstrap_dict()
