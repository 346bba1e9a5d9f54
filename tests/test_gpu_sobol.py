"""The scrambled Sobol stream on the device (ABI 19): rc_draws_sobol_f64[_async] against code-robchar_amd/sobol.py - the integer
points bit for bit, Phi^-1 against mpmath -, the fused kernel rc_mc_fidelity_sobol_f64_async against generator + tensor kernel bit
for bit and against the oracle, and the statistical claim behind all of it on a shipped controller.

Phi^-1 on the device.  The NumPy restatement's worst relative error on the probe set of tests/test_sobol_definition.py is 7.12e-16
(measured there against mpmath at 50 digits); the device differs from it in ln_table, the reciprocal root and fused multiply-adds,
so its bar is four times that, 2.85e-15 relative, and - whatever is measured - 1e-13 max(1, |z|) absolute.  Measured on an MI355X:
6.85e-16 relative against mpmath, 8.9e-16 against the NumPy restatement, 1.8e-15 absolute.

The statistical claim (N = 7, the first shipped delocalised 0 -> 6 controller, sigma = 0.05, R = 16, P = 1024).  On the CPU, sobol.py +
the oracle against 2^18 NumPy normals: SE_MC(K = 16 384) = 1.416e-3; SE_RQMC = 1.36e-4 with the scramble seed 2026 used here, a ratio
of 10.5 (seeds 1 and 2 give 8.9 and 9.1: the SE of 16 replicate means is itself known to about 18 %); |mean_RQMC - mean_MC| is 0.07
of its allowance 5 SE + 5 SE.  The test asks for a ratio of 5.  (On an MI355X, against 2^18 Philox draws: the same 10.5.)"""
import importlib

import numpy as np
import pytest

import chain_checks as cc
from oracle import robchar_oracle as orc
from test_sobol_definition import checked_reference, probe_words

pytestmark = pytest.mark.gpu
sobol = importlib.import_module("code-robchar_amd.sobol")
TOL = 1e-10
PHI_REL_BAR = 4 * 7.12e-16
SHAPES = ((1, 100, 100), (3, 64, 192), (2, 128, 200))                 # (R, P, K): K = 192 crosses n0 = 64 and 128
SKIPS = (0, 320, 2 ** 20 + 64, 2 ** 32 - 128)


@pytest.fixture(scope="module")
def dev(be):
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def host_bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("D", (6, 21, 39, 96))
def test_integer_points_equal_the_definition(be, dev, D):
    C = 3
    for R, P, K in SHAPES:
        for per_row in (False, True):
            dirnum, shift = sobol.scramble(D, R, seed=100 * D + R, C=C if per_row else None)
            for skip in SKIPS:
                want = sobol.points(dirnum, shift, P, K, skip, C=C)
                got = be.sobol_points(dirnum, shift, P, K, skip=skip, C=C, device=dev, as_torch=True)
                assert got.shape == (C, K, D) and np.array_equal(host_bits(got), want), (D, R, P, K, skip, per_row)
    # the blocking twin on host arrays, and both outputs of one launch
    dirnum, shift = sobol.scramble(D, 3, seed=9, C=C)
    want = sobol.points(dirnum, shift, 64, 192, 320)
    got = be.sobol_points(dirnum, shift, 64, 192, skip=320)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    both = be._sobol_generate(("draws", "bits"), dirnum, shift, 64, 192, 320, 1.0, None, dev, True)
    assert np.array_equal(host_bits(both["bits"]), want)
    assert np.array_equal(both["draws"].cpu().numpy(), be.sobol_normal(dirnum, shift, 64, 192, skip=320))


def device_normals(be, dev, words, sigma=1.0):
    """z of chosen words: with an all-zero direction table the point IS the shift - one row per 96 words, one sample per row"""
    n = len(words)
    C = -(-n // 96)
    shift = np.zeros((C, 1, 96), dtype=np.uint32)
    shift.reshape(-1)[:n] = words
    res = be._sobol_generate(("draws", "bits"), np.zeros((1, 96, 32), dtype=np.uint32), shift, 1, 1, 0, sigma, C, dev, True)
    assert np.array_equal(host_bits(res["bits"]).reshape(-1)[:n], words)
    return res["draws"].cpu().numpy().reshape(-1)[:n]


def test_phi_inverse_on_the_device(be, dev):
    words = probe_words()
    z = device_normals(be, dev, words)
    assert np.array_equal(device_normals(be, dev, ~words), -z)                      # z(~x) == -z(x) bit for bit
    ref = checked_reference(words)
    rel = np.abs(z - ref) / np.abs(ref)
    host = sobol.normal_from_bits(words)
    print(f"Phi^-1 on the device vs mpmath: worst relative error {rel.max():.3e} at word {int(words[rel.argmax()])} (bar {PHI_REL_BAR:.3e}); "
          f"vs the NumPy restatement: {np.abs(z / host - 1).max():.3e}; worst absolute error {np.abs(z - ref).max():.3e}")
    assert np.all(np.abs(z - ref) <= 1e-13 * np.maximum(1.0, np.abs(ref)))
    assert rel.max() <= PHI_REL_BAR


def test_draws_are_one_rounded_product_of_the_device_normal(be, dev):
    D, C, R, P, K = 21, 4, 2, 128, 200
    dirnum, shift = sobol.scramble(D, R, seed=77, C=C)
    z = be.sobol_normal(dirnum, shift, P, K, skip=64, sigma=1.0, C=C, device=dev, as_torch=True).cpu().numpy()
    sig = np.array([0.05, 0.0, 1e-3, 0.3])
    got = be.sobol_normal(dirnum, shift, P, K, skip=64, sigma=sig, C=C, device=dev, as_torch=True).cpu().numpy()
    assert np.array_equal(got, sig[:, None, None] * z)
    assert np.all(got[1] == 0.0) and np.signbit(got[1]).any() and not np.signbit(got[1]).all()      # +-0
    assert np.array_equal(be.sobol_normal(dirnum, shift, P, K, skip=64, sigma=0.05, C=C, device=dev, as_torch=True).cpu().numpy(), 0.05 * z)
    assert np.abs(z / sobol.normal_from_bits(sobol.points(dirnum, shift, P, K, 64)) - 1).max() < PHI_REL_BAR


def two_routes(be, dev, ctrl, N, a, b, dirnum, shift, P, K, skip, sigma, **static):
    """(fused, generator + tensor kernel) fidelities as host arrays"""
    import torch
    C = ctrl.shape[0]
    ct = torch.from_numpy(ctrl).to(dev)
    draws = be.sobol_normal(dirnum, shift, P, K, skip=skip, sigma=sigma, C=C, device=dev, as_torch=True).view(C, K, N, 3)
    want = be.mc_fidelity(ct, draws, N, a, b, kernel="auto", **static)
    got = be.mc_fidelity_sobol(ct, K, N, a, b, dirnum, shift, P, skip=skip, sigma=sigma, **static)
    return got.cpu().numpy(), want.cpu().numpy()


@pytest.mark.parametrize("N", range(2, 14))
def test_fused_kernel_is_bit_identical_to_generator_plus_tensor_kernel(be, dev, N):
    """every instantiation of the fused kernel.  The controllers of seed 5100 + N pass `assert_has_teeth` at every N (on the CPU, the
    oracle reference below: the smallest median F is 0.196, at N = 11, and every sample is above 1e-3), so no seed had to move."""
    rng = np.random.default_rng(5100 + N)
    C = 4
    ctrl = cc.deloc_ctrl(rng, C, N, 0.5)
    ctrl[2, N // 2] = np.nan                                                        # a padded row
    static = dict(h0_diag=rng.uniform(-0.3, 0.3, N), h0_offdiag=rng.uniform(0.8, 1.2, N - 1))
    sig = np.array([0.05, 0.0, 0.05, 0.1])
    pairs = ((0, N - 1), (N - 1, 0)) if N == 2 else ((0, N - 1), (1, N - 2) if N > 3 else (1, 0))
    for (R, P, K), skip in zip(SHAPES, (0, 320, 2 ** 32 - 128)):
        for per_row in (False, True):
            dirnum, shift = sobol.scramble(3 * N, R, seed=N + R, C=C if per_row else None)
            for a, b in pairs:
                for sigma in (0.05, sig):
                    got, want = two_routes(be, dev, ctrl, N, a, b, dirnum, shift, P, K, skip, sigma, **static)
                    assert np.isnan(got[2]).all() and np.array_equal(got, want, equal_nan=True), (N, R, P, K, skip, per_row, a, b)
                    assert np.nanmax(got) > 1e-3
    # the independent reference: the oracle fed with the definition's normals
    dirnum, shift = sobol.scramble(3 * N, 2, seed=3, C=C)
    good = np.ascontiguousarray(ctrl[[0, 1, 3]])
    sh = np.ascontiguousarray(shift[[0, 1, 3]])
    got, _ = two_routes(be, dev, good, N, 0, N - 1, dirnum, sh, 128, 200, 64, sig[[0, 1, 3]], **static)
    want = orc.fidelity_eigh(good, sobol.normals(dirnum, sh, 128, 200, 64, sigma=sig[[0, 1, 3]]).reshape(3, 200, N, 3), N, 0, N - 1, **static)
    cc.assert_has_teeth(want, what=(N, "sobol"))
    err = np.abs(got - want)
    print(f"fused Sobol kernel vs oracle, N = {N}: abs {err.max():.1e} rel {(err[want > 1e-3] / want[want > 1e-3]).max():.1e}")
    assert err.max() < TOL and np.all(err[want > 1e-3] <= 1e-9 * want[want > 1e-3]), (N, err.max())
    assert np.array_equal(got[1], np.full(200, got[1, 0]))                         # the sigma = 0 row: the nominal fidelity


@pytest.mark.parametrize("N", (6, 7))
def test_fused_kernel_repair_lanes_regenerate_their_coordinates(be, dev, N):
    """the project's hard inputs: a uniform chain, near-degenerate biases and a mirror-symmetric controller on a chain cut in the
    middle (odd N: on both sides of the middle site) with very weak noise - exactly or nearly degenerate spectra, which the
    eigenvalue-only weights hand to the eigenvector repair; its lanes make their coordinates again, element by element.  Every
    pair of both N must take the repair route in some tile (measured at N = 6: the 8 tiles of the two mirror-symmetric rows)"""
    rng = np.random.default_rng(77 + N)
    h = N // 2
    ctrl = np.zeros((4, N + 1))
    ctrl[:, N] = (7.0, 5.0, 9.0, 7.0)
    ctrl[1, :N] = rng.uniform(-1e-6, 1e-6, N)                                      # near-degenerate biases
    ctrl[2, :h] = rng.uniform(-2, 2, h)
    ctrl[2, N - h:N] = ctrl[2, :h][::-1]                                           # mirror-symmetric
    ctrl[3] = ctrl[2]
    h0o = np.ones(N - 1)
    h0o[h - 1] = h0o[N - 1 - h] = 0.0                                              # two identical halves (odd N: and a lone middle site)
    sig = np.array([0.05, 0.05, 1e-13, 0.0])
    dirnum, shift = sobol.scramble(3 * N, 2, seed=41, C=4)
    for a, b in ((1, 1), (0, N - 1), (1, h - 1)):
        import torch
        ct = torch.from_numpy(ctrl).to(dev)
        draws = be.sobol_normal(dirnum, shift, 128, 200, skip=64, sigma=sig, C=4, device=dev, as_torch=True).view(4, 200, N, 3)
        want = be.mc_fidelity(ct, draws, N, a, b, h0_offdiag=h0o).cpu().numpy()
        be.general_path_tiles(reset=True)
        got = be.mc_fidelity_sobol(ct, 200, N, a, b, dirnum, shift, 128, skip=64, sigma=sig, h0_offdiag=h0o).cpu().numpy()
        tiles = be.general_path_tiles()
        print(f"N = {N} ({a}, {b}): {tiles} of 16 tiles took the repair route")
        assert np.array_equal(got, want), (N, a, b)
        assert tiles >= 1, (N, a, b)
        ref = orc.fidelity_eigh(ctrl, sobol.normals(dirnum, shift, 128, 200, 64, sigma=sig).reshape(4, 200, N, 3), N, a, b, h0_offdiag=h0o)
        assert np.abs(got - ref).max() < TOL, (N, a, b)


def test_rqmc_beats_plain_monte_carlo_on_a_shipped_controller(be, dev, lbfgs_n7):
    import torch
    N, R, P, sigma = 7, 16, 1024, 0.05
    ctrl = np.ascontiguousarray(lbfgs_n7["ctrl_0-6"][:1])
    ct = torch.from_numpy(ctrl).to(dev)
    dirnum, shift = sobol.scramble(3 * N, R, seed=2026)
    fid = be.mc_fidelity_sobol(ct, R * P, N, 0, 6, dirnum, shift, P, sigma=sigma)
    means = fid.view(R, P).mean(dim=1).cpu().numpy()
    se_q = means.std(ddof=1) / np.sqrt(R)
    mc = be.mc_fidelity_philox(ct, 2 ** 18, N, 0, 6, seed=12345, sigma=sigma)[0]
    se_big = float(mc.std()) / np.sqrt(2 ** 18)
    se_16k = float(mc[:16384].std()) / np.sqrt(16384)
    print(f"RQMC mean {means.mean():.6f} SE {se_q:.3e}; Philox mean {float(mc.mean()):.6f} SE(2^18) {se_big:.3e} SE(16 384) {se_16k:.3e}; "
          f"ratio {se_16k / se_q:.1f}")
    assert len(set(means.tolist())) > 1                                             # (a)
    assert abs(means.mean() - float(mc.mean())) <= 5 * se_big + 5 * se_q            # (b)
    assert se_q <= se_16k / 5                                                       # (c)
    # the same numbers through the noise model, fused route and - forced - the generator + tensor kernel route
    nm = importlib.import_module("code-robchar_amd.noise")
    model = nm.structured_perturbation(Nspin=N, inspin=0, outspin=6, noise=sigma)
    res = model.fidelity_rqmc(ctrl, replicates=R, points=P, seed=2026)
    assert res["mean"].shape == res["se"].shape == (1,) and res["replicate_means"].shape == (1, R)
    assert abs(res["mean"][0] - means.mean()) < 1e-12 and abs(res["se"][0] - se_q) < 1e-12
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(be, "sobol_fused_supported", lambda *a, **k: False)
        two = model.fidelity_rqmc(ctrl, replicates=R, points=P, seed=2026)
    assert np.array_equal(two["replicate_means"], res["replicate_means"])
    zero = model.fidelity_rqmc(ctrl, replicates=4, points=64, seed=1, sigma=0.0)
    assert zero["se"][0] == 0.0


def test_hip_host_client(be, dev, tmp_path):
    """tests/host/hip_client_sobol.cpp: table -> generator -> tensor kernel and the fused kernel through the C entries on the
    program's own stream, no Python; its replicate means against `mc_fidelity_sobol` with the same tables"""
    import os
    import shutil
    import subprocess
    import torch
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "code-robchar_amd", "csrc")
    exe = str(tmp_path / "hip_client_sobol")
    subprocess.run([hipcc, "-O1", "--offload-arch=gfx950", "-I", os.path.join(root, "include"), "-o", exe,
                    os.path.join(root, "tests", "host", "hip_client_sobol.cpp"), "-L", libdir, "-lrobchar_hip", f"-Wl,-rpath,{libdir}"], check=True)
    N, C, R, P, skip, sigma = 5, 3, 4, 128, 64, 0.05
    ctrl = cc.deloc_ctrl(np.random.default_rng(12), C, N, 0.5)
    res = subprocess.run([exe] + [str(v) for v in (N, 0, N - 1, C, R, P, skip, sigma)], input=" ".join(repr(float(v)) for v in ctrl.ravel()),
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.strip().split("\n")
    assert lines[0] == "identical 1"
    got = np.array([[float(v) for v in line.split()] for line in lines[1:]])
    D = 3 * N
    dirnum = np.broadcast_to(sobol.direction_numbers(D), (R, D, 32)).copy()
    shift = ((np.arange(1, R * D + 1, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(1, R, D)
    fid = be.mc_fidelity_sobol(torch.from_numpy(ctrl).to(dev), R * P, N, 0, N - 1, dirnum, shift, P, skip=skip, sigma=sigma).cpu().numpy()
    want = fid.reshape(C, R, P).mean(axis=2)
    assert got.shape == (C, R) and np.abs(got - want).max() < 1e-14 and want.mean() > 1e-2


def test_get_qmc_dict_on_the_seeded_small_experiment(workdir, monkeypatch):
    """the product: `MCDataSim.get_qmc_dict` on the experiment of test_gpu_mcdatasim.py (N = 5, 0 -> 2, levels 0 / 0.05 / 0.1, three
    controllers + one padded) against the plain Monte Carlo RIM_1 of `get_metrics_dict` with 400 draws per level"""
    import json
    import os
    from conftest import load_json
    mcmod = importlib.import_module("code-robchar_amd.mc_data_sim")
    rm = importlib.import_module("code-robchar_amd.rim_metrics")
    g = load_json("mcsim_run.json")
    os.makedirs("experiments/golden")
    json.dump(g["le"], open(f"experiments/golden/ppo_spin_{g['Nspin']}_{g['inspin']}-{g['outspin']}_c_{g['numcontrollers']}.le", "w"))
    np.random.seed(1234)
    K = 400
    sim = mcmod.MCDataSim(experiment_name="golden", Nspin=g["Nspin"], inspin=g["inspin"], outspin=g["outspin"], noises=np.array(g["noises"]),
                          bootreps=K, training_noise=0.05, numcontrollers=g["numcontrollers"], filemarker=".le", verbose=False)
    metrics = sim.get_metrics_dict()
    table = sim.get_qmc_dict(replicates=8, points=256, seed=5)
    assert list(table) == list(metrics)
    for algo, t in table.items():
        rim, se = np.array(t["rim"], dtype=np.float64), np.array(t["rim_se"], dtype=np.float64)
        ref = np.array(metrics[algo][rm.METRIC_NAMES[0]], dtype=np.float64)
        se_mc = np.array(metrics[algo][rm.METRIC_NAMES[3]], dtype=np.float64) / np.sqrt(K)
        assert rim.shape == ref.shape == (3, g["numcontrollers"]) and np.array_equal(np.isnan(rim), np.isnan(ref))
        ok = ~np.isnan(ref)
        print(algo, "max |rim - RIM_1| / (5 SE_RQMC + 5 SE_MC):", np.nanmax(np.abs(rim - ref)[1:] / (5 * se + 5 * se_mc)[1:]),
              "sigma = 0 level: max |rim - RIM_1|", np.nanmax(np.abs(rim - ref)[0]))
        assert np.all(np.abs(rim - ref)[ok] <= (5 * se + 5 * se_mc)[ok]), algo
        assert np.all(se[0][ok[0]] == 0.0) and np.all(se[1:][ok[1:]] > 0.0)
        assert np.all(np.array(t["std_se"], dtype=np.float64)[0][ok[0]] == 0.0)
    # a second call reads the cache
    monkeypatch.setattr(sim.noise_model, "fidelity_rqmc_replicates", lambda *a, **k: pytest.fail("recomputed"))
    again = sim.get_qmc_dict(replicates=8, points=256, seed=5)
    assert json.dumps(again) == json.dumps(table)
