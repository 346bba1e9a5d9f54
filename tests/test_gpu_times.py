"""`backend.mc_fidelity_times` / `mc_fidelity_times_philox` - the chain fidelity on a grid of readout times from one eigen
decomposition per sample - on the device: the checks of times_checks.py (oracle with teeth on every instantiation N = 2 ... 16,
the closed-form spin-j chain, every output against its definition, tile boundaries, M = 1 and 64, a NaN row, shared draws,
negative T a + b), slab j against the rows kernel BIT FOR BIT, torch tensors on a side stream, the kernel that generates its
draws bit-identical to `philox_normal` + the tensor kernel, and the wrappers on top (`fidelity_readout_jitter_philox`,
`MCDataSim.get_readout_dict`).  Shapes are the smallest that reach those paths.
ROBCHAR_TIMES_FORCED_GENERAL=1 announces a -DRC_TIMES_FORCE_GENERAL=1 variant build (scripts/build_variant.sh), in which every
tile takes the sweep-cap fallback: the same file runs and the counter must count."""
import importlib
import os

import numpy as np
import pytest

import chain_checks as cc
import stand_in
import times_checks as tc
from oracle import philox_host
from oracle import robchar_oracle as orc

pytestmark = pytest.mark.gpu
FORCED = os.environ.get("ROBCHAR_TIMES_FORCED_GENERAL") == "1"      # a -DRC_TIMES_FORCE_GENERAL=1 variant build
EPS = 2.0 ** -52
SEED = 0x5EED0010


def counted(be, run):
    """`run()` between two resets of the fallback counter: zero tiles on the product build, some on the forced variant"""
    be.times_general_tiles(reset=True)
    res = run()
    tiles = be.times_general_tiles(reset=True)
    assert (tiles > 0) if FORCED else (tiles == 0), tiles
    return res


@pytest.mark.parametrize("N,a,b", tc.EVERY_SIZE)
def test_oracle_with_teeth(be, N, a, b):
    worst = cc.Worst()
    counted(be, lambda: tc.check_oracle(be, N, a, b, worst))
    print("times vs oracle:", (N, a, b), worst)


@pytest.mark.parametrize("N", tc.STEP_SIZES)
def test_closed_form(be, N):
    worst = cc.Worst()
    counted(be, lambda: tc.check_closed_form(be, N, worst))
    print("times vs closed form:", N, worst)


@pytest.mark.parametrize("N,a,b", tc.EVERY_SIZE)
def test_slabs_are_the_rows_kernel_bit_for_bit(be, N, a, b):
    """The same operations as mc_fidelity(kernel="tridiag_ql") at the row's time, so the same bits.  (The forced variant runs the
    textbook routine instead - another summation order: there the bound between two fp64 eigen routes of tests/test_gpu_grad.py,
    64 N eps max(1, |t| ||H||), applies.)"""
    worst = tc.check_against_rows_kernel(be, N, a, b, exact=not FORCED)
    print("times vs rows kernel, max |dF|:", (N, a, b), worst)
    if FORCED:
        ctrl, draws, _ = tc.oracle_workload(N, a, b)
        t = tc.times_of(ctrl[:, N], tc.TSCALE, tc.TSHIFT).max()
        norm = np.abs(np.linalg.eigvalsh(orc.assemble_hamiltonians(ctrl, draws, N))).max()
        assert worst <= 64 * N * EPS * max(1.0, t * norm), worst


def test_semantics(be):
    counted(be, lambda: tc.check_semantics(be))


def test_edges(be):
    counted(be, lambda: tc.check_edges(be))


@pytest.mark.parametrize("N", tc.STEP_SIZES)
def test_hard_inputs_need_no_fallback(be, N):
    """The inputs a spectral route is most likely to get wrong (grad_checks.hard_inputs: uniform and mirror-symmetric chains, a
    clustered spectrum, a cut bond, T = 0, biases of 1e3): the rows route has no condition on any of them - the product build
    counts zero fallback tiles (the forced variant counts every tile) and gives the rows kernel's bits."""
    import grad_checks as gc
    for name, ctrl, draws in gc.hard_inputs(N, np.random.default_rng(7700 + N)):
        for (a, b) in ((0, N - 1), (N // 2, N // 2)):
            want = tc.reference_slabs(ctrl, draws, N, a, b, tc.TSCALE, tc.TSHIFT)
            got = counted(be, lambda: be.mc_fidelity_times(ctrl, draws, N, a, b, tscale=tc.TSCALE, tshift=tc.TSHIFT, want=("fid",))["fid"])
            t = be.readout_times(ctrl[:, N], tc.TSCALE, tc.TSHIFT)
            if not FORCED:
                for j in range(len(tc.TSCALE)):
                    rows = be.mc_fidelity(tc.with_time(ctrl, t[:, j]), draws, N, a, b, kernel="tridiag_ql")
                    assert np.array_equal(got[j], rows), (name, N, a, b, j)
            if name == "bias 1e3":
                # eigenvalues of size 1e3 carry N eps 1e3 of rounding, which t multiplies: the bound between two fp64 eigen routes
                # of tests/test_gpu_grad.py, 64 N eps max(1, |t| ||H||)
                assert np.abs(got - want).max() <= 64 * N * EPS * max(1.0, t.max() * 1.0e3), name
            else:
                cc.compare(got, want, (name, N, a, b))


def test_a_null_matrix_takes_the_textbook_routine(be):
    """The one input known to leave the fast path: every bond cut and every bias zero - H = 0, so no coupling (1e-150 after the
    exact cancellation) is ever negligible against |d_l| + |d_l+1| = 0 and the fast QL runs into its sweep cap.  Those samples
    take the textbook routine in LDS, on the product build too: the results are exact and the counter counts."""
    N, K = 7, 65
    ctrl = np.zeros((2, N + 1))
    ctrl[:, N] = (3.0, 2.0)
    ctrl[0, :N] = 0.25                                                   # H = 0.25 * 1: as null up to a global phase, d != 0
    draws = np.zeros((2, K, N, 3))
    draws[:, :, 1:, 1] = -1.0                                            # every bond cut: H diagonal
    be.times_general_tiles(reset=True)
    res = be.mc_fidelity_times(ctrl, draws, N, 0, 2, tscale=tc.TSCALE, tshift=tc.TSHIFT, weights=np.ones(5), want=be.TIMES_OUTPUTS)
    same = be.mc_fidelity_times(ctrl, draws, N, 3, 3, tscale=tc.TSCALE, tshift=tc.TSHIFT, want=("fid", "min"))
    tiles = be.times_general_tiles(reset=True)
    assert all(np.abs(v).max() < 1e-200 for v in res.values())           # nothing is transferred
    assert np.abs(same["fid"] - 1.0).max() < 1e-14 and np.abs(same["min"] - 1.0).max() < 1e-14
    assert tiles == (8 if FORCED else 4), tiles                          # row 1 (H = 0): its two tiles, in both launches


def test_torch_tensors_on_a_side_stream(be):
    import torch
    N, a, b = 7, 0, 6
    ctrl, draws, _ = tc.oracle_workload(N, a, b)
    w = np.array([0.1, 0.2, 0.4, 0.2, 0.1])
    want = be.mc_fidelity_times(ctrl, draws, N, a, b, tscale=tc.TSCALE, tshift=tc.TSHIFT, weights=w, want=be.TIMES_OUTPUTS)
    dev = be.compute_device()
    side = torch.cuda.Stream(device=dev)
    ct, dt = torch.from_numpy(np.array(ctrl)).to(dev), torch.from_numpy(np.array(draws)).to(dev)
    torch.cuda.current_stream(dev).synchronize()
    with torch.cuda.stream(side):
        got = be.mc_fidelity_times(ct, dt, N, a, b, tscale=tc.TSCALE, tshift=tc.TSHIFT, weights=w, want=be.TIMES_OUTPUTS)
    side.synchronize()
    assert sorted(got) == sorted(want) and all(v.is_cuda for v in got.values())
    for k in want:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    # slab j goes to the existing consumers unchanged
    red = be.reduce_metrics(got["fid"][3], q_thresholds=())
    assert np.abs(red["rim1"][0].cpu().numpy() - (1.0 - want["fid"][3].mean(axis=1))).max() < 1e-12


# ------------------------------------------------------------------------------------------------------------------------
# draws generated inside the kernel
# ------------------------------------------------------------------------------------------------------------------------

def philox_rows(N, nan_row=True):
    rng = np.random.default_rng(40 + N)
    ctrl = cc.deloc_ctrl(rng, 3, N, 0.5)
    ctrl[2, N] = -ctrl[2, N]                                             # a negative time entry
    if nan_row:
        ctrl[1, 0] = np.nan
    return ctrl


def two_kernels(be, ctrl, K, N, a, b, offset, sigma, **grid):
    """`philox_normal` into a (C, K, N, 3) tensor - row by row when sigma is per row: row c starts at offset + c K 3 N -, then the
    tensor kernel"""
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (ctrl.shape[0],))
    draws = np.concatenate([be.philox_normal((1, K, N, 3), SEED, scale=float(s), offset=offset + c * K * N * 3)
                            for c, s in enumerate(sig)])
    return be.mc_fidelity_times(ctrl, draws, N, a, b, want=be.TIMES_OUTPUTS, **grid), draws


def fused(be, ctrl, K, N, a, b, offset, sigma, **grid):
    res = be.mc_fidelity_times_philox(ctrl, K, N, a, b, SEED, offset=offset, sigma=sigma, want=be.TIMES_OUTPUTS, **grid)
    return {k: v.cpu().numpy() for k, v in res.items()}


GRID = dict(tscale=tc.TSCALE, tshift=tc.TSHIFT, weights=np.array([0.1, 0.2, 0.4, 0.2, 0.1]))


@pytest.mark.parametrize("N", tc.SIZES)
def test_philox_is_bit_identical_to_the_two_kernel_route(be, N):
    """both parities of the first element, K = 65 (a full tile and a lane), a NaN row, a negative time entry"""
    ctrl = philox_rows(N)
    for (a, b) in ((0, N - 1), (N // 2, max(0, N // 2 - 1))):
        for offset in (0, 7):
            want, _ = two_kernels(be, ctrl, 65, N, a, b, offset, 0.05, **GRID)
            cc.assert_has_teeth(want["fid"], what=("two-kernel route", N, a, b))
            got = counted(be, lambda: fused(be, ctrl, 65, N, a, b, offset, 0.05, **GRID))
            for k in be.TIMES_OUTPUTS:
                assert np.isnan(got[k][..., 1, :]).all()
                assert np.array_equal(got[k], want[k], equal_nan=True), (N, a, b, offset, k)


@pytest.mark.parametrize("N", (7, 12))
def test_philox_per_row_sigma_and_a_far_offset(be, N):
    """sigma_rows = (0, 0.02, 0.1) and offset = 2^40 + 3: every row is the two-kernel route at the row's own sigma and offset; in the
    sigma = 0 row all K samples carry the same bits; against host-regenerated draws and the oracle too"""
    K, a, b, offset = 65, 0, N - 1, 2 ** 40 + 3
    rows = np.array([0.0, 0.02, 0.1])
    ctrl = philox_rows(N, nan_row=False)
    want, draws = two_kernels(be, ctrl, K, N, a, b, offset, rows, **GRID)
    got = fused(be, ctrl, K, N, a, b, offset, rows, **GRID)
    for k in be.TIMES_OUTPUTS:
        assert np.array_equal(got[k], want[k]), (N, k)
    assert (got["fid"][:, 0] == got["fid"][:, 0, :1]).all() and not (got["fid"][:, 2] == got["fid"][:, 2, :1]).all()
    host = rows[:, None, None, None] * philox_host.philox_normal(SEED, offset, 3 * K * N * 3, 1.0).reshape(3, K, N, 3)
    cc.compare(got["fid"], tc.reference_slabs(ctrl, host, N, a, b, tc.TSCALE, tc.TSHIFT), (N, "host-regenerated draws"))


# ------------------------------------------------------------------------------------------------------------------------
# wrappers
# ------------------------------------------------------------------------------------------------------------------------

def test_readout_jitter_against_the_oracle_at_the_nodes(be):
    noise = importlib.import_module("code-robchar_amd.noise")
    N, a, b, K, sigma, sigma_t = 5, 0, 4, 70, 0.05, 0.3
    model = noise.structured_perturbation(Nspin=N, inspin=a, outspin=b, noise=sigma)
    ctrl = cc.deloc_ctrl(np.random.default_rng(8), 3, N, 0.5)
    got = model.fidelity_readout_jitter_philox(ctrl, K, SEED, sigma_t)
    draws = sigma * philox_host.philox_normal(SEED, 0, 3 * K * N * 3, 1.0).reshape(3, K, N, 3)
    x, wx = np.polynomial.hermite.hermgauss(8)
    slabs = tc.reference_slabs(ctrl, draws, N, a, b, None, np.sqrt(2.0) * sigma_t * x)
    want = np.tensordot(wx / np.sqrt(np.pi), slabs, axes=1)
    plain = orc.fidelity_eigh(ctrl, draws, N, a, b)
    assert got.shape == (3, K) and np.median(np.abs(want - plain)) > 1e-3           # the jitter matters at this sigma_t
    # every node's fidelity within 1e-10 of the oracle's, positive weights that sum to 1: the same bound for their weighted sum
    cc.compare(got, want, "jitter-averaged fidelity")


def test_get_readout_dict_against_the_stand_in(be, tmp_path, monkeypatch):
    """a two-algorithm, two-level toy experiment on the device against the same experiment around the NumPy stand-ins"""
    mcmod = importlib.import_module("code-robchar_amd.mc_data_sim")
    T = tc.TOY
    monkeypatch.chdir(tmp_path)
    tc.write_toy_experiment("readout")
    make = lambda: mcmod.MCDataSim(experiment_name="readout", Nspin=T["N"], inspin=T["A"], outspin=T["B"], noises=T["NOISES"],
                                   bootreps=5, training_noise=T["TN"], numcontrollers=T["C"], filemarker=".le", verbose=False,
                                   seed=T["SEED"], cache_format="none")
    K = 70
    got = make().get_readout_dict(samples=K, tscale=T["TSCALE"], tshift=T["TSHIFT"])
    with monkeypatch.context() as m:
        m.setattr(be, "mc_fidelity_times_philox", tc.standin_times_philox)
        m.setattr(be, "reduce_metrics", stand_in.reduce_metrics)
        want = make().get_readout_dict(samples=K, tscale=T["TSCALE"], tshift=T["TSHIFT"])
    assert list(got) == list(want) == ["ppo", "lbfgs"]
    for algo in got:
        assert got[algo]["noises"] == want[algo]["noises"] and got[algo]["tshift"] == want[algo]["tshift"]
        g, w = ({k: np.array(t[algo][k], dtype=np.float64) for k in ("rim", "std", "worst", "window_rim")} for t in (got, want))
        for k in g:
            assert g[k].shape == w[k].shape and np.array_equal(np.isnan(g[k]), np.isnan(w[k])), (algo, k)
            assert np.isnan(g[k][..., 3]).all() and not np.isnan(g[k][..., :3]).any()
        # every fidelity is within 1e-10 of the oracle's: so are a row's mean, its minimum and the mean of the per-sample minima;
        # std is 1-Lipschitz in the rms of the samples' errors (1e-10) and its own rounding is K eps max F^2 / (2 std) < 1e-11 for
        # std >= 1e-3, which the reference has
        assert np.nanmin(w["std"]) >= 1e-3
        for k, bound in (("rim", 1e-10), ("worst", 1e-10), ("window_rim", 1e-10), ("std", 2e-10)):
            err = np.nanmax(np.abs(g[k] - w[k]))
            print(algo, k, err)
            assert err < bound, (algo, k, err)
