"""The end-to-end chain kernels with the fidelity formed without weights (rc::ends_amplitude, tridiag_core.h) on the GPU:
delocalised controllers where the relative bound bites, NaN rows, cut bonds, the |d| ~ 100, T = 99 corner against the rows
mode, a close eigenvalue pair, and the fused-draws kernel bit for bit.  Every shape is C = 4, K = 130: two full 64-sample
tiles and a 2-lane partial tile per controller; sigma = 0.05."""
import numpy as np
import pytest

from oracle import robchar_oracle as orc
from test_host_core import _close_pair_matrix

pytestmark = pytest.mark.gpu
C, K, SIGMA = 4, 130, 0.05
ABS_TOL = 1e-10
REL_TOL = 1e-9
BIG = 1e-3                # the relative bound holds wherever the reference fidelity exceeds this
MIN_SHARE = 0.5
FLOOR = 1.5e-11           # the fuzz campaigns' recorded worst case at |d| ~ 100, |T| ~ 100


def _deloc(N, seed):
    """Delocalised rows: biases |B| <= 1 against the hopping J = 1, T in [2, 30]."""
    rng = np.random.default_rng(seed)
    ctrl = np.empty((C, N + 1))
    ctrl[:, :N] = rng.uniform(-1.0, 1.0, (C, N))
    ctrl[:, N] = rng.uniform(2.0, 30.0, C)
    draws = SIGMA * rng.standard_normal((C, K, N, 3))
    return ctrl, draws


def _inject(ctrl_row, draws_row, d, e):
    """Make one sample's matrix exactly tridiag(d, e): g0 = d - x, g1 = e - 1, g2 = 0 (h0 = 0, J = 1)."""
    N = len(d)
    draws_row[:, 0] = d - ctrl_row[:N]
    draws_row[1:, 1] = e - 1.0
    draws_row[:, 2] = 0.0


@pytest.mark.parametrize("N", [2, 5, 7, 10, 14])
def test_delocalised_rows_vs_oracle(be, N):
    ctrl, draws = _deloc(N, 7300 + N)
    want = orc.fidelity_eigh(ctrl, draws, N, 0, N - 1)
    big = want > BIG
    assert big.mean() >= MIN_SHARE, (N, float(big.mean()))
    got = be.mc_fidelity(ctrl, draws, N, 0, N - 1, kernel="auto")
    err = np.abs(got - want)
    rel = (err[big] / want[big]).max()
    print(f"N={N}: share F>1e-3 {big.mean():.3f}  max abs {err.max():.3e}  max rel {rel:.3e}")
    assert err.max() <= ABS_TOL, (N, float(err.max()))
    assert rel <= REL_TOL, (N, float(rel))


def test_nan_controller_row(be):
    N = 7
    ctrl, draws = _deloc(N, 7401)
    ctrl[2] = np.nan
    got = be.mc_fidelity(ctrl, draws, N, 0, N - 1, kernel="auto")
    assert np.isnan(got[2]).all() and got[2].size == K
    assert np.isfinite(np.delete(got, 2, axis=0)).all()
    want = orc.fidelity_eigh(ctrl, draws, N, 0, N - 1)
    assert np.nanmax(np.abs(got - want)) <= ABS_TOL


def test_cut_bonds_give_zero_on_the_fast_path(be):
    """J + g1 = 0, g2 = 0 on one bond of one sample: the product of the squared couplings carries 1e-300, F is zero at that
    level and the sample stays on the fast path.  Two cut bonds in one sample: the product underflows, F = 0, no NaN."""
    N = 7
    ctrl, draws = _deloc(N, 7402)
    draws[1, 70, 3, 1], draws[1, 70, 3, 2] = -1.0, 0.0
    draws[3, 129, 2, 1], draws[3, 129, 2, 2] = -1.0, 0.0
    draws[3, 129, 5, 1], draws[3, 129, 5, 2] = -1.0, 0.0
    be.general_path_tiles(reset=True)
    got = be.mc_fidelity(ctrl, draws, N, 0, N - 1, kernel="auto")
    assert be.general_path_tiles() == 0
    assert np.isfinite(got).all()
    assert 0.0 <= got[1, 70] < 1e-290, got[1, 70]
    assert got[3, 129] == 0.0, got[3, 129]
    want = orc.fidelity_eigh(ctrl, draws, N, 0, N - 1)
    assert np.abs(got - want).max() <= ABS_TOL


def test_large_bias_long_time_no_worse_than_rows_mode(be):
    """|d| ~ 100, T = 99 (|T lambda| ~ 1e4: the fuzz campaigns' hard corner, recorded floor 1.5e-11): the end-to-end kernel
    may not be further from the oracle than the rows mode - eigenvector rows through an all-fp64 QL - by more than 2e-11.
    Rows 0, 1: biases U(-100, 100) - localised, F ~ 1e-28, nothing to get wrong; rows 2, 3: a common offset of +-100 with
    delocalised biases on top - the same |T lambda| with a median fidelity of 0.1, where an eigenvalue error of a few ulp
    is a phase error of 1e-12 (host build of both modes on these rows: 7e-13 ... 1.1e-12 from the oracle)."""
    N = 7
    rng = np.random.default_rng(7403)
    ctrl = np.empty((C, N + 1))
    ctrl[:, :N] = rng.uniform(-100.0, 100.0, (C, N))
    ctrl[:, N] = 99.0
    ctrl[2:, :N] = np.array([100.0, -100.0])[:, None] + rng.uniform(-1.0, 1.0, (2, N))
    draws = SIGMA * rng.standard_normal((C, K, N, 3))
    want = orc.fidelity_eigh(ctrl, draws, N, 0, N - 1)
    assert (want[2:] > BIG).mean() >= MIN_SHARE
    e_new = np.abs(be.mc_fidelity(ctrl, draws, N, 0, N - 1, kernel="auto") - want).max()
    e_rows = np.abs(be.mc_fidelity(ctrl, draws, N, 0, N - 1, kernel="tridiag_ql") - want).max()
    print(f"|d| ~ 100, T = 99: max|dF| end-to-end {e_new:.3e}  rows mode {e_rows:.3e}")
    assert e_new <= FLOOR, float(e_new)
    assert e_new <= e_rows + 2e-11, (float(e_new), float(e_rows))


def test_close_pair_stays_on_the_wave_wide_route(be):
    """A pair of eigenvalues 1e-6 of the spectral scale apart with O(1) weights on both members, several samples per tile
    (Jacobi matrices with a prescribed spectrum, injected through the draws): parity 1e-10 and no general-path tile."""
    N = 7
    rng = np.random.default_rng(7404)
    ctrl, draws = _deloc(N, 7404)
    ctrl[:, N] = rng.uniform(15, 30, C)
    for c in range(C):
        for k in range(0, K, 9):
            d, e, true, j = _close_pair_matrix(N, 1e-6 * 10.0, rng)      # levels in [-10, 10]: scale 10
            _inject(ctrl[c], draws[c, k], d + rng.uniform(-3, 3), e)
    be.general_path_tiles(reset=True)
    got = be.mc_fidelity(ctrl, draws, N, 0, N - 1, kernel="auto")
    want = orc.fidelity_eigh(ctrl, draws, N, 0, N - 1)
    assert np.abs(got - want).max() <= ABS_TOL, float(np.abs(got - want).max())
    assert be.general_path_tiles() == 0


def test_fused_draws_kernel_is_bit_identical(be):
    import torch
    N, seed = 7, 7405
    ctrl, _ = _deloc(N, seed)
    ct = torch.from_numpy(ctrl).cuda()
    draws = be.philox_normal((C, K, N, 3), seed=seed, scale=SIGMA, as_torch=True)
    plain = be.mc_fidelity(ct, draws, N, 0, N - 1)
    fused = be.mc_fidelity_philox(ct, K, N, 0, N - 1, seed, sigma=SIGMA)
    assert torch.equal(fused, plain)
    want = orc.fidelity_eigh(ctrl, draws.cpu().numpy(), N, 0, N - 1)
    assert np.abs(plain.cpu().numpy() - want).max() <= ABS_TOL
