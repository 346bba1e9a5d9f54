"""code-robchar_amd/sobol.py, the definition of the scrambled Sobol stream the device reproduces: the committed direction-number
header against the installed SciPy, the unscrambled points against scipy.stats.qmc.Sobol bit for bit, the net property of every
scrambled replicate (and a stand-in scrambler that must fail it), random access, and the NumPy restatement of the device's Phi^-1:
exact antisymmetry and its error against mpmath at 50 digits.  Runs without a GPU (the table comes from the library's host entry).

Phi^-1 measured here (the whole set of `probe_words`): worst relative error 7.12e-16 against mpmath (central branch 7.12e-16, tail
branch 6.49e-16; worst absolute error 1.8e-15) - AS 241's own approximation error (1e-16) plus the rounding of ~20 operations.
The mpmath values of the whole set are kept in tests/golden/sobol_phi_inv_ref.npy (47 s to recompute: `python
tests/test_sobol_definition.py --write-golden`); the test recomputes the chosen words and a random thousand of the rest - a different
thousand on every run - with mpmath and compares the file with them bit for bit, then uses the file for all 100 076 words."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sobol = importlib.import_module("code-robchar_amd.sobol")


def probe_words(n_random=100_000, seed=7):
    """x = 0, 2^32 - 1, both sides of the branch boundary |u - 1/2| = 0.425, all powers of two and their complements, random words
    (shared with tests/test_gpu_sobol.py)"""
    edge = int(np.floor(0.075 * 2 ** 32 - 0.5))               # p = (x + 0.5) 2^-32 crosses 0.075 between edge and edge + 1
    words = [0, 2 ** 32 - 1] + [edge + d for d in (-1, 0, 1, 2)] + [2 ** j for j in range(32)]
    words = np.array(words, dtype=np.uint32)
    rnd = np.random.Generator(np.random.Philox(key=seed)).integers(0, 2 ** 32, size=n_random, dtype=np.uint32)
    both = np.concatenate([words, ~words, rnd])
    return both


def phi_inv_reference(words):
    """Phi^-1((x + 0.5) 2^-32) by mpmath at 50 digits, rounded to fp64; the lower half is evaluated and mirrored"""
    import mpmath
    mpmath.mp.dps = 50
    words = np.asarray(words, dtype=np.uint32)
    upper = words >= 2 ** 31
    folded = np.where(upper, ~words, words)
    uniq, inv = np.unique(folded, return_inverse=True)
    root2 = mpmath.sqrt(2)
    ref = np.array([float(-root2 * mpmath.erfinv(1 - 2 * (mpmath.mpf(int(x)) + mpmath.mpf(1) / 2) / 2 ** 32)) for x in uniq])
    return np.where(upper, -ref[inv], ref[inv])


GOLDEN = os.path.join(ROOT, "tests", "golden", "sobol_phi_inv_ref.npy")
N_CHOSEN = 2 * 38                                           # the chosen words and their complements lead `probe_words`


def checked_reference(words):
    """the golden mpmath values of `probe_words()`, after a live mpmath check of the chosen words and of 1000 random ones - another
    thousand on every run (the seed is drawn from the run and printed), so that no fixed part of the file goes unchecked"""
    ref = np.load(GOLDEN)
    assert ref.shape == words.shape
    seed = int(np.random.SeedSequence().entropy)
    print(f"golden Phi^-1 reference: live mpmath check of the {N_CHOSEN} chosen words and 1000 random ones, subset seed {seed}")
    pick = np.concatenate([np.arange(N_CHOSEN), N_CHOSEN + np.random.default_rng(seed).choice(len(words) - N_CHOSEN, 1000, replace=False)])
    assert np.array_equal(phi_inv_reference(words[pick]), ref[pick]), seed
    return ref


def test_committed_header_is_what_scipy_gives():
    pytest.importorskip("scipy")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        mk = importlib.import_module("make_sobol_table")
    finally:
        sys.path.pop(0)
    assert open(mk.HEADER).read() == mk.header_text()
    assert np.array_equal(sobol.direction_numbers(96), mk.table(96))


@pytest.mark.parametrize("D", (6, 21, 96))
def test_unscrambled_points_equal_scipy_bit_for_bit(D):
    qmc = pytest.importorskip("scipy.stats.qmc")
    want = qmc.Sobol(D, scramble=False, bits=32).random(4096) * 2.0 ** 32
    got = sobol.points(sobol.direction_numbers(D), None, P=4096, K=4096)
    assert got.shape == (1, 4096, D) and got.dtype == np.uint32
    assert np.array_equal(got[0].astype(np.float64), want)


def one_per_interval(x, m):
    """do the first 2^m words fall one per interval of width 2^-m (per trailing axis entry)?  x: [2^m][...] uint32"""
    cells = np.sort(x[: 2 ** m] >> np.uint32(32 - m), axis=0)
    return np.array_equal(cells, np.broadcast_to(np.arange(2 ** m, dtype=np.uint32).reshape((-1,) + (1,) * (x.ndim - 1)), cells.shape))


def test_net_property_of_every_scrambled_replicate_and_a_scrambler_that_breaks_it():
    D, R = 39, 5
    dirnum, shift = sobol.scramble(D, R, seed=2024, C=3)
    assert dirnum.shape == (R, D, 32) and shift.shape == (3, R, D) and dirnum.dtype == shift.dtype == np.uint32
    assert not np.array_equal(dirnum[0], dirnum[1]) and not np.array_equal(dirnum[0], sobol.direction_numbers(D))
    x = sobol.points(dirnum, shift, P=4096, K=R * 4096)                    # [3][R 4096][D]
    for c in range(3):
        per_rep = x[c].reshape(R, 4096, D).transpose(1, 0, 2)              # [4096][R][D]
        for m in range(6, 13):
            assert one_per_interval(per_rep, m), (c, m)
    # a stand-in scrambler: the same random words used as FULL matrix columns (not triangular) - singular leading blocks
    rng = np.random.Generator(np.random.Philox(key=2024))
    cols = rng.integers(0, 2 ** 32, size=(R, D, 32), dtype=np.uint32)
    bad = sobol.apply_matrices(sobol.direction_numbers(D), cols)
    xb = sobol.points(bad, None, P=4096, K=R * 4096)[0].reshape(R, 4096, D).transpose(1, 0, 2)
    assert not all(one_per_interval(xb, m) for m in range(6, 13))
    # same seed, same tables; another seed, other tables
    again = sobol.scramble(D, R, seed=2024, C=3)
    assert np.array_equal(again[0], dirnum) and np.array_equal(again[1], shift)
    assert not np.array_equal(sobol.scramble(D, R, seed=2025, C=3)[0], dirnum)
    # the shifts of C = None are those of row 0 (common random numbers)
    assert np.array_equal(sobol.scramble(D, R, seed=2024)[1][0], shift[0])


@pytest.mark.parametrize("skip", (64, 320, 2 ** 20 + 64))
def test_random_access_with_skip_equals_slicing(skip):
    D = 21
    dirnum, shift = sobol.scramble(D, 1, seed=5)
    if skip < 4096:
        whole = sobol.points(dirnum, shift, P=4096, K=4096)
        assert np.array_equal(sobol.points(dirnum, shift, P=4096 - skip, K=1000, skip=skip)[0], whole[0, skip:skip + 1000])
    # a far point against the recurrence x_{n+1} = x_n ^ v[ctz(n + 1)]
    far = sobol.points(dirnum, shift, P=256, K=256, skip=skip)[0]
    for i in range(255):
        n1 = skip + i + 1
        j = (n1 & -n1).bit_length() - 1
        assert np.array_equal(far[i + 1], far[i] ^ dirnum[0, :, j])
    # replicates: sample k is point skip + k mod P of replicate k // P
    d2, s2 = sobol.scramble(D, 3, seed=6)
    x = sobol.points(d2, s2, P=64, K=192, skip=skip)
    for r in range(3):
        assert np.array_equal(x[0, 64 * r:64 * r + 64], sobol.points(d2[r], s2[:, r:r + 1], P=64, K=64, skip=skip)[0])


def test_contract_is_refused():
    d, s = sobol.scramble(6, 2, seed=1)
    for kw in (dict(P=100, K=100), dict(P=64, K=129), dict(P=64, K=64, skip=32), dict(P=128, K=128, skip=2 ** 32 - 64)):
        with pytest.raises(ValueError):
            sobol.points(d, s, **kw)
    assert sobol.points(d[:1], s[:, :1], P=100, K=100).shape == (1, 100, 6)       # R = 1: any P
    assert sobol.points(d, s, P=128, K=200, skip=2 ** 32 - 128).shape == (1, 200, 6)
    with pytest.raises(ValueError):
        sobol.direction_numbers(97)


def test_phi_inverse_is_exactly_odd_and_close_to_mpmath():
    pytest.importorskip("mpmath")
    words = probe_words()
    z = sobol.normal_from_bits(words)
    assert np.array_equal(sobol.normal_from_bits(~words), -z)
    assert np.all(np.isfinite(z)) and 6.33 < np.abs(z).max() < 6.34
    assert z[0] < 0 < z[1]                                                # x = 0: u = 2^-33, z = -6.338; x = 2^32 - 1: +6.338
    ref = checked_reference(words)
    rel = np.abs(z - ref) / np.abs(ref)
    print(f"Phi^-1 (NumPy restatement) vs mpmath: worst relative error {rel.max():.3e} at word {int(words[rel.argmax()])}")
    assert rel.max() < 1e-15                                              # measured 7.12e-16 (module text)
    assert np.all(np.abs(z - ref) <= 1e-13 * np.maximum(1.0, np.abs(ref)))
    # normals(): one rounded product per element
    d, s = sobol.scramble(6, 1, seed=3, C=2)
    sig = np.array([0.05, 0.0])
    dr = sobol.normals(d, s, P=64, K=64, sigma=sig)
    zz = sobol.normal_from_bits(sobol.points(d, s, P=64, K=64))
    assert np.array_equal(dr[0], 0.05 * zz[0]) and np.all(dr[1] == 0.0)


if __name__ == "__main__" and "--write-golden" in sys.argv[1:]:
    np.save(GOLDEN, phi_inv_reference(probe_words()))
