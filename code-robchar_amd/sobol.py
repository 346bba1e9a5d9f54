"""Scrambled Sobol points and their normals: the DEFINITION the device reproduces (csrc/sobol_core.h, rc_draws_sobol_f64_async,
rc_mc_fidelity_sobol_f64_async) - bit for bit for the integer points, to a few ulp for the normals.  NumPy only.

Point.  Dimension d, point index n (0 <= n < 2^32), direction numbers v[d][0..31] (uint32, bit 31 = first binary digit):

    x = XOR over the set bits j of gray(n) = n ^ (n >> 1) of v[d][j],   then  x ^= shift[d]

- the Gray-code order of SciPy and torch, evaluated by random access.
Uniform and normal.  u = (x + 0.5) 2^-32 in (0, 1), exact in fp64;  z = Phi^-1(u), |z| <= 6.34;  draw = fl(sigma z).
Sample map.  Sample k of controller row c belongs to replicate r = k // P and is point n = skip + (k mod P) of that replicate;
its D = 3 N coordinates are dimension 3 i + s for site i, slot s - the draw layout [C][K][N][3].  Tables: dirnum[R][D][32],
shift[Cs][R][D], read at row c (Cs = C) or at row 0 (Cs = 1: common random numbers across controllers).
Contract (anything else is refused, RC_EINVAL in the C entries): 1 <= D <= 96, R >= 1, K <= R P, skip % 64 == 0, P % 64 == 0
whenever R > 1, skip + min(P, K) <= 2^32.

Scrambling (`scramble`): per (replicate, dimension) a random lower-triangular 32 x 32 bit matrix with unit diagonal applied to
every v[d][j] over GF(2) (linear matrix scrambling: it keeps the net property of every dimension), then a random 32-bit digital
shift.  All random bits come from np.random.Generator(np.random.Philox(key=seed)) in this order:

    1.  cols  = integers(0, 2^32, size=(R, D, 32), dtype=uint32)    column l of matrix (r, d): binary digit l (bit 31 - l) is the
                                                                    unit diagonal, the digits below it (bits 30 - l .. 0) are
                                                                    the random word's, the digits above it are zero
    2.  shift = integers(0, 2^32, size=(C or 1, R, D), dtype=uint32)
"""
from __future__ import annotations

import ctypes

import numpy as np

MAX_DIM = 96                         # RC_SOBOL_MAX_DIM of include/robchar_hip.h


def direction_numbers(D: int) -> np.ndarray:
    """The unscrambled Joe-Kuo table uint32 [D][32], from the library's host-only entry `rc_sobol_dirnum_u32`."""
    from . import _lib
    D = int(D)
    if not (1 <= D <= MAX_DIM):
        raise ValueError(f"D must be in [1, {MAX_DIM}]")
    out = np.empty((D, 32), dtype=np.uint32)
    _lib.check(_lib.load().rc_sobol_dirnum_u32(D, ctypes.c_void_p(out.ctypes.data)))
    return out


def scramble_matrices(cols: np.ndarray) -> np.ndarray:
    """Random words -> the columns of lower-triangular unit-diagonal bit matrices: column l keeps the word's bits below bit
    31 - l and gets bit 31 - l set (see the module text)."""
    l = np.arange(32, dtype=np.uint64)
    diag = (np.uint64(1) << (np.uint64(31) - l))
    return ((cols.astype(np.uint64) & (diag - np.uint64(1))) | diag).astype(np.uint32)


def apply_matrices(v: np.ndarray, columns: np.ndarray) -> np.ndarray:
    """M v over GF(2) for every direction number: v [D][32] (or [R][D][32]), columns [R][D][32] -> [R][D][32]; digit l of a
    word v[d][j] (bit 31 - l) adds column l of matrix (r, d)."""
    v = np.broadcast_to(np.asarray(v, dtype=np.uint32), columns.shape)
    out = np.zeros(columns.shape, dtype=np.uint32)
    for l in range(32):
        digit = ((v >> np.uint32(31 - l)) & np.uint32(1)).astype(bool)          # [R][D][32 (j)]
        out ^= np.where(digit, columns[..., l:l + 1], np.uint32(0)).astype(np.uint32)
    return out


def scramble(D: int, R: int, seed: int, C=None, base=None):
    """-> (dirnum uint32 [R][D][32], shift uint32 [C or 1][R][D]): R independently scrambled copies of the first D dimensions
    (`base`: another unscrambled table [D][32] than `direction_numbers(D)`)."""
    D, R = int(D), int(R)
    if not (1 <= D <= MAX_DIM) or R < 1:
        raise ValueError(f"D must be in [1, {MAX_DIM}] and R >= 1")
    rng = np.random.Generator(np.random.Philox(key=int(seed)))
    cols = rng.integers(0, 2 ** 32, size=(R, D, 32), dtype=np.uint32)
    shift = rng.integers(0, 2 ** 32, size=(1 if C is None else int(C), R, D), dtype=np.uint32)
    v = direction_numbers(D) if base is None else np.asarray(base, dtype=np.uint32)
    return apply_matrices(v, scramble_matrices(cols)), shift


def check_contract(D, R, P, skip, K):
    D, R, P, skip, K = (int(a) for a in (D, R, P, skip, K))
    if not (1 <= D <= MAX_DIM):
        raise ValueError(f"D must be in [1, {MAX_DIM}]")
    if R < 1 or P < 1 or K < 0 or K > R * P:
        raise ValueError("R >= 1, P >= 1 and 0 <= K <= R P")
    if skip < 0 or skip % 64:
        raise ValueError("skip must be a non-negative multiple of 64")
    if R > 1 and P % 64:
        raise ValueError("P must be a multiple of 64 when R > 1")
    if skip + min(P, K) > 2 ** 32:
        raise ValueError("skip + min(P, K) must not exceed 2^32")


def points(dirnum, shift, P: int, K: int, skip: int = 0, C=None) -> np.ndarray:
    """The scrambled integer points uint32 [C][K][D]: dirnum [R][D][32] (or [D][32]: one replicate), shift [Cs][R][D] with
    Cs = 1 (every row reads row 0) or Cs = C, or None (no shift); C defaults to Cs."""
    dirnum = np.asarray(dirnum, dtype=np.uint32)
    if dirnum.ndim == 2:
        dirnum = dirnum[None]
    R, D, _ = dirnum.shape
    if shift is None:
        shift = np.zeros((1, R, D), dtype=np.uint32)
    shift = np.asarray(shift, dtype=np.uint32).reshape(-1, R, D)
    C = shift.shape[0] if C is None else int(C)
    if shift.shape[0] not in (1, C):
        raise ValueError("shift: [1][R][D] or [C][R][D]")
    check_contract(D, R, P, skip, K)
    k = np.arange(int(K), dtype=np.uint64)
    r = (k // np.uint64(P)).astype(np.int64)
    n = np.uint64(skip) + k % np.uint64(P)
    g = n ^ (n >> np.uint64(1))
    x = np.zeros((int(K), D), dtype=np.uint32)
    for j in range(32):
        bit = ((g >> np.uint64(j)) & np.uint64(1)).astype(bool)
        x ^= np.where(bit[:, None], dirnum[r, :, j], np.uint32(0)).astype(np.uint32)
    rows = shift[:, r, :]                                                       # [Cs][K][D]
    return np.ascontiguousarray(np.broadcast_to(x[None] ^ rows, (C, int(K), D)))


# ---- Phi^-1: Wichura's AS 241 (PPND16), restated with the device's branches and coefficients (csrc/sobol_core.h)
# central branch |u - 1/2| <= 0.425: q A(r) / B(r), r = 0.180625 - q^2; tails: C(t) / D(t), t = sqrt(-ln p) - 1.6, p = min(u, 1 - u).
# p >= 2^-33 here, so sqrt(-ln p) <= 4.79: AS 241's far-tail branch (sqrt(-ln p) > 5) is never reached and is left out.
PPND_A = (3.3871328727963666080e0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
          4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3)
PPND_B = (1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3,
          2.1213794301586595867e+4, 3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3)
PPND_C = (1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
          1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
PPND_D = (1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1,
          1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
PPND_SPLIT = 0.425


def _horner(coef, r):
    acc = np.full_like(r, coef[7])
    for c in coef[6::-1]:
        acc = acc * r + c
    return acc


def normal_from_bits(x) -> np.ndarray:
    """z = Phi^-1((x + 0.5) 2^-32) for uint32 words x, as the device evaluates it: the word is folded to the lower half
    (xm = x < 2^31 ? x : ~x, p = (xm + 0.5) 2^-32 <= 1/2, both exact), |z| is computed from p alone and the sign comes from the
    word's top bit - so z(~x) == -z(x) bit for bit."""
    x = np.asarray(x, dtype=np.uint32)
    upper = x >= np.uint32(0x80000000)
    xm = np.where(upper, ~x, x)
    p = (xm.astype(np.float64) + 0.5) * 2.0 ** -32
    qa = 0.5 - p                                                                # |u - 1/2|, exact
    central = qa <= PPND_SPLIT
    r = np.where(central, 0.180625 - qa * qa, 0.0)
    za = _horner(PPND_A, r) * qa / _horner(PPND_B, r)
    t = np.sqrt(-np.log(np.where(central, 0.25, p))) - 1.6
    zt = _horner(PPND_C, t) / _horner(PPND_D, t)
    z = np.where(central, za, zt)
    return np.where(upper, z, -z)


def normals(dirnum, shift, P: int, K: int, skip: int = 0, sigma=1.0, C=None) -> np.ndarray:
    """fl(sigma_c z) fp64 [C][K][D] of `points(...)`: sigma a float or a (C,) array."""
    z = normal_from_bits(points(dirnum, shift, P, K, skip, C))
    sigma = np.asarray(sigma, dtype=np.float64)
    return (sigma.reshape(-1, 1, 1) if sigma.ndim else sigma) * z
