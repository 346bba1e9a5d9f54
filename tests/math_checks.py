"""Checks of the hand-written fp64 primitives every kernel rests on (csrc/tridiag_core.h: sincos_table, sincos_reduced,
sqrt_rsqrt, rcp_full, the v_rsq_f64 / v_rcp_f64 seeds; csrc/philox_core.inc.h: ln_table, box_muller_pair) against mpmath at 212
bits, evaluated at the exact fp64 inputs - on CHOSEN inputs: every table entry and every tie of the reductions, the ends of the
documented domains, powers of two and their neighbours, the deep tail and the u1 -> 1 end of the logarithm, and the one 53-bit
pattern (a = 2^53 - 1) whose u1 rounds to 1.

Everything is written against ONE callable
    fn(name, x, scale=None) -> (out (n, nout) float64, twin (n, nout) float64 or None)
name / x / out:  "sincos_table" u -> (s, c)     "sincos_reduced" x -> (s, c)     "sqrt_rsqrt" x -> (root, inv)     "rcp_full" x -> (1/x,)
                 "seed_rsq" x -> (y,)   "seed_rcp" x -> (y,)   "ln_table" u -> (ln u,)
                 "box_muller_pair" (n, 2) uint64 (a, b), scale -> (amp, cs, sn, amp * cs, amp * sn)
`twin`: a second build of the same pure-IEEE function (the two sincos routines) that must agree BIT FOR BIT.  Three such callables
exist: `ProbeFn` (tests/host/hip_math_probe.cpp: under hipcc the device with the host compilation of the same binary as twin -
tests/test_gpu_math.py; under g++ the host build of the RC_HD primitives with the NumPy restatement below as twin),
`numpy_fn` (the restatement with an exact fma, which also has ln_table and box_muller_pair - they are device-only code) and its
broken variants (tests/test_math_checks.py), each of which one of the checks must catch.

Inputs are fixed-seed, at most 20 000 per primitive and launch; inputs and references are computed once per process, shared and
read-only.  Every bar is derived in its check's docstring - from the arithmetic, not from what the code returns - and every check
prints and returns the worst case it measured."""
import os
import struct
import subprocess

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "code-robchar_amd", "csrc")
PROBE_SRC = os.path.join(ROOT, "tests", "host", "hip_math_probe.cpp")

U = 2.0 ** -53                      # unit roundoff of fp64: half the spacing in [1, 2), the spacing in [1/2, 1)
PREC = 212
MAX_COUNT = 20000
IDS = {"sincos_table": 0, "sincos_reduced": 1, "sqrt_rsqrt": 2, "rcp_full": 3, "seed_rsq": 4, "seed_rcp": 5, "ln_table": 6,
       "box_muller_pair": 7}
NOUT = {"sincos_table": 2, "sincos_reduced": 2, "sqrt_rsqrt": 2, "rcp_full": 1, "seed_rsq": 1, "seed_rcp": 1, "ln_table": 1,
        "box_muller_pair": 5}
SCALES = (1.0, 0.05)
A_ONE = 2 ** 53 - 1                 # the 53-bit pattern whose u1 = (a + 0.5) 2^-53 rounds to 1.0
ABS_AT_ZERO_RADIUS = 1e-15          # the suite's absolute bar of the generated draws (test_gpu_rng.py)

BAR_SINCOS = 2.0                    # units of 2^-53, absolute
BAR_INV, BAR_ROOT, BAR_RCP = 1.25, 2.25, 1.0        # spacings of the reference
BAR_SEED = 1e-6                     # relative
BAR_LN = 4.0                        # units of 2^-53, relative
BAR_BM = 16.0                       # units of 2^-53 * scale * radius

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        val = make()
        for a in (val if isinstance(val, tuple) else (val,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = val
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------


def _decades(rng, lo, hi, per, signs=True):
    """`per` log-uniform values in every decade [10^d, 10^(d+1)), d = lo .. hi - 1, with both signs"""
    x = np.concatenate([10.0 ** rng.uniform(d, d + 1, per) for d in range(lo, hi)])
    return np.concatenate([x, -x]) if signs else x


def sincos_table_inputs():
    """u (angle in units of pi/32): every decade 1e-3 .. 1e9 with both signs; every integer and half-integer in [-70, 70] (every
    table entry, every tie of rint); the last values of the domain; zeros, 1e-300, a denormal.  Nothing at or beyond 2^31."""
    def make():
        rng = np.random.default_rng(5301)
        edge = [2.0 ** 31 - 1, -(2.0 ** 31 - 1), 2.0 ** 31 - 1.5, 2.0 ** 31 - 0.75, 0.0, -0.0, 1e-300, 5e-324]
        u = np.concatenate([_decades(rng, -3, 9, 250), np.arange(-140, 141) / 2.0, edge])
        assert np.abs(np.rint(u)).max() <= 2.0 ** 31 - 1 and u.size <= MAX_COUNT      # rint(u) is what must fit an int
        return u
    return _once("in sincos_table", make)


def sincos_reduced_inputs():
    """x: every decade 1e-3 .. 1e5 (the routine's documented domain), both signs"""
    return _once("in sincos_reduced", lambda: _decades(np.random.default_rng(5302), -3, 5, 500))


def _magnitudes(rng, n):
    """10^U(-300, 300), 10^U(-8, 8), the powers of two inside [1e-300, 1e300] and their two neighbours; no zero, no denormal"""
    p2 = 2.0 ** np.arange(-996, 997)
    x = np.concatenate([10.0 ** rng.uniform(-300, 300, n), 10.0 ** rng.uniform(-8, 8, n), p2, np.nextafter(p2, 0.0), np.nextafter(p2, np.inf)])
    assert x.min() >= 1e-300 and x.max() <= 1e300
    return x


def sqrt_rsqrt_inputs():
    return _once("in sqrt_rsqrt", lambda: _magnitudes(np.random.default_rng(5303), 2000))


def rcp_full_inputs():
    def make():
        x = _magnitudes(np.random.default_rng(5304), 2000)
        x = np.concatenate([x, -x])
        assert x.size <= MAX_COUNT
        return x
    return _once("in rcp_full", make)


def seed_inputs():
    return _once("in seed", lambda: 10.0 ** np.random.default_rng(5305).uniform(-8, 8, 4000))


def a_list():
    """the 53-bit integers whose u1 sits at the edges of ln_table: the deep tail (0, 1, 2), every power of two and its neighbours
    (change of exponent, first and last table bin), the last values below u1 = 1"""
    a = {0, 1, 2, 2 ** 53 - 2}
    for k in range(1, 53):
        a |= {2 ** k - 1, 2 ** k, 2 ** k + 1}
    a |= {2 ** 53 - 2 ** j for j in range(1, 13)}
    assert max(a) < A_ONE
    return np.array(sorted(a), dtype=np.uint64)


def u_of(a):
    """(a + 0.5) 2^-53 as the device and the definition form it (a + 0.5 rounds for a >= 2^52)"""
    return (np.asarray(a, dtype=np.uint64).astype(np.float64) + 0.5) * 2.0 ** -53


def ln_table_inputs():
    """u: the a list; for each of the 128 table bins the first and the last f of the bin at three exponents; 4 000 random a below
    2^20 (deep tail), 4 000 random a over all 53 bits"""
    def make():
        rng = np.random.default_rng(5306)
        k = np.arange(128)
        f = np.concatenate([0.5 + k / 256.0, np.nextafter(0.5 + (k + 1) / 256.0, 0.0)])
        bins = np.concatenate([f, f * 2.0 ** -1, f * 2.0 ** -30])
        a = np.concatenate([a_list(), rng.integers(0, 2 ** 20, 4000, dtype=np.uint64), rng.integers(0, 2 ** 53, 4000, dtype=np.uint64)])
        a = a[a != A_ONE]
        u = np.concatenate([u_of(a), bins])
        assert u.min() > 0.0 and u.max() < 1.0 and u.size <= MAX_COUNT
        return u
    return _once("in ln_table", make)


def b_list():
    """0 and 2^53 - 1; the quadrant points k 2^51; (2 n + 1) 2^46 - 64 u2 = n + 1/2 + 2^-48, next to the ties of the table
    reduction - for 16 n around the circle; 200 random"""
    rng = np.random.default_rng(5307)
    n = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 61, 62, 63)
    b = [0, 2 ** 53 - 1] + [k * 2 ** 51 for k in range(4)] + [(2 * v + 1) * 2 ** 46 for v in n]
    return np.concatenate([np.array(b, dtype=np.uint64), rng.integers(0, 2 ** 53, 200, dtype=np.uint64)])


B_AT_ONE = (0, 3 * 2 ** 50 + 12345, 2 ** 53 - 1)


def box_muller_inputs():
    """(a, b): the a list crossed with the b list, then a = 2^53 - 1 (u1 == 1) with three values of b - the LAST three rows"""
    def make():
        a, b = a_list(), b_list()
        ab = np.stack([np.repeat(a, b.size), np.tile(b, a.size)], axis=1)
        return np.concatenate([ab, np.array([[A_ONE, v] for v in B_AT_ONE], dtype=np.uint64)])
    return _once("in box_muller_pair", make)


def standard_requests():
    """every (name, x, scale) the checks below ask for - a probe runs them in one process"""
    req = [("sincos_table", sincos_table_inputs(), None), ("sincos_reduced", sincos_reduced_inputs(), None),
           ("sqrt_rsqrt", sqrt_rsqrt_inputs(), None), ("rcp_full", rcp_full_inputs(), None), ("seed_rsq", seed_inputs(), None),
           ("seed_rcp", seed_inputs(), None), ("ln_table", ln_table_inputs(), None)]
    return req + [("box_muller_pair", box_muller_inputs(), s) for s in SCALES]


# ------------------------------------------------------------------------------------------------------------------------
# references (mpmath at PREC bits, kept as an unevaluated sum hi + lo of two doubles: good to ~1e-32 relative) and error measures
# ------------------------------------------------------------------------------------------------------------------------


def _dd(vals):
    hi = np.array([float(v) for v in vals], dtype=np.float64)
    lo = np.array([float(v - mpmath.mpf(h)) for v, h in zip(vals, hi)], dtype=np.float64)
    return hi, lo


def _ref(key, x, funcs):
    """(hi, lo) per function of `funcs`, each applied to the exact value of every double of x"""
    def make():
        with mpmath.workprec(PREC):
            xs = [mpmath.mpf(float(v)) for v in x]
            return tuple(_dd([f(v) for v in xs]) for f in funcs)
    return _once(key, make)


def abs_err(got, ref):
    """|got - (hi + lo)|: got - hi is exact wherever the two are within a factor of two of each other"""
    hi, lo = ref
    return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)


def spacing_of(ref):
    """spacing of the fp64 grid at the exact value hi + lo (at a power of two reached from below: the finer one)"""
    hi, lo = ref
    m, e = np.frexp(np.abs(hi))
    below = (m == 0.5) & (np.sign(lo) * np.sign(hi) < 0)
    return np.ldexp(1.0, e - 53 - below.astype(np.int64))


def _worst(err, x):
    i = int(np.argmax(np.where(np.isnan(err), np.inf, err)))
    return float(err[i]), x[i]


def _report(what, worst, at, bar, unit):
    print(f"math check  {what:<28s} worst {worst:9.4g} {unit} at {at!r}   bar {bar:g}")


def _shape(out, n, name):
    out = np.asarray(out, dtype=np.float64)
    assert out.shape == (n, NOUT[name]), (name, out.shape, n)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------------------------------


def _check_sincos(fn, name, x, ref, bar):
    out, twin = fn(name, x)
    out = _shape(out, x.size, name)
    assert np.isfinite(out).all(), (name, x[~np.isfinite(out).all(axis=1)][:5])
    assert twin is not None, (name, "the bit-for-bit comparison needs a second build of the function")
    twin = _shape(twin, x.size, name)
    same = (out.view(np.uint64) == twin.view(np.uint64)).all(axis=1)
    assert same.all(), (name, "differs from its twin build", int((~same).sum()), x[~same][:5], out[~same][:5], twin[~same][:5])
    res = {}
    for j, part in enumerate(("sin", "cos")):
        err = abs_err(out[:, j], ref[j]) / U
        worst, at = _worst(err, x)
        _report(f"{name} {part}", worst, at, bar, "2^-53 abs")
        assert worst <= bar, (name, part, worst, at)
        res[part] = worst
    return res


def check_sincos_table(fn):
    """(sin, cos)(u pi/32), |u| <= 2^31 - 1.  (1) Bit-identical to the twin build: the routine is a fixed sequence of IEEE
    operations (one rint, one exact subtraction, products, fmas, a table read), so any difference is a contraction the source
    does not have or a different table.  (2) Absolute error <= 2 * 2^-53.  Derivation, in units of 2^-53 = the spacing of the
    results' binade [1/2, 1) (half of it: the rounding error u of one operation there): r = u - n is exact.  s = fma(sh, cl,
    ch sl): the final rounding 1/2; the table entries sh, ch are rounded to nearest, 1/2 each at most, entering weighted
    |cl| <= 1 and |sl| <= pi/64 = 0.05; cl = fma(z, pc, 1) is rounded in [1/2, 1], 1/2, weighted |sh| <= 1; the product ch sl
    and sl's own polynomial carry ~4 roundings RELATIVE to |sl| <= 0.05, 0.1 in all; truncation 5e-18 / 2e-20 is 0.05.  Entry and
    cl cannot both be at their worst with full weight (|sh| = 1 has an exact entry; at 45 degrees both weights are 0.71):
    0.5 + 0.71 (0.5 + 0.5) + 0.25 < 1.5.  Measured on the host build: 1.31.  The bar of 2 leaves 0.5 for what the derivation
    rounds off, not for a wrong entry: ONE entry off by an ulp already fails (1), a dropped Taylor term is 1e3 units."""
    u = sincos_table_inputs()
    ref = _ref("ref sincos_table", u, (lambda v: mpmath.sinpi(v / 32), lambda v: mpmath.cospi(v / 32)))
    return _check_sincos(fn, "sincos_table", u, ref, BAR_SINCOS)


def check_sincos_reduced(fn):
    """sin, cos on the documented domain |x| < 1e5: bit-identical to the twin build, absolute error <= 2 * 2^-53.  Derivation
    (units of 2^-53): n = rint(x 2/pi) <= 6.4e4; r = fma(-n, pio2_hi, x) is ONE rounding of the exact x - n pio2_hi, at most 1/2
    (|r| <= pi/4 < 1), the second fma another 1/2 at most, what pio2_hi + pio2_lo misses of pi/2 times n is 6e4 * 1e-33; the
    fdlibm kernels on |r| <= pi/4 are good to < 1 ulp of the result including their final rounding (0.5 + polynomial ~0.3).  The
    two reduction roundings move the ARGUMENT, which moves the result by at most as much (|sin'|, |cos'| <= 1): 0.5 + 0.5 + 0.8 =
    1.8 with everything at its worst at once.  Measured on the host build: 1.36."""
    x = sincos_reduced_inputs()
    ref = _ref("ref sincos_reduced", x, (mpmath.sin, mpmath.cos))
    return _check_sincos(fn, "sincos_reduced", x, ref, BAR_SINCOS)


def _check_spacings(what, got, ref, x, bar):
    assert np.isfinite(got).all(), (what, x[~np.isfinite(got)][:5])
    err = abs_err(got, ref) / spacing_of(ref)
    worst, at = _worst(err, x)
    _report(what, worst, at, bar, "spacings")
    assert worst <= bar, (what, worst, at)
    return worst


def check_sqrt_rsqrt(fn):
    """sqrt(x), 1/sqrt(x) on [1e-300, 1e300], in spacings of the fp64 grid at the exact value.  Inverse <= 1.25: the third-order
    step leaves 5/16 e^3 ~ 3e-22 before rounding; the roundings of t = x y, of e, q = y e and p = 1/2 + 3/8 e all enter the result
    multiplied by |e| <= 2e-7 (y + q p: q p is a correction of relative size e) - nothing; what is left is the ONE rounding of the
    final fma, 2^-53 relative, which is 1 spacing for a result at the bottom of its binade and 1/2 at the top: 1, plus 0.25 for
    the second-order terms.  Root <= 2.25: root = x * inv inherits inv's relative error (2^-53: up to 1 spacing of the root) and
    adds the rounding of its own product (2^-53 relative: up to 1 more), plus the same 0.25.  Measured on the host build (emulated
    +-5e-8 seeds): 0.97 and 1.62."""
    x = sqrt_rsqrt_inputs()
    ref = _ref("ref sqrt_rsqrt", x, (mpmath.sqrt, lambda v: 1 / mpmath.sqrt(v)))
    out = _shape(fn("sqrt_rsqrt", x)[0], x.size, "sqrt_rsqrt")
    return {"root": _check_spacings("sqrt_rsqrt root", out[:, 0], ref[0], x, BAR_ROOT),
            "inv": _check_spacings("sqrt_rsqrt inv", out[:, 1], ref[1], x, BAR_INV)}


def check_rcp_full(fn):
    """1/x to <= 1 spacing, both signs, |x| in [1e-300, 1e300].  After two Newton steps from a seed good to < 1e-6 the error
    before the last rounding is (1e-6)^4 (nothing) plus the rounding of the residual 1 - x y, which the step multiplies by
    y * 1e-12 (nothing): what is left is the ONE rounding of the final fma, 2^-53 relative = at most 1 spacing at the bottom of
    a binade, 1/2 at its top.  Measured on the host build: 0.50."""
    x = rcp_full_inputs()
    ref = _ref("ref rcp_full", x, (lambda v: 1 / v,))
    out = _shape(fn("rcp_full", x)[0], x.size, "rcp_full")
    return {"rcp": _check_spacings("rcp_full", out[:, 0], ref[0], x, BAR_RCP)}


def check_seeds(fn):
    """The raw v_rsq_f64 / v_rcp_f64 seeds (host build: their +-5e-8 imitation): relative error < 1e-6.  That is what the ONE
    refinement step behind them needs: the third-order step leaves 5/16 e^3 with e = 2 * (seed error) - 5/16 (2e-6)^3 = 2.5e-18,
    a fortieth of 2^-53 - and two Newton steps leave (1e-6)^4.  The measured figure is what tridiag_core.h quotes next to them."""
    x = seed_inputs()
    res = {}
    for name, f in (("seed_rsq", lambda v: 1 / mpmath.sqrt(v)), ("seed_rcp", lambda v: 1 / v)):
        ref = _ref("ref " + name, x, (f,))[0]
        out = _shape(fn(name, x)[0], x.size, name)[:, 0]
        assert np.isfinite(out).all(), name
        err = abs_err(out, ref) / np.abs(ref[0])
        worst, at = _worst(err, x)
        _report(name, worst, at, BAR_SEED, "relative")
        assert worst < BAR_SEED, (name, worst, at)
        res[name] = worst
    return res


def check_ln_table(fn):
    """ln u, u in (0, 1): relative error <= 4 * 2^-53.  Budget, in units of 2^-53 relative to |ln u| >= 2^-52 (u < 1 here; the
    last table bin has c = 1, ln c = 0 exactly and r = f - 1 exact, so u -> 1 keeps RELATIVE accuracy): the table entry ln c_k,
    rounded to nearest: 1/2 at most; r = (f - c_k) * (1/c_k): the rounded 1/c_k and the product, 2 relative to |r| <= |ln u|
    where ln c_k is small and far less elsewhere, halved at least once the entry dominates: 1; the series (five fmas on
    |r| <= 1/128, truncation r^7/8 <= 2^-52 |r| only where |ln f| > 0.3): 1/2; the sum ln c_k + p: 1/2; the final fma with RN(ln 2)
    (off by 0.2 * 2^-53 relative): 1/2 + 0.2.  Sum 3.2 - the terms cannot all be at their largest in one bin."""
    u = ln_table_inputs()
    ref = _ref("ref ln_table", u, (mpmath.log,))[0]
    out = _shape(fn("ln_table", u)[0], u.size, "ln_table")[:, 0]
    assert np.isfinite(out).all(), u[~np.isfinite(out)][:5]
    err = abs_err(out, ref) / np.abs(ref[0]) / U
    worst, at = _worst(err, u)
    _report("ln_table", worst, at, BAR_LN, "2^-53 rel")
    assert worst <= BAR_LN, (worst, at)
    return {"ln": worst}


def _two_prod(a, b):
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def box_muller_reference(scale):
    """(radius as fp64, (hi, lo) of element 0, (hi, lo) of element 1) for `box_muller_inputs()`: scale sqrt(-2 ln u1) (cos, sin)(2 pi u2)
    at the fp64 u1, u2 of the definition - mpmath once per distinct a and per distinct b, the products in double-double"""
    def make():
        ab = box_muller_inputs()
        ua, ia = np.unique(ab[:, 0], return_inverse=True)
        ub, ib = np.unique(ab[:, 1], return_inverse=True)
        with mpmath.workprec(PREC):
            rad = _dd([mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(float(v)))) for v in u_of(ua)])
            u2 = [mpmath.mpf(float(v)) for v in u_of(ub)]
            cs, sn = _dd([mpmath.cospi(2 * v) for v in u2]), _dd([mpmath.sinpi(2 * v) for v in u2])
        rh, rl = rad[0][ia], rad[1][ia]

        def times(t):
            th, tl = t[0][ib], t[1][ib]
            ph, pl = _two_prod(rh, th)
            pl = pl + (rh * tl + rl * th)
            qh, ql = _two_prod(np.full_like(ph, scale), ph)
            ql = ql + scale * pl
            hi = qh + ql
            return hi, (qh - hi) + ql
        return rh.copy(), times(cs), times(sn)
    return _once(("ref box_muller_pair", scale), make)


def philox_host_arithmetic(ab, scale):
    """lines of `oracle.philox_host.philox_normal` behind its Philox call, on given (a, b): elements 0 (cos) and 1 (sin) of each
    pair.  tests/test_math_checks.py holds it against `philox_normal` itself on real stream elements, bit for bit."""
    u1, u2 = u_of(ab[:, 0]), u_of(ab[:, 1])
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 6.283185307179586476925286766559 * u2
    return np.stack([scale * rad * np.cos(ang), scale * rad * np.sin(ang)], axis=1)


def check_box_muller(fn, scale):
    """Both elements of every pair: finite, and |got - ref| <= 16 * 2^-53 * scale * radius_ref; where the reference radius is 0
    (a = 2^53 - 1: u1 == 1) the bar is the suite's 1e-15 absolute.  Derivation (units of 2^-53, relative to scale * radius):
    the radicand -2 ln u carries ln_table's relative error (budget 3.2, bar 4), the root halves it: 2 at most; sqrt_rsqrt's root
    2.25 spacings <= 2.25; the products scale * radius and amp * cos: 1/2 each; the trig factor 1.31 absolute, i.e. 1.31 times
    the radius: 2 + 2.25 + 1 + 1.31 < 8, and the bar is twice that.  The definition itself (`philox_host_arithmetic`: libm log,
    sqrt, 2 pi u2 rounded - half a spacing of an angle up to 6.28 is 4 units - cos / sin) is held to the same bar against
    the same reference, so what the device is compared with elsewhere in the suite is pinned too."""
    ab = box_muller_inputs()
    radius, ref0, ref1 = box_muller_reference(scale)
    bar = np.where(radius > 0.0, BAR_BM * U * scale * radius, ABS_AT_ZERO_RADIUS)
    assert (radius[-len(B_AT_ONE):] == 0.0).all() and (radius[:-len(B_AT_ONE)] > 0.0).all()
    defn = philox_host_arithmetic(ab, scale)
    ratio_def = max(float((abs_err(defn[:, j], r) / bar).max()) for j, r in enumerate((ref0, ref1)))
    _report(f"philox_host arithmetic s={scale:g}", ratio_def, None, 1, "of the bar")
    assert ratio_def <= 1.0, ("the definition disagrees with the reference", ratio_def)
    out = _shape(fn("box_muller_pair", ab, scale)[0], ab.shape[0], "box_muller_pair")
    bad = ~np.isfinite(out).all(axis=1)
    assert not bad.any(), ("not finite", int(bad.sum()), ab[bad][:5], out[bad][:5])
    worst = 0.0
    for j, r in enumerate((ref0, ref1)):
        ratio = abs_err(out[:, 3 + j], r) / bar
        w, at = _worst(ratio, ab)
        _report(f"box_muller_pair[{j}] s={scale:g}", w * BAR_BM, tuple(int(v) for v in at), BAR_BM, "2^-53 s rad")
        assert w <= 1.0, (j, scale, w * BAR_BM, at)
        worst = max(worst, w)
    at_one = np.abs(out[-len(B_AT_ONE):, 3:]).max()
    print(f"math check  u1 == 1: |element| <= {at_one:.3g} (definition: 0; bar {ABS_AT_ZERO_RADIUS:g})")
    return {"ratio": worst * BAR_BM, "definition": ratio_def * BAR_BM, "at_one": float(at_one)}


ALL_CHECKS = (check_sincos_table, check_sincos_reduced, check_sqrt_rsqrt, check_rcp_full, check_seeds, check_ln_table)


# ------------------------------------------------------------------------------------------------------------------------
# the NumPy restatement: every operation of the C++ written out, fma exact
# ------------------------------------------------------------------------------------------------------------------------


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma(a, b, c):
    """a * b + c with ONE rounding (Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums: proved algorithms using
    rounding to odd", IEEE TC 2008, algorithm 5): the product and two sums split exactly, the two small parts added with rounding
    to odd, one final addition.  Exact away from overflow and underflow of the intermediates (|a|, |b| < 2^990, results normal);
    NaN and infinity give NaN (which is what the real fma gives wherever this module feeds them in).  Held against libm's fma by
    tests/test_math_checks.py."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    with np.errstate(all="ignore"):
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, ul)
        vh, vl = _two_sum(uh, th)
        s, e = _two_sum(tl, vl)
        bits = s.copy().view(np.uint64)
        fix = (e != 0.0) & ((bits & np.uint64(1)) == 0) & np.isfinite(s)
        grow = (e > 0.0) == (s > 0.0)                  # the discarded part points away from zero
        bits = np.where(fix & grow, bits + np.uint64(1), np.where(fix & ~grow, bits - np.uint64(1), bits))
        return vh + bits.view(np.float64)


LN2 = 6.93147180559945286227e-01


def _tables():
    """the two constant tables, parsed from the headers the kernels are compiled from"""
    def make():
        def values(path, macro):
            lines = open(os.path.join(CSRC, path)).read().split("#define " + macro, 1)[1].splitlines()
            body = []
            for ln in lines:                               # the macro's continuation lines
                body.append(ln.rstrip().rstrip("\\"))
                if not ln.rstrip().endswith("\\"):
                    break
            return np.array([float(v) for v in " ".join(body).replace(",", " ").split()])
        sc = values("tridiag_core.h", "RC_SINCOS_TABLE_VALUES")
        ln = values("philox_core.inc.h", "RC_LN_TABLE_VALUES")
        assert sc.size == 128 and ln.size == 256, (sc.size, ln.size)
        return sc, ln
    return _once("tables", make)


def np_seed(x, kind):
    """the host build's imitation of the hardware seeds: +-5e-8, sign from a mantissa bit"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        y = 1.0 / np.sqrt(x) if kind == "rsq" else 1.0 / x
        return y * (1.0 + np.where((x.copy().view(np.uint64) & np.uint64(8)) != 0, 5e-8, -5e-8))


def np_sincos_table(u, broken=None):
    """`broken`: "entry" one table entry one ulp off, "taylor" the last Taylor term of the sine dropped, "k31" index & 31"""
    tab = _tables()[0].copy()
    if broken == "entry":
        tab[2 * 9 + 1] = np.nextafter(tab[2 * 9 + 1], 1.0)
    u = np.asarray(u, dtype=np.float64)
    n = np.rint(u)
    r = u - n
    z = r * r
    ps = fma(z, -1.7440893260086657e-11, 7.600081085793214e-08)
    if broken == "taylor":
        ps = np.full_like(z, 7.600081085793214e-08)
    ps = fma(z, ps, -1.577060784927359e-04)
    ps = fma(z, ps, 9.817477042468103e-02)
    sl = r * ps
    pc = fma(z, 2.140319614762968e-13, -1.2435603596778489e-09)
    pc = fma(z, pc, 3.870689512650269e-06)
    pc = fma(z, pc, -4.819142773969413e-03)
    cl = fma(z, pc, 1.0)
    k = n.astype(np.int64) & (31 if broken == "k31" else 63)
    ch, sh = tab[2 * k], tab[2 * k + 1]
    return np.stack([fma(sh, cl, ch * sl), fma(ch, cl, -sh * sl)], axis=1)


def np_sincos_reduced(x):
    x = np.asarray(x, dtype=np.float64)
    n = np.rint(x * 6.36619772367581382433e-01)
    r = fma(-n, 1.57079632679489655800e+00, x)
    r = fma(-n, 6.12323399573676603587e-17, r)
    z = r * r
    ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08)
    for c in (2.75573137070700676789e-06, -1.98412698298579493134e-04, 8.33333333332248946124e-03, -1.66666666666666324348e-01):
        ps = fma(z, ps, c)
    sr = fma(z * r, ps, r)
    pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09)
    for c in (-2.75573143513906633035e-07, 2.48015872894767294178e-05, -1.38888888888741095749e-03, 4.16666666666666019037e-02):
        pc = fma(z, pc, c)
    cr = fma(z * z, pc, fma(z, -0.5, 1.0))
    q = n.astype(np.int64)
    sa, ca = np.where(q & 1, cr, sr), np.where(q & 1, sr, cr)
    return np.stack([np.where(q & 2, -sa, sa), np.where((q + 1) & 2, -ca, ca)], axis=1)


def np_sqrt_rsqrt(x, broken=None):
    """`broken`: "newton" the step without its third-order term (p = 1/2)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        y = np_seed(x, "rsq")
        t = x * y
        e = fma(-t, y, 1.0)
        p = np.full_like(e, 0.5) if broken == "newton" else fma(0.375, e, 0.5)
        q = y * e
        inv = fma(q, p, y)
        return np.stack([x * inv, inv], axis=1)


def np_rcp_full(x, broken=None):
    """`broken`: "one step" a single Newton step"""
    x = np.asarray(x, dtype=np.float64)
    y = np_seed(x, "rcp")
    y = fma(y, fma(-x, y, 1.0), y)
    if broken != "one step":
        y = fma(y, fma(-x, y, 1.0), y)
    return y[:, None]


def np_ln_table(u, broken=None):
    """`broken`: "invc" the 1/c_k of one bin off by 1e-12 relative (a wrong last digit)"""
    tab = _tables()[1].copy()
    if broken == "invc":
        tab[2 * 100 + 1] *= 1.0 + 1e-12
    u = np.asarray(u, dtype=np.float64)
    f, ex = np.frexp(u)
    k = ((f.copy().view(np.uint64) >> np.uint64(32 + 13)) & np.uint64(127)).astype(np.int64)
    ck = 0.5 + (k + 1).astype(np.float64) * 2.0 ** -8
    r = (f - ck) * tab[2 * k + 1]
    p = fma(r, 1.0 / 7.0, -1.0 / 6.0)
    for c in (0.2, -0.25, 1.0 / 3.0, -0.5):
        p = fma(r, p, c)
    p = fma(r * r, p, r)
    return fma(ex.astype(np.float64), LN2, tab[2 * k] + p)[:, None]


def np_box_muller(ab, scale, broken=None):
    """`broken`: "unfixed" the radicand without its nudge (the routine before the fix), "parity" sine and cosine swapped"""
    ab = np.asarray(ab, dtype=np.uint64)
    u1, u2 = u_of(ab[:, 0]), u_of(ab[:, 1])
    lnu = np_ln_table(u1)[:, 0]
    x = -2.0 * lnu if broken == "unfixed" else fma(-2.0, lnu, 2.0 ** -1074)
    rad = np_sqrt_rsqrt(x)[:, 0]
    sc = np_sincos_table(64.0 * u2)
    sn, cs = (sc[:, 1], sc[:, 0]) if broken == "parity" else (sc[:, 0], sc[:, 1])
    with np.errstate(all="ignore"):
        amp = scale * rad
        return np.stack([amp, cs, sn, amp * cs, amp * sn], axis=1)


def numpy_fn(broken=None, twin=None):
    """the restatement as a callable; `broken` = (primitive name, defect) replaces one routine; `twin` supplies the second build
    of the two sincos routines (default: the restatement itself, unbroken)"""
    def fn(name, x, scale=None):
        b = broken[1] if broken and broken[0] == name else None
        if name == "sincos_table":
            return np_sincos_table(x, b), (twin or (lambda n, v: np_sincos_table(v)))(name, x)
        if name == "sincos_reduced":
            return np_sincos_reduced(x), (twin or (lambda n, v: np_sincos_reduced(v)))(name, x)
        if name == "sqrt_rsqrt":
            return np_sqrt_rsqrt(x, b), None
        if name == "rcp_full":
            return np_rcp_full(x, b), None
        if name in ("seed_rsq", "seed_rcp"):
            return np_seed(x, name[5:])[:, None], None
        if name == "ln_table":
            return np_ln_table(x, b), None
        if name == "box_muller_pair":
            return np_box_muller(x, scale, b), None
        raise KeyError(name)
    return fn


# ------------------------------------------------------------------------------------------------------------------------
# tests/host/hip_math_probe.cpp as a callable
# ------------------------------------------------------------------------------------------------------------------------


def build_probe(outdir, compiler):
    """`compiler` = path of hipcc (device build, gfx950) or "g++" (host build of the RC_HD primitives); returns the program"""
    exe = os.path.join(str(outdir), "hip_math_probe")
    if os.path.basename(compiler).startswith("hipcc"):
        cmd = [compiler, "-O1", "--offload-arch=gfx950", "-I", CSRC, "-o", exe, PROBE_SRC]
    else:
        cmd = [compiler, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe, PROBE_SRC]
    subprocess.run(cmd, check=True)
    return exe


class ProbeFn:
    """Runs the probe program: `prefetch(requests)` evaluates many requests in ONE process (one launch per record, a request of
    more than 20 000 inputs is cut into several records); a call returns the prefetched result for the same inputs or runs the
    program for it.  `twin_of`: callable (name, x) -> array used where the program itself writes no second build (the g++ build)."""

    def __init__(self, exe, workdir, twin_of=None, timeout=120):
        self.exe, self.workdir, self.twin_of, self.timeout = exe, str(workdir), twin_of, timeout
        self.done, self.runs = {}, 0

    @staticmethod
    def _norm(name, x):
        return np.ascontiguousarray(x, dtype=np.uint64 if name == "box_muller_pair" else np.float64)

    @staticmethod
    def _key(name, x, scale):
        return name, None if scale is None else float(scale), x.tobytes()

    def prefetch(self, requests):
        requests = [(name, self._norm(name, x), scale) for name, x, scale in requests]
        requests = [r for r in requests if self._key(*r) not in self.done]
        if not requests:
            return
        parts, plan = [], []
        for name, x, scale in requests:
            n = x.shape[0]
            cuts = list(range(0, n, MAX_COUNT))
            plan.append((name, x, scale, len(cuts)))
            for c in cuts:
                chunk = x[c:c + MAX_COUNT]
                parts.append(struct.pack("<qqd", IDS[name], chunk.shape[0], 0.0 if scale is None else float(scale)) + chunk.tobytes())
        self.runs += 1
        fin = os.path.join(self.workdir, f"math_probe_{self.runs}.in")
        fout = os.path.join(self.workdir, f"math_probe_{self.runs}.out")
        with open(fin, "wb") as f:
            f.write(b"".join(parts))
        # its own time limit (the probe is the only program of these tests that opens the GPU): `timeout` ends it, the
        # subprocess timeout behind it is the backstop
        r = subprocess.run(["timeout", "-k", "10", str(self.timeout), self.exe, fin, fout], capture_output=True, text=True,
                           timeout=self.timeout + 30)
        assert r.returncode == 0, ("hip_math_probe failed", r.returncode, r.stderr[-2000:])
        data = open(fout, "rb").read()
        pos = 0
        for name, x, scale, ncuts in plan:
            first, second = [], []
            for _ in range(ncuts):
                pid, n, nd, nh = struct.unpack_from("<qqqq", data, pos)
                pos += 32
                assert pid == IDS[name] and nd == NOUT[name] and nh in (0, nd), (name, pid, n, nd, nh)
                first.append(np.frombuffer(data, dtype=np.float64, count=n * nd, offset=pos).reshape(n, nd))
                pos += 8 * n * nd
                if nh:
                    second.append(np.frombuffer(data, dtype=np.float64, count=n * nh, offset=pos).reshape(n, nh))
                    pos += 8 * n * nh
            out = np.concatenate(first)
            assert out.shape[0] == x.shape[0], (name, out.shape, x.shape)
            self.done[self._key(name, x, scale)] = (out, np.concatenate(second) if second else None)
        assert pos == len(data), ("trailing bytes in the probe's output", pos, len(data))

    def __call__(self, name, x, scale=None):
        key = self._key(name, self._norm(name, x), scale)
        if key not in self.done:
            self.prefetch([(name, x, scale)])
        out, twin = self.done[key]
        if twin is None and self.twin_of is not None and name in ("sincos_table", "sincos_reduced"):
            twin = self.twin_of(name, x)
        return out, twin


# ------------------------------------------------------------------------------------------------------------------------
# large angles through the fidelity kernels: the spin-j chain, whose fidelity is known in closed form at any T
# ------------------------------------------------------------------------------------------------------------------------

LA_NS = (2, 3, 7, 10)
LA_TARGETS = (1e5, 1e6, 1e7, 1e8, 0.9 * 2.0 ** 31 * np.pi / 32)      # largest |T (lam_k - lam_0)| of a case; the last: 0.9 of the domain
LA_C, LA_K = 3, 65
LA_GS = (0.25, -0.5, 0.125)                                           # one per controller row
LA_FLOOR, LA_PER_ANGLE = 1e-10, 8.0 * U


def spin_chain_closed_form(N, g, dg, T):
    """F(0 -> b), b = 0 .. N - 1, of the spin-j chain with bias slopes g + dg_k at time T, in mpmath at the fp64 inputs:
    ((K, N) float64, largest angle T (N - 1) om over the samples)"""
    from math import comb
    F = np.empty((len(dg), N))
    angle_max = 0.0
    with mpmath.workprec(PREC):
        for k, d in enumerate(dg):
            gk = mpmath.mpf(float(g)) + mpmath.mpf(float(d))
            om = mpmath.sqrt(1 + gk * gk)
            angle_max = max(angle_max, float(om * mpmath.mpf(float(T)) * (N - 1)))
            nz2 = (gk / om) ** 2
            cc = nz2 + (1 - nz2) * mpmath.cos(om * mpmath.mpf(float(T)))
            for b in range(N):
                F[k, b] = float(comb(N - 1, b) * ((1 + cc) / 2) ** (N - 1 - b) * ((1 - cc) / 2) ** b)
    return F, angle_max


def large_angle_case(N, target):
    """Couplings sqrt(n (N - n)) / 2, biases g ((N - 1) / 2 - n): H = Jx + g Jz of a spin (N - 1) / 2, levels equally spaced by
    om = sqrt(1 + g^2), F(0 -> b) = C(N-1, b) ((1 + c) / 2)^(N-1-b) ((1 - c) / 2)^b with c = nz^2 + (1 - nz^2) cos(om T), nz = g / om.
    Row c has g = LA_GS[c]; sample k adds the "draw" dg_k ((N - 1) / 2 - n), dg_k = (k - 32) / 1024, to the diagonal, so every sample
    is a spin-j chain of its own (g + dg_k) and all of g, dg, the half-integers and their products and sums are EXACT in fp64: the
    diagonal the kernel forms is the closed form's, to the bit.  T is set per row so that the largest angle T (N - 1) om over the
    row's samples is `target`.  Returns (ctrl, draws, offdiag, angle_max, {(a, b): reference (C, K)} for a in (0, N - 1), all b):
    the closed form in mpmath at these fp64 inputs (the fp64 closed form and an eigendecomposition lose eps * angle themselves)."""
    def make():
        site = (N - 1) / 2.0 - np.arange(N)
        dg = (np.arange(LA_K) - 32) / 1024.0
        ctrl = np.empty((LA_C, N + 1))
        draws = np.zeros((LA_C, LA_K, N, 3))
        draws[:, :, :, 0] = dg[None, :, None] * site[None, None, :]
        n = np.arange(1, N)
        off = 0.5 * np.sqrt(n * (N - n))
        F0 = np.empty((LA_C, LA_K, N))
        angle_max = 0.0
        for c, g in enumerate(LA_GS):
            om_max = max(np.hypot(1.0, g + dg))
            T = float(target / ((N - 1) * om_max) * (1.0 - 2.0 ** -30 * (c + 1)))
            ctrl[c, :N], ctrl[c, N] = g * site, T
            F0[c], am = spin_chain_closed_form(N, g, dg, T)
            angle_max = max(angle_max, am)
        assert np.array_equal(ctrl[:, :N] + draws[:, 0, :, 0], (np.array(LA_GS)[:, None] + dg[0]) * site[None, :])      # exact diagonal
        assert angle_max * 32 / np.pi < 2.0 ** 31 - 1 and 0.98 * target <= angle_max <= 1.0001 * target
        refs = {}
        for b in range(N):
            refs[0, b] = np.ascontiguousarray(F0[:, :, b])
            refs[N - 1, b] = np.ascontiguousarray(F0[:, :, N - 1 - b])
        for r in refs.values():
            r.setflags(write=False)
        return ctrl, draws, off, angle_max, refs
    return _once(("large angle", N, target), make)


def large_angle_bar(N, angle_max):
    """|dF| <= 1e-10 + 8 * 2^-53 * angle_max * (1 - 1/N).  F = sum_{k,l} w_k w_l cos(th_k - th_l), th_k = T (lam_k - lam_0), so a
    phase error moves F by at most max_{k,l} |d(th_k - th_l)| * sum_{k != l} |w_k w_l|, and sum_{k != l} |w_k w_l| = (sum |w_k|)^2 -
    sum w_k^2 <= 1 - 1/N (Cauchy-Schwarz both ways: sum |w_k| <= 1 for products of two rows of an orthogonal matrix) - that is
    the N-dependent factor, 1/2 at N = 2.  The phase: lam_k - lam_0 is one rounding (2^-53 relative, the difference of the two
    largest being the largest angle), its product with the rounded T 32/pi two more, the eigenvalues themselves - a backward
    stable QL / a Halley-polished root of the Sturm recurrence - a few 2^-53 ||H|| = a few 2^-53 angle_max / 2 each, the rounded
    couplings sqrt(n (N - n)) / 2 another 2^-53 angle_max / 2: about 6 * 2^-53 angle_max in all; the bar has 8.  The floor 1e-10
    is the suite's bound at small angles (weights, everything that does not grow with T)."""
    return LA_FLOOR + LA_PER_ANGLE * angle_max * (1.0 - 1.0 / N)


def check_large_angles(fid, N, target, kernels=("auto",)):
    """`fid(ctrl, draws, N, a, b, offdiag, kernel) -> (C, K)`: every kernel, from both ends to every site, against the closed form.
    Guard on the reference alone: its median over the case is >= 1e-2 (zeros cannot pass).  Returns the worst |dF| / bar."""
    ctrl, draws, off, angle_max, refs = large_angle_case(N, target)
    bar = large_angle_bar(N, angle_max)
    worst = 0.0
    for a in (0, N - 1):
        med = float(np.median(np.concatenate([refs[a, b].ravel() for b in range(N)])))
        assert med >= 1e-2, ("the reference cannot tell a wrong kernel from a right one", N, a, target, med)
        for kern in kernels:
            for b in range(N):
                got = np.asarray(fid(ctrl, draws, N, a, b, off, kern), dtype=np.float64)
                assert got.shape == (LA_C, LA_K) and np.isfinite(got).all(), (N, a, b, kern, target)
                err = float(np.abs(got - refs[a, b]).max())
                worst = max(worst, err / bar)
                assert err <= bar, (N, a, b, kern, target, err, bar)
    print(f"math check  large angles N={N:<2d} angle_max {angle_max:.4g}: worst |dF| / bar = {worst:.3g} (bar {bar:.3g})")
    return worst
