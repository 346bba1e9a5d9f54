"""The checks of tests/math_checks.py have teeth, and their bars hold on the reference side before any GPU run.  CPU only.

(1) Each of eight broken stand-ins - the NumPy restatement of the primitives with one defect: a table entry one ulp off, a dropped
    Taylor term, k & 31, the Householder term missing, one Newton step, 1 / c_k off in one bin, the unfixed u1 == 1, sine and cosine
    swapped - fails the check that is there for it; so do a lost phase and zeros in the large-angle check.
(2) The real checks pass on a g++ host build of the RC_HD primitives (tests/host/hip_math_probe.cpp compiled without HIP: the
    emulated +-5e-8 seeds), whose two sincos routines must equal the NumPy restatement bit for bit, and on the NumPy / exact-fma
    restatement of ln_table and box_muller_pair (device-only code).
(3) The scaffolding itself: the emulated fma against libm's, the restatement against the host build, the restated definition
    against `oracle.philox_host.philox_normal` on real stream elements, the input lists against what they promise."""
import ctypes
import ctypes.util
import shutil

import numpy as np
import pytest

import math_checks as mc
from oracle import philox_host


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the g++ host build of the probe; twin of the sincos routines = the NumPy restatement"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("mathprobe_host")
    nf = mc.numpy_fn()
    fn = mc.ProbeFn(mc.build_probe(d, "g++"), d, twin_of=lambda name, x: nf(name, x)[0])
    fn.prefetch(r for r in mc.standard_requests() if r[0] not in ("ln_table", "box_muller_pair"))
    return fn


# ---- (2) the bars hold on the reference side ---------------------------------------------------------------------------------

@pytest.mark.parametrize("check", [mc.check_sincos_table, mc.check_sincos_reduced, mc.check_sqrt_rsqrt, mc.check_rcp_full, mc.check_seeds],
                         ids=lambda c: c.__name__)
def test_host_build_passes(host, check):
    check(host)


def test_restated_ln_table_passes():
    mc.check_ln_table(mc.numpy_fn())


@pytest.mark.parametrize("scale", mc.SCALES)
def test_restated_box_muller_passes(scale):
    res = mc.check_box_muller(mc.numpy_fn(), scale)
    assert 0.0 < res["at_one"] <= 1e-150     # the nudged radicand: radius sqrt(2^-1074) = 2.2e-162 where the definition has 0


def test_device_only_primitives_are_refused_by_the_host_build(host):
    with pytest.raises(AssertionError, match="device-only"):
        host("ln_table", np.array([0.5]))


# ---- (1) teeth ------------------------------------------------------------------------------------------------------------------

BROKEN = [
    (("sincos_table", "entry"), mc.check_sincos_table, "differs from its twin"),           # a table entry off by 1 ulp
    (("sincos_table", "taylor"), mc.check_sincos_table, "differs from its twin"),          # the last Taylor term dropped
    (("sincos_table", "k31"), mc.check_sincos_table, "differs from its twin"),             # k & 31
    (("sqrt_rsqrt", "newton"), mc.check_sqrt_rsqrt, "sqrt_rsqrt"),                         # the Householder term missing
    (("rcp_full", "one step"), mc.check_rcp_full, "rcp_full"),                             # one Newton step
    (("ln_table", "invc"), mc.check_ln_table, None),                                        # 1 / c_k off in one bin
]


@pytest.mark.parametrize("broken,check,msg", BROKEN, ids=[f"{b[0]}:{b[1]}" for b, _, _ in BROKEN])
def test_broken_primitive_fails_its_check(broken, check, msg):
    with pytest.raises(AssertionError, match=msg):
        check(mc.numpy_fn(broken=broken))


@pytest.mark.parametrize("defect", ["taylor", "k31"])
def test_broken_sincos_fails_the_accuracy_bar_too(defect):
    """without a twin to differ from (a twin with the same defect) the absolute bar alone catches the two large defects; the
    one-ulp table entry is what the bit-for-bit comparison is for"""
    with pytest.raises(AssertionError, match="sincos_table', '(sin|cos)'"):
        mc.check_sincos_table(mc.numpy_fn(broken=("sincos_table", defect), twin=lambda name, x: mc.np_sincos_table(x, defect)))


def test_unfixed_u1_equal_one_fails():
    """the routine as it was before the fix (radicand -2 ln u1 = 0 at a = 2^53 - 1): both elements NaN - caught by the finiteness
    assertion, on exactly the three pairs with that a"""
    out = mc.np_box_muller(mc.box_muller_inputs(), 1.0, "unfixed")
    bad = ~np.isfinite(out).all(axis=1)
    assert bad.sum() == len(mc.B_AT_ONE) and bad[-len(mc.B_AT_ONE):].all() and np.isnan(out[bad][:, 3:]).all()
    with pytest.raises(AssertionError, match="not finite"):
        mc.check_box_muller(mc.numpy_fn(broken=("box_muller_pair", "unfixed")), 1.0)


def test_clamping_u1_would_not_do():
    """u1 clamped to 1 - 2^-53... rounds to 1 - 2^-53's neighbour: radius sqrt(2 * 1.1e-16) = 1.5e-8, far above the 1e-15 the pair
    is held to where the definition's radius is 0"""
    assert np.sqrt(-2.0 * np.log1p(-2.0 ** -53)) > 1e7 * mc.ABS_AT_ZERO_RADIUS


def test_parity_swap_fails():
    with pytest.raises(AssertionError):
        mc.check_box_muller(mc.numpy_fn(broken=("box_muller_pair", "parity")), 0.05)


def test_large_angle_check_catches_a_lost_phase_and_zeros():
    """the closed-form check against (a) fidelities whose phases carry a relative error of 5e-14 (450 * 2^-53: a sloppy
    reduction) - the exact closed form at T (1 + 5e-14) - and (b) zeros"""
    N, target = 3, mc.LA_TARGETS[-1]
    dg = (np.arange(mc.LA_K) - 32) / 1024.0

    def sloppy(ctrl, draws, N, a, b, off, kern):
        F = np.stack([mc.spin_chain_closed_form(N, g, dg, ctrl[c, N] * (1.0 + 5e-14))[0] for c, g in enumerate(mc.LA_GS)])
        return F[:, :, b if a == 0 else N - 1 - b]

    with pytest.raises(AssertionError):
        mc.check_large_angles(lambda *a: np.zeros((mc.LA_C, mc.LA_K)), N, target)
    with pytest.raises(AssertionError):
        mc.check_large_angles(sloppy, N, target)
    exact = lambda ctrl, draws, N, a, b, off, kern: np.stack(
        [mc.spin_chain_closed_form(N, g, dg, ctrl[c, N])[0] for c, g in enumerate(mc.LA_GS)])[:, :, b if a == 0 else N - 1 - b]
    assert mc.check_large_angles(exact, N, target) == 0.0


# ---- (3) scaffolding ----------------------------------------------------------------------------------------------------------

def test_emulated_fma_equals_libm():
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fma.restype, libm.fma.argtypes = ctypes.c_double, [ctypes.c_double] * 3
    rng = np.random.default_rng(77)
    n = 6000
    a = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    b = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    c = -a * b * (1.0 + rng.integers(-3, 4, n) * 2.0 ** -52)                                # heavy cancellation: the low part decides
    c[::3] += rng.standard_normal(n)[::3] * 1e-22 * np.abs(a * b)[::3]                      # ... and something below it (sticky bit)
    c[1::4] = rng.standard_normal(n)[1::4]
    a[:4], b[:4], c[:4] = (-2.0, 1.0, 2.0 ** 52 + 1, 3.0), (0.0, 1e-300, 2.0 ** 52 + 1, 2.0 ** -53), (1e-300, -0.0, -2.0 ** 104, 1.0)
    want = np.array([libm.fma(x, y, z) for x, y, z in zip(a, b, c)])
    got = mc.fma(a, b, c)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), int((got != want).sum())
    assert (got != a * b + c).sum() > n // 10                                              # the cases do tell an fma from two roundings


@pytest.mark.parametrize("name", ["sqrt_rsqrt", "rcp_full", "seed_rsq", "seed_rcp"])
def test_restatement_equals_host_build(host, name):
    """(the two sincos routines: inside their checks, as the twin)"""
    x = {"sqrt_rsqrt": mc.sqrt_rsqrt_inputs(), "rcp_full": mc.rcp_full_inputs()}.get(name, mc.seed_inputs())
    assert np.array_equal(mc.numpy_fn()(name, x)[0].view(np.uint64), host(name, x)[0].view(np.uint64))


def test_restated_ln_of_one_is_exactly_zero():
    """what makes a = 2^53 - 1 special: u1 rounds to 1.0, ln_table(1.0) = +0.0 exactly, the radicand vanishes"""
    assert mc.u_of([mc.A_ONE])[0] == 1.0 and mc.u_of([mc.A_ONE - 1])[0] == 1.0 - 2.0 ** -52
    ln1 = mc.np_ln_table(np.array([1.0]))[0, 0]
    assert ln1 == 0.0 and not np.signbit(ln1)
    # ... and the nudge changes no other radicand: -2 ln u >= 4.4e-16 for every other a
    ln = mc.np_ln_table(mc.ln_table_inputs())[:, 0]
    assert np.array_equal(mc.fma(-2.0, ln, 2.0 ** -1074), -2.0 * ln)
    assert (-2.0 * mc.np_ln_table(mc.u_of(mc.a_list()))[:, 0]).min() >= 4.4e-16


def test_definition_restated_equals_philox_host():
    """`math_checks.philox_host_arithmetic` on the (a, b) of real counters is `philox_normal`, bit for bit"""
    seed, n = 0x1234_5678_9ABC_DEF0, 4096
    ctr = np.arange(n // 2, dtype=np.uint64)
    w0, w1, w2, w3 = philox_host.philox4x32_10(ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)
    a = ((w1.astype(np.uint64) << np.uint64(32)) | w0.astype(np.uint64)) >> np.uint64(11)
    b = ((w3.astype(np.uint64) << np.uint64(32)) | w2.astype(np.uint64)) >> np.uint64(11)
    pairs = mc.philox_host_arithmetic(np.stack([a, b], axis=1), 0.05)
    assert np.array_equal(pairs.ravel(), philox_host.philox_normal(seed, 0, n, 0.05))


def test_the_inputs_hold_what_they_are_there_for():
    u = mc.sincos_table_inputs()
    k = np.rint(u).astype(np.int64) & 63
    assert set(k.tolist()) == set(range(64)) and (np.abs(u - np.rint(u)) == 0.5).sum() >= 140        # every entry, every tie
    assert (np.abs(u) >= 1e8).sum() >= 400 and np.abs(np.rint(u)).max() == 2 ** 31 - 1 and np.signbit(u[u == 0]).sum() == 1 and (u == 5e-324).any()
    assert np.abs(mc.sincos_reduced_inputs()).max() < 1e5
    for x in (mc.sqrt_rsqrt_inputs(), np.abs(mc.rcp_full_inputs())):
        assert x.min() >= 1e-300 and x.max() <= 1e300 and (np.frexp(x)[0] == 0.5).sum() >= 1993
    assert (mc.rcp_full_inputs() < 0).mean() == 0.5
    lu = mc.ln_table_inputs()
    f, e = np.frexp(lu)
    kk = ((f.view(np.uint64) >> np.uint64(45)) & np.uint64(127)).astype(int)
    assert set(kk.tolist()) == set(range(128)) and e.min() <= -52 and lu.max() == 1.0 - 2.0 ** -53 and (lu == 1.0 - 2.0 ** -52).any() and lu.min() == 2.0 ** -54
    ab = mc.box_muller_inputs()
    assert (ab[-3:, 0] == mc.A_ONE).all() and (ab[:-3, 0] != mc.A_ONE).all() and ab.shape[0] == mc.a_list().size * mc.b_list().size + 3
    assert mc.b_list().size == 222 and {0, 2 ** 53 - 1, 2 ** 51, 2 ** 52, 3 * 2 ** 51} <= set(int(v) for v in mc.b_list())
    assert max(len(x) for _, x, _ in mc.standard_requests() if x.ndim == 1) <= mc.MAX_COUNT
