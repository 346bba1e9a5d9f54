"""The checks of tests/tail_select_checks.py have teeth: they pass on the NumPy route of `noise.tail_weights` (the definition), and
each of seven broken selections fails the check that is there for it.  CPU only: NumPy against the independent reference."""
import importlib

import numpy as np
import pytest

import tail_select_checks as tc

noise = importlib.import_module("code-robchar_amd.noise")


def select_numpy(F, alpha):
    lst, w = noise.tail_weights(F, alpha)
    m = lst.shape[1]
    var = np.where(np.isnan(F).any(axis=1), np.nan, np.sort(F, axis=1)[:, m - 1])
    return lst, w, var


def select_broken(broken):
    """`noise.tail_weights` rewritten with one defect:
        "ties high"    ties resolved to the higher index          "minus zero"  -0.0 ordered before +0.0 regardless of index
        "last slot"    w_last on the last slot of the list          "nan kept"    a NaN row not emptied
        "48 bits"      keys compared on their upper 48 bits only    "value order" the list left in value order
        "floor"        m = floor(alpha K) for fractional alpha K"""
    def select(F, alpha):
        C, K = F.shape
        ak = alpha * K
        m = min(K, int(np.ceil(ak)))
        if broken == "floor" and ak != np.floor(ak):
            m = max(1, int(np.floor(ak)))
        w_body, w_last = 1.0 / ak, (ak - (m - 1)) / ak
        idx = np.broadcast_to(np.arange(K), F.shape)
        keys = tc.key_bits(np.where(np.isnan(F), np.inf, F))
        if broken == "ties high":
            order = np.stack([np.lexsort((-idx[c], keys[c])) for c in range(C)])
        elif broken == "48 bits":
            order = np.argsort(keys >> np.uint64(16), axis=1, kind="stable")
        elif broken == "minus zero":
            raw = np.where(np.signbit(F) & (F == 0.0), keys - np.uint64(1), keys)          # -0.0 just below +0.0
            order = np.argsort(raw, axis=1, kind="stable")
        else:
            order = np.argsort(keys, axis=1, kind="stable")
        order = order[:, :m]
        last = order[:, m - 1:m]
        listed = order if broken == "value order" else np.sort(order, axis=1)
        weights = np.where(listed == last, w_last, w_body)
        if broken == "last slot":
            weights = np.full(listed.shape, w_body)
            weights[:, m - 1] = w_last
        var = np.take_along_axis(F, last, 1)[:, 0]
        bad = np.isnan(F).any(axis=1, keepdims=True)
        if broken == "nan kept":
            return listed.astype(np.int32), weights, np.where(bad[:, 0], np.nan, var)
        return np.where(bad, -1, listed).astype(np.int32), np.where(bad, 0.0, weights), np.where(bad[:, 0], np.nan, var)
    return select


@pytest.mark.parametrize("K", tc.RANDOM_K)
@pytest.mark.parametrize("which", range(6), ids=("m=1", "0.03", "0.1", "0.5", "0.95", "1.0"))
def test_random_rows(K, which):
    tc.check_random(select_numpy, ks=(K,), which=(which,))


@pytest.mark.parametrize("check", [c for c in tc.ALL_CHECKS if c is not tc.check_random], ids=lambda c: c.__name__)
def test_numpy_route_passes(check):
    check(select_numpy)


def test_sound_rewrite_passes_the_small_checks():
    """the rewrite the stand-ins are made from is itself right: what fails below fails for its defect"""
    sound = select_broken(None)
    tc.check_random(sound, ks=(1, 2, 63, 257, 1000))
    for check in (tc.check_ties, tc.check_constant_rows, tc.check_last_digit, tc.check_special_values):
        check(sound)


@pytest.mark.parametrize("broken, check, kwargs", [
    ("ties high", tc.check_ties, {"cases": tc.TIE_CASES[:1]}),
    ("last slot", tc.check_random, {"ks": (257,)}),
    ("48 bits", tc.check_last_digit, {}),
    ("minus zero", tc.check_special_values, {}),
    ("nan kept", tc.check_random, {"ks": (257,)}),
    ("value order", tc.check_random, {"ks": (257,)}),
    ("floor", tc.check_random, {"ks": (257,)}),
])
def test_broken_stand_in_fails_its_check(broken, check, kwargs):
    with pytest.raises(AssertionError):
        check(select_broken(broken), **kwargs)


def test_stand_ins_pass_where_their_defect_does_not_show():
    """each defect is what its check catches, not a generally wrong selection: on rows of distinct values with no NaN and no zero,
    at an alpha with integer alpha K, five of the seven are right"""
    F = np.random.default_rng(5).random((3, 200)) + 0.5
    exp = tc.expected(F, 0.1)
    for broken in ("ties high", "48 bits", "minus zero", "nan kept", "floor"):
        tc.compare(select_broken(broken), F, exp, (broken, 200, 0.1))
