"""The workspace plan of the blocking entries (code-robchar_amd/csrc/ws_plan.h: which of a call's arrays take space in the device
workspace, where, how much in all) compiled for the host with g++ (tests/host/host_ws_plan.cpp) - runs without a GPU.  A plan whose
total and offsets disagree makes a kernel write past the workspace; here every way of declaring up to six slots is carved and the
carving is held to the properties below.  The same properties must reject a hand-kept sum-and-walk pair with a slip in it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# how a slot is declared (host_ws_plan.cpp's numbering)
IN_HOST, IN_DEV, OUT_ABSENT, OUT_HOST, OUT_DEV, OUT_ALWAYS_HOST, OUT_ALWAYS_DEV, OUT_ALWAYS_ABSENT, SCRATCH = range(9)
STAGED = (IN_HOST, OUT_HOST, OUT_ALWAYS_HOST, OUT_ALWAYS_DEV, SCRATCH)      # take space in the workspace
IN_PLACE = (IN_DEV, OUT_DEV)                                                # the kernel gets the caller's pointer
ABSENT = (OUT_ABSENT, OUT_ALWAYS_ABSENT)                                    # the kernel gets NULL
SIZES = np.array([0, 1, 255, 256, 257, 65 * 8, (1 << 20) + 8], dtype=np.uint64)
WS = 0x10000000                                   # the workspace's address: 256-aligned, as hipMalloc's are
USER = 0x700000000000                             # the callers' arrays: far from the workspace, one address per slot


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    out = tmp_path_factory.mktemp("wsplan") / "librc_wsplan.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out),
                    os.path.join(ROOT, "tests", "host", "host_ws_plan.cpp")], check=True)
    return ctypes.CDLL(str(out))


def carve(lib, kind, nbytes, slip=0):
    """ptr [M][n], total [M] of the M plans of n slots declared by kind / nbytes [M][n]"""
    kind = np.ascontiguousarray(kind, dtype=np.int32)
    nbytes = np.ascontiguousarray(nbytes, dtype=np.uint64)
    M, n = kind.shape
    user = np.ascontiguousarray(np.broadcast_to(USER + 0x10000000 * np.arange(n, dtype=np.uint64), (M, n)))
    ptr, total = np.full((M, n), 0xdead, dtype=np.uint64), np.full(M, 0xdead, dtype=np.uint64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.rc_host_ws_plans(slip, ctypes.c_longlong(M), n, vp(kind), vp(nbytes), vp(user), ctypes.c_uint64(WS), vp(ptr), vp(total))
    assert rc == 0
    return user, ptr, total


def check(kind, nbytes, user, ptr, total):
    """the properties of a sound carving, for M plans at once"""
    kind, n = np.asarray(kind), kind.shape[1]
    nbytes, total = nbytes.astype(np.int64), total.astype(np.int64)
    staged, off = np.isin(kind, STAGED), ptr.astype(np.int64) - WS
    up = (nbytes + 255) // 256 * 256
    assert (off[staged] >= 0).all() and (off[staged] % 256 == 0).all(), "a staged slot is not 256-aligned"
    for i in range(n):
        for j in range(i + 1, n):
            both = staged[:, i] & staged[:, j]
            assert (off[both, j] >= off[both, i] + nbytes[both, i]).all(), "staged slots overlap or are out of declaration order"
    assert ((off + nbytes)[staged] <= np.broadcast_to(total[:, None], off.shape)[staged]).all(), "a staged slot ends past the total"
    assert np.array_equal(total, np.where(staged, up, 0).sum(axis=1)), "the total is not the sum of the rounded staged sizes"
    in_place = np.isin(kind, IN_PLACE)
    assert np.array_equal(ptr[in_place], user[in_place]), "an in-place slot does not return the caller's pointer"
    assert (ptr[np.isin(kind, ABSENT)] == 0).all(), "an absent output does not yield NULL"


def all_kinds(n):
    """every way of declaring n slots: [9^n][n]"""
    return np.indices((9,) * n).reshape(n, -1).T


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_every_declaration(hostlib, n):
    kind = all_kinds(n)
    rng = np.random.default_rng(n)
    for rep in range(2):
        nbytes = SIZES[rng.integers(0, len(SIZES), kind.shape)]
        check(kind, nbytes, *carve(hostlib, kind, nbytes))


def test_every_declaration_with_every_size(hostlib):
    """one and two slots: every (declaration, size) combination"""
    for n in (1, 2):
        both = np.indices((9, len(SIZES)) * n).reshape(2 * n, -1).T
        kind, nbytes = both[:, 0::2], SIZES[both[:, 1::2]]
        check(kind, nbytes, *carve(hostlib, kind, nbytes))


def test_in_place_and_absent_slots_take_no_space(hostlib):
    kind = np.array([[IN_DEV, OUT_ABSENT, OUT_DEV, OUT_ALWAYS_ABSENT, IN_HOST, OUT_HOST]])
    nbytes = np.array([[257, 257, 257, 257, 257, 1]], dtype=np.uint64)
    user, ptr, total = carve(hostlib, kind, nbytes)
    assert ptr[0].tolist() == [user[0, 0], 0, user[0, 2], 0, WS, WS + 512] and total[0] == 768


@pytest.mark.parametrize("slip,message", [(1, "not 256-aligned"), (2, "ends past the total")])
def test_the_checks_reject_a_wrong_carving(hostlib, slip, message):
    """the hand-kept sum and walk of host_ws_plan.cpp with a slip in the walk: 1 = one slot not rounded, 2 = the walk forgets
    the `absent` condition that the sum has"""
    kind = all_kinds(3)
    nbytes = SIZES[np.random.default_rng(0).integers(0, len(SIZES), kind.shape)]
    check(kind, nbytes, *carve(hostlib, kind, nbytes, slip=0))
    with pytest.raises(AssertionError, match=message):
        check(kind, nbytes, *carve(hostlib, kind, nbytes, slip=slip))
    if slip == 2:         # (an absent output alone, where nothing ends past the total: it must still come out as NULL)
        kind, nbytes = np.array([[OUT_ABSENT]]), np.array([[0]], dtype=np.uint64)
        with pytest.raises(AssertionError, match="does not yield NULL"):
            check(kind, nbytes, *carve(hostlib, kind, nbytes, slip=2))
