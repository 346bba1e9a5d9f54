"""tests/arena.py has teeth: "kernels" that write through the raw pointer of CPU tensors, the way a HIP kernel writes through
`data_ptr()` - a clean one passes every check, and each broken one fails the check meant for it with a message that names
the block, the side and the distance.  (The GPU use is tests/test_gpu_placement.py.)"""
import ctypes

import numpy as np
import pytest
import torch

from arena import SENTINEL, Arena

CANONICAL_NAN = np.uint64(0x7FF8000000000000).view(np.float64)


def poke(t, i, value):
    """store `value` at element offset `i` (negative or past the end allowed) from the first element of `t`, as a kernel would"""
    ctype = {torch.float64: ctypes.c_double, torch.int32: ctypes.c_int32, torch.int64: ctypes.c_int64}[t.dtype]
    ctype.from_address(t.data_ptr() + i * t.element_size()).value = value


def kernel(fid, lst, first=0, stop=None, lst_stop=None, extra=()):
    """the stand-in entry: row 0 of `fid` (2, 5) canonical NaN, row 1 values; `lst` (2, 3) -1 in row 0, indices in row 1.
    `first` / `stop` / `lst_stop`: the element range it covers; `extra`: stray (tensor, offset) stores"""
    n = fid.numel()
    for i in range(first, n if stop is None else stop):
        poke(fid, i, CANONICAL_NAN if i < 5 else 0.25 * i)
    for i in range(lst.numel() if lst_stop is None else lst_stop):
        poke(lst, i, -1 if i < 3 else i)
    for t, off in extra:
        poke(t, off, 1.5 if t.dtype == torch.float64 else 7)


def run(shift, guard=64, **broken):
    arena = Arena(guard=guard, shift=shift, device="cpu")
    fid = arena.empty((2, 5), dtype=torch.float64, device="cpu")
    lst = arena.empty(2, 3, dtype=torch.int32, device="cpu")
    stray = {"fid": fid, "lst": lst}
    extra = [(stray[k], off) for k, off in broken.pop("extra", ())]
    kernel(fid, lst, extra=extra, **broken)
    arena.check_guards()
    arena.assert_written(fid, "fid")
    arena.assert_written(lst, "lst")
    return arena, fid, lst


@pytest.mark.parametrize("shift", (0, 1))
def test_clean_stand_in_passes(shift):
    arena, fid, lst = run(shift)
    assert np.isnan(fid[0].numpy()).all() and (lst[0].numpy() == -1).all()           # NaN rows and empty lists are not sentinels
    assert fid.is_contiguous() and fid.storage_offset() == 64 + shift and fid.data_ptr() % 16 == 8 * shift


@pytest.mark.parametrize("shift", (0, 1))
@pytest.mark.parametrize("broken, message", [
    (dict(first=-1), r"guard overwritten: block #0 empty float64\[2, 5\], before the body, 1 word\(s\) changed, the nearest 1 element"),
    (dict(stop=11), r"guard overwritten: block #0 empty float64\[2, 5\], after the body, 1 word\(s\) changed, the nearest 1 element"),
    (dict(extra=[("fid", 10 + 63)]), r"block #0 .* after the body, 1 word\(s\) changed, the nearest 64 element"),
    (dict(extra=[("lst", 6)]), r"block #1 empty int32\[2, 3\], after the body, 1 word\(s\) changed, the nearest 1 element"),
    (dict(extra=[("lst", -2)]), r"block #1 empty int32\[2, 3\], before the body, 1 word\(s\) changed, the nearest 2 element"),
    (dict(stop=9), r"unwritten: 1 of 10 element\(s\) of fid float64\[2, 5\] still hold the sentinel, the first at flat index 9"),
    (dict(first=1), r"unwritten: 1 of 10 element\(s\) of fid .* the first at flat index 0"),
    (dict(lst_stop=5), r"unwritten: 1 of 6 element\(s\) of lst int32\[2, 3\] still hold the sentinel, the first at flat index 5"),
], ids=["one_before", "one_after", "far_edge_after", "list_one_after", "list_two_before", "last_unwritten", "first_unwritten",
        "list_slot_unwritten"])
def test_broken_stand_in_fails_for_its_own_reason(shift, broken, message):
    with pytest.raises(AssertionError, match=message):
        run(shift, **dict(broken))


def test_far_edge_before_the_body():
    """the outermost guard word is still watched (at shift = 1 the front guard is one word longer)"""
    for shift in (0, 1):
        with pytest.raises(AssertionError, match=rf"before the body, 1 word\(s\) changed, the nearest {64 + shift} element"):
            run(shift, extra=[("fid", -(64 + shift))])


def test_a_write_shift_elements_early_lands_in_the_guard():
    """a kernel that rounds its base pointer down to 16 bytes writes one element early at shift = 1 - and nowhere wrong at shift = 0"""
    def aligned_down(fid, lst):
        off = -(fid.data_ptr() % 16) // 8
        kernel(fid, lst, first=off, stop=fid.numel() + off)
        if off:
            poke(fid, fid.numel() - 1, 2.5)              # (the last element written by somebody else: only the guard tells)
    for shift in (0, 1):
        arena = Arena(guard=64, shift=shift, device="cpu")
        fid, lst = arena.empty((2, 5), dtype=torch.float64, device="cpu"), arena.empty((2, 3), dtype=torch.int32, device="cpu")
        aligned_down(fid, lst)
        if shift:
            with pytest.raises(AssertionError, match=r"before the body, 1 word\(s\) changed, the nearest 1 element\(s\) from the body .*shift 1"):
                arena.check_guards()
        else:
            arena.check_guards()
            arena.assert_written(fid)


@pytest.mark.parametrize("fill", ("sentinel", "finite"))
@pytest.mark.parametrize("shift", (0, 1))
def test_place_copies_the_input_between_poisoned_guards(shift, fill):
    arena = Arena(guard=8, shift=shift, device="cpu")
    x = np.arange(12.0).reshape(3, 4)
    idx = np.arange(5, dtype=np.int32)
    tx, ti = arena.place(x, fill), arena.place(torch.from_numpy(idx), fill)
    assert tx.dtype == torch.float64 and tuple(tx.shape) == (3, 4) and tx.is_contiguous() and np.array_equal(tx.numpy(), x)
    assert ti.dtype == torch.int32 and np.array_equal(ti.numpy(), idx)
    assert tx.data_ptr() % 16 == 8 * shift and tx.storage_offset() == 8 + shift
    before = ctypes.c_uint64.from_address(tx.data_ptr() - 8).value
    after = ctypes.c_int32.from_address(ti.data_ptr() + 5 * 4).value
    if fill == "sentinel":
        assert before == SENTINEL[torch.float64] and after == SENTINEL[torch.int32]
    else:
        assert ctypes.c_double.from_address(tx.data_ptr() - 8).value == 1e300 and after == -1
    arena.check_guards()
    poke(tx, 12, 0.0)                                    # an entry that WRITES behind an input is caught as well
    with pytest.raises(AssertionError, match=rf"block #0 place\({fill}\) float64\[3, 4\], after the body"):
        arena.check_guards()
    with pytest.raises(ValueError):
        arena.place(np.zeros(3, dtype=np.float32))
    with pytest.raises(ValueError):
        arena.place(x, "zeros")


def test_size_forms_and_zero_sizes():
    arena = Arena(guard=8, shift=1, device="cpu")
    kw = dict(dtype=torch.float64, device="cpu")
    shapes = [tuple(arena.empty(*size, **kw).shape) for size in ((2, 3), ((2, 3),), ([2, 3],), (torch.Size((2, 3)),), (6,), (0,), ((0,),),
                                                                  ((3, 0),), (4, 0, 2), ((),))]
    assert shapes == [(2, 3), (2, 3), (2, 3), (2, 3), (6,), (0,), (0,), (3, 0), (4, 0, 2), ()]
    assert len(arena.blocks) == len(shapes)
    for b in arena.blocks:                               # a zero-size request still owns both guards
        assert b.raw.numel() == 8 + 1 + b.n + 8
    empty = arena.empty((3, 0), dtype=torch.int64, device="cpu")
    arena.assert_written(empty)
    arena.check_guards()
    for dtype in (torch.float64, torch.int32, torch.int64):
        t = arena.empty(3, dtype=dtype, device="cpu")
        with pytest.raises(AssertionError, match="unwritten: 3 of 3"):
            arena.assert_written(t)


def test_unsupported_calls_go_to_torch_empty(monkeypatch):
    arena = Arena(guard=8, shift=1, device="cpu")
    monkeypatch.setattr(torch, "empty", arena.empty)
    plain = [torch.empty(4), torch.empty((2, 2), dtype=torch.float32), torch.empty(3, dtype=torch.complex128),
             torch.empty(3, dtype=torch.float64, pin_memory=False), torch.empty((2, 3), dtype=torch.float64, memory_format=torch.contiguous_format),
             torch.empty(3, dtype=torch.float64, requires_grad=True), torch.empty(3, out=torch.zeros(3, dtype=torch.float64))]
    assert not arena.blocks
    assert all(t.storage_offset() == 0 for t in plain)
    assert plain[0].dtype == torch.float32 and plain[2].dtype == torch.complex128 and plain[5].requires_grad
    guarded = torch.empty((2, 3), dtype=torch.float64, device="cpu")       # the form backend.py uses
    assert len(arena.blocks) == 1 and guarded.storage_offset() == 9
    monkeypatch.undo()
    assert torch.empty(3, dtype=torch.float64).storage_offset() == 0


def test_alignment_assertion_and_arguments(monkeypatch):
    import arena as arena_mod
    real = arena_mod._REAL_EMPTY
    monkeypatch.setattr(arena_mod, "_REAL_EMPTY", lambda n, **kw: real(n + 1, **kw)[1:])     # an allocator that hands out 8 mod 16
    with pytest.raises(AssertionError, match="16-byte boundary"):
        Arena(guard=8, shift=0, device="cpu").empty(4, dtype=torch.float64, device="cpu")
    monkeypatch.undo()
    for bad in (dict(shift=2), dict(guard=7), dict(guard=0)):
        with pytest.raises(ValueError):
            Arena(**bad)
