"""CPU tests of tests/device_arena.py: the layout's congruences, the NaN bands, and that the checks of Arena.run see
what they are there to see - through device_arena.HostTransport, where the "device" is host memory and the "entry" a
Python function that writes through the pointers it is given.  This is what keeps test_gpu_caller_arrays.py from
passing by not looking."""
import ctypes

import numpy as np
import pytest

from device_arena import CANARY, GUARD, QNAN, Arena, HostTransport, check_image, image, layout, slot


def mixed_slots():
    rng = np.random.default_rng(11)
    return [slot("b", rng.uniform(-1, 1, (3, 5, 4, 7)), field=True),
            slot("one", np.array([3.5])),                               # length 1
            slot("cell", np.full(5, 7, dtype=np.int64), output=True),   # odd lengths
            slot("sign", np.full(5, 7, dtype=np.int32), output=True),
            slot("i1", np.array([9], dtype=np.int32), output=True),
            slot("g", rng.uniform(-1, 1, 3 * 9), field=True),
            slot("seeds", rng.uniform(0, 1, (3, 3))),
            slot("iters", np.full(4, 7, dtype=np.int32)),
            slot("pos", np.full((5, 3), 7.0), output=True, field=True),     # an in/out field
            slot("last", np.arange(3, dtype=np.int64))]


def test_layout_congruences_and_guards():
    slots = mixed_slots()
    placed, total = layout(slots)
    assert [p.name for p in placed] == [s.name for s in slots]
    end = 0
    for s, p in zip(slots, placed):
        assert p.end - p.start == s.array.nbytes
        assert p.start - end >= GUARD, (p.name, p.start - end)          # a guard before every array
        assert p.start - end < GUARD + 16                               # and no more padding than the congruence needs
        if s.array.dtype.itemsize == 8:
            assert p.start % 16 == 8, p
        else:
            assert p.start % 8 == 4, p
        end = p.end
    assert total - end == GUARD
    # 256-aligned bases keep the congruences
    for base in (0, 256, 4096 + 768):
        assert all((base + p.start) % 16 == 8 for s, p in zip(slots, placed) if s.array.dtype.itemsize == 8)


def test_image_contents_and_nan_bands():
    slots = mixed_slots()
    placed, total = layout(slots)
    img = image(slots, placed, total)
    covered = np.zeros(total, dtype=bool)
    nan = np.zeros(total, dtype=bool)
    for s, p in zip(slots, placed):
        assert np.array_equal(img[p.start:p.end].view(s.array.dtype).reshape(s.array.shape), s.array)
        covered[p.start:p.end] = True
        if p.field:
            for a, b in ((p.start - GUARD, p.start), (p.end, p.end + GUARD)):
                assert np.all(img[a:b].view(np.uint64) == QNAN) and np.isnan(img[a:b].view(np.float64)).all()
                nan[a:b] = True
            # what a kernel reads one element outside the field is a NaN
            assert np.isnan(img[p.start - 8:p.start].view(np.float64)[0])
            assert np.isnan(img[p.end:p.end + 8].view(np.float64)[0])
    # the bands lie exactly beside the input fields: every other guard byte is canary
    assert np.all(img[~covered & ~nan] == CANARY)
    assert nan.sum() > 0 and not np.any(nan & covered)
    for s, p in zip(slots, placed):
        if not p.field:
            left_is_field = any(q.field and q.end + GUARD > p.start - 8 for q in placed if q.end <= p.start)
            right_is_field = any(q.field and q.start - GUARD < p.end + 8 for q in placed if q.start >= p.end)
            assert left_is_field or img[p.start - 1] == CANARY
            assert right_is_field or img[p.end] == CANARY


def poke(ptr, nbytes_offset, ctype, value):
    ctype.from_address(ptr.value + nbytes_offset).value = value


def run_with(fn, written=None, plain=False):
    slots = mixed_slots()
    A = Arena(HostTransport(), slots, plain=plain)
    out = A.run(fn, written=written)
    assert not A.t.live                                                 # freed
    return A, slots, out


def test_clean_call_and_writes_into_outputs_are_accepted():
    def entry(b, one, cell, sign, i1, g, seeds, iters, pos, last):
        if b.value % 256:                                               # (plain=True: every array 256-aligned)
            assert b.value % 16 == 8 and sign.value % 8 == 4 and i1.value % 8 == 4 and pos.value % 16 == 8
        else:
            assert all(p.value % 256 == 0 for p in (one, cell, sign, i1, g, seeds, iters, pos, last))
        for k in range(5):
            poke(cell, 8 * k, ctypes.c_int64, 100 + k)
            poke(sign, 4 * k, ctypes.c_int32, -k)
        poke(i1, 0, ctypes.c_int32, 1)
        poke(pos, 8 * 14, ctypes.c_double, 2.5)
        return 42
    A, slots, out = run_with(entry)
    assert A.rc == 42 and len(out) == len(slots)
    assert np.array_equal(out[2], 100 + np.arange(5)) and np.array_equal(out[3], -np.arange(5)) and out[4][0] == 1
    assert out[8][4, 2] == 2.5 and np.all(out[8].reshape(-1)[:14] == 7.0)
    for k in (0, 1, 5, 6, 7, 9):
        assert np.array_equal(out[k], slots[k].array) and out[k].dtype == slots[k].array.dtype
    # the same through separate allocations
    B, _s, out2 = run_with(entry, plain=True)
    assert B.rc == 42 and all(np.array_equal(x, y) for x, y in zip(out, out2))


NAMES = [s.name for s in mixed_slots()]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("side", ("before", "after"))
def test_a_write_of_one_element_outside_an_array_is_seen(name, side):
    """one element just before and just after every array - doubles, int64 and int32, inputs and outputs, next to a NaN
    band and next to canary - is reported against that array with its distance"""
    slots = mixed_slots()
    k = NAMES.index(name)
    size = slots[k].array.dtype.itemsize
    ctype = {(8, "f"): ctypes.c_double, (8, "i"): ctypes.c_int64, (4, "i"): ctypes.c_int32}[
        (size, slots[k].array.dtype.kind)]

    def entry(*ptrs):
        poke(ptrs[k], -size if side == "before" else slots[k].array.nbytes, ctype, 1)
        return 0
    with pytest.raises(AssertionError) as e:
        run_with(entry)
    msg = str(e.value)
    if side == "before":
        # (a little-endian 1 changes the lowest byte, or for a double the two highest)
        assert "before the start of %s " % name in msg and ("guard changed %d bytes" % size in msg or
                                                             "guard changed 2 bytes" in msg), msg
    else:
        assert "past the end of %s " % name in msg and ("guard changed 0 bytes" in msg or
                                                         "guard changed 6 bytes" in msg), msg


def test_a_changed_input_is_seen():
    def entry(b, one, cell, sign, i1, g, seeds, iters, pos, last):
        poke(iters, 4 * 3, ctypes.c_int32, 8)
        return 0
    with pytest.raises(AssertionError, match="input iters changed at byte 12"):
        run_with(entry)
    with pytest.raises(AssertionError, match="input iters changed at byte 12"):
        run_with(entry, plain=True)

    def entry2(b, *rest):
        poke(b, 8 * 17, ctypes.c_double, 0.0)
        return 0
    with pytest.raises(AssertionError, match="input b changed at byte 1"):
        run_with(entry2)


def test_slots_past_the_records_written():
    def entry(b, one, cell, sign, i1, g, seeds, iters, pos, last):
        for k in range(3):
            poke(cell, 8 * k, ctypes.c_int64, k)
            poke(sign, 4 * k, ctypes.c_int32, k)
            for d in range(3):
                poke(pos, 8 * (3 * k + d), ctypes.c_double, 1.0)
        return 0
    three = {"cell": 3, "sign": 3, "pos": 3}
    _A, _s, out = run_with(entry, written=three)
    assert np.array_equal(out[2], [0, 1, 2, 7, 7]) and np.all(out[8][3:] == 7.0) and np.all(out[8][:3] == 1.0)
    run_with(entry, written=lambda: three)                              # counts known only after the call
    run_with(entry, written=three, plain=True)
    for plain in (False, True):
        # (7.0 -> 1.0 changes the two highest bytes of the double)
        with pytest.raises(AssertionError, match="output pos: a slot past the 2 records written changed, byte 6 past"):
            run_with(entry, written={"cell": 3, "sign": 3, "pos": 2}, plain=plain)
        with pytest.raises(AssertionError, match="output sign: a slot past the 2 records written changed, byte 0 past"):
            run_with(entry, written={"sign": 2}, plain=plain)
        with pytest.raises(AssertionError, match="output cell: a slot past the 0 records written changed"):
            run_with(entry, written={"cell": 0}, plain=plain)


def test_check_image_names_the_nearer_array():
    slots = mixed_slots()
    placed, total = layout(slots)
    before = image(slots, placed, total)
    b, one = placed[0], placed[1]
    for at, want in ((b.end + 100, "100 bytes past the end of b "), (one.start - 100, "100 bytes before the start of one "),
                     (5, "%d bytes before the start of b " % (b.start - 5)),
                     (total - 1, "%d bytes past the end of last " % (GUARD - 1))):
        after = before.copy()
        after[at] ^= 0xFF
        with pytest.raises(AssertionError, match=want):
            check_image(slots, placed, before, after)
    check_image(slots, placed, before, before.copy())
