"""Caller arrays the way a caller has them: views into one larger device allocation, aligned as far as their element
type asks and no further, with other data on both sides (INTEGRATION.md "Device-resident fields").  Used by
test_gpu_caller_arrays.py on the *_device entries; the layout and the checks are plain numpy over a host image of the
allocation and are tested without a GPU (test_device_arena.py) through a transport that keeps the image in host memory.

    arena = Arena(LibTransport(L), [slot("B", b, field=True), slot("cell", np.full(m, 7, np.int64), output=True), ...])
    B, cell, ... = arena.run(lambda dB, dcell, ...: L.entry(h, dB, ..., dcell, ...), written={"cell": nf})

One allocation holds every array of the call, in the order given.  Each array lies between guard bands of at least
GUARD bytes; arrays of 8-byte elements start at an address = 8 (mod 16), arrays of 4-byte elements at = 4 (mod 8) (the
allocation itself starts where the allocator puts it: 256-aligned).  The GUARD bytes on either side of an input field
(`field=True`; in/out fields too) hold quiet NaN doubles, so that a read outside the field reaches the result even where its weight is 0;
every other guard byte holds CANARY.  After the call the whole image is read back and compared with what went up:
every byte outside the arrays declared `output=True` must be unchanged - guards and inputs alike - and so must every
slot of an output past its `written` records.  plain=True puts the same arrays into allocations of their own (each
256-aligned, nothing beside it): the layout of the rest of the suite, as the comparison partner."""
import collections
import ctypes

import numpy as np

GUARD = 4096
CANARY = 0xA5
QNAN = np.array([np.nan]).view(np.uint64)[0]            # 0x7ff8000000000000

Slot = collections.namedtuple("Slot", ["name", "array", "output", "field"])
Placed = collections.namedtuple("Placed", ["name", "start", "end", "output", "field"])


def slot(name, array, output=False, field=False):
    """one array of a call: output - the entry may write it (an in/out array is an output); field - a field the entry
    reads (an in/out field is both), NaN bands beside it"""
    a = np.ascontiguousarray(array)
    assert a.dtype.itemsize in (4, 8) and a.size > 0, (name, a.dtype, a.shape)
    assert not field or a.dtype == np.float64, (name, a.dtype)
    return Slot(name, a, bool(output), bool(field))


def layout(slots):
    """(placed, total): the byte extent [start, end) of every slot in an allocation whose base is 16-aligned, and the
    size of that allocation"""
    placed, pos = [], 0
    for s in slots:
        size = s.array.dtype.itemsize
        start = pos + GUARD
        want = 8 if size == 8 else 4                    # = 8 (mod 16), or = 4 (mod 8)
        start += (want - start) % (2 * size)
        placed.append(Placed(s.name, start, start + s.array.nbytes, s.output, s.field))
        pos = start + s.array.nbytes
    return placed, pos + GUARD


def image(slots, placed, total):
    """the host image of the allocation: canary, NaN bands beside the input fields, the arrays' contents"""
    img = np.full(total, CANARY, dtype=np.uint8)
    for p in placed:
        if p.field:                                     # (p.start is 8-aligned: whole doubles)
            img[p.start - GUARD:p.start].view(np.uint64)[:] = QNAN
            img[p.end:p.end + GUARD].view(np.uint64)[:] = QNAN
    for s, p in zip(slots, placed):                     # (after the bands: a band never reaches into an array, the
        img[p.start:p.end] = s.array.reshape(-1).view(np.uint8)   # guards being at least as wide)
    return img


def written_bytes(s, count):
    """the bytes of the first `count` records (along the first axis) of a slot's array"""
    n = len(s.array)
    assert 0 <= count <= n, (s.name, count, n)
    return (s.array.nbytes // n) * int(count)


def check_image(slots, placed, before, after, written=None):
    """AssertionError unless `after` equals `before` in every byte outside the outputs and in every slot of an output
    past its written records; the message names the array and the distance from it"""
    written = written or {}
    free = np.zeros(len(before), dtype=bool)            # the bytes the call may change
    for s, p in zip(slots, placed):
        if p.output:
            free[p.start:(p.start + written_bytes(s, written[s.name])) if s.name in written else p.end] = True
    bad = np.nonzero((before != after) & ~free)[0]
    if len(bad) == 0:
        return
    at = int(bad[0])
    for i, (s, p) in enumerate(zip(slots, placed)):
        if p.start <= at < p.end:
            if p.output:
                raise AssertionError("output %s: a slot past the %d records written changed, byte %d past their end "
                                     "(%d bytes differ in all)" % (p.name, written[s.name], at - p.start -
                                                                   written_bytes(s, written[s.name]), len(bad)))
            raise AssertionError("input %s changed at byte %d (%d bytes differ in all)" % (p.name, at - p.start, len(bad)))
        if at < p.start:                                # in the guard before p: the nearer array is named
            prev = placed[i - 1] if i > 0 else None
            if prev is not None and at - prev.end < p.start - at:
                break
            raise AssertionError("guard changed %d bytes before the start of %s (%d bytes differ in all)"
                                 % (p.start - at, p.name, len(bad)))
    else:
        prev = placed[-1]
    raise AssertionError("guard changed %d bytes past the end of %s (%d bytes differ in all)"
                         % (at - prev.end, prev.name, len(bad)))


class LibTransport:
    """device memory through the library's own helpers (ndsm_hip_device_alloc and the blocking copies)"""

    def __init__(self, L):
        self.L = L

    def _ok(self, rc, what):
        from ndsm_amd import _lib
        assert rc == 0, (what, rc, _lib.last_error(self.L))

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        self._ok(self.L.ndsm_hip_device_alloc(nbytes, ctypes.byref(p)), "device_alloc")
        return p.value

    def free(self, base):
        self.L.ndsm_hip_device_free(ctypes.c_void_p(base))

    def h2d(self, dst, host):
        self._ok(self.L.ndsm_hip_memcpy_h2d(ctypes.c_void_p(dst), host.ctypes.data, host.nbytes), "h2d")

    def d2h(self, host, src):
        self._ok(self.L.ndsm_hip_memcpy_d2h(host.ctypes.data, ctypes.c_void_p(src), host.nbytes), "d2h")


class HostTransport:
    """the same interface over host memory: the "device pointers" are addresses in buffers of this process, and the call
    is a Python function that writes through them (test_device_arena.py)"""

    def __init__(self):
        self.live = {}

    def alloc(self, nbytes):
        buf = np.zeros(nbytes + 256, dtype=np.uint8)
        base = buf.ctypes.data + (-buf.ctypes.data) % 256
        self.live[base] = buf
        return base

    def free(self, base):
        del self.live[base]

    def h2d(self, dst, host):
        ctypes.memmove(dst, host.ctypes.data, host.nbytes)

    def d2h(self, host, src):
        ctypes.memmove(host.ctypes.data, src, host.nbytes)


class Arena:
    def __init__(self, transport, slots, plain=False):
        self.t, self.slots, self.plain = transport, list(slots), plain
        names = [s.name for s in self.slots]
        assert len(set(names)) == len(names), names
        self.placed, self.total = layout(self.slots)
        self.rc = None

    def run(self, call, written=None):
        """upload, call(*device pointers), download, free; the arrays as they came back, in the order of the slots.
        The call's return value is kept in self.rc.  written: {name: records written} for outputs whose later slots must
        stay as they were, or a function that returns it once the call has run.  AssertionError: see check_image."""
        if self.plain:
            return self._run_plain(call, written)
        before = image(self.slots, self.placed, self.total)
        after = np.empty_like(before)
        base = self.t.alloc(self.total)
        try:
            assert base % 16 == 0, base
            self.t.h2d(base, before)
            self.rc = call(*[ctypes.c_void_p(base + p.start) for p in self.placed])
            self.t.d2h(after, base)
        finally:
            self.t.free(base)
        check_image(self.slots, self.placed, before, after, written() if callable(written) else written)
        return [after[p.start:p.end].view(s.array.dtype).reshape(s.array.shape).copy()
                for s, p in zip(self.slots, self.placed)]

    def _run_plain(self, call, written):
        bases, out = [], []
        try:
            for s in self.slots:
                bases.append(self.t.alloc(s.array.nbytes))
                self.t.h2d(bases[-1], s.array)
            self.rc = call(*[ctypes.c_void_p(b) for b in bases])
            for s, b in zip(self.slots, bases):
                out.append(np.empty_like(s.array))
                self.t.d2h(out[-1], b)
        finally:
            for b in bases:
                self.t.free(b)
        written = (written() if callable(written) else written) or {}
        for s, a in zip(self.slots, out):
            same = a.reshape(-1).view(np.uint8) == s.array.reshape(-1).view(np.uint8)
            if not s.output:
                assert same.all(), "input %s changed at byte %d" % (s.name, int(np.nonzero(~same)[0][0]))
            elif s.name in written:
                nb = written_bytes(s, written[s.name])
                assert same[nb:].all(), ("output %s: a slot past the %d records written changed, byte %d past their end"
                                         % (s.name, written[s.name], int(np.nonzero(~same[nb:])[0][0])))
        return out
