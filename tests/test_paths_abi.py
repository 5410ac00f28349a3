"""CPU tests of the field-line path entry points (include/ndsm_hip.h, part 2): they are declared, exported, reachable
from Python with the documented defaults, and fail cleanly - an error code, never a crash, outputs cleared as the header
says, inputs untouched - without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndsm_hip.h")
ENTRIES = ["ndsm_hip_vecpot_paths", "ndsm_hip_vecpot_paths_device"]


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_paths_entries_declared_and_exported(lib):
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    import ndsm_amd
    out = subprocess.check_output(["nm", "-D", "--defined-only", ndsm_amd.lib_path()], text=True)
    live = {l.split()[-1] for l in out.splitlines() if re.search(r" T ", l)}
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in live, name
        assert hasattr(lib, name)
        # the argument list of the issue: every and an int64 max_points after direction, offsets and total before
        # the four point arrays
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
        args = [a.strip() for a in decl.split(",")]
        assert len(args) == 21 and args[8] == "int every" and args[9] == "int64_t max_points", args
        assert args[15].startswith("int64_t *") and args[16] == "int64_t *total", args
        assert len(getattr(lib, name).argtypes) == 21
    # the kernel layer behind them stays internal
    assert not any(s.startswith("ndsmk_") for s in live)
    kern = open(os.path.join(ROOT, "ndsm_amd", "csrc", "ndsm_kernels.h")).read()
    assert "ndsmk_paths_count" in kern and "ndsmk_paths_fill" in kern
    iface = open(os.path.join(ROOT, "ndsm_amd", "fsrc", "ndsmh_iface.f90")).read()
    assert 'name="ndsmk_paths_count"' in iface and 'name="ndsmk_paths_fill"' in iface
    # the header states the rules for every, offsets, max_points and OUTSIDE lines
    block = text[text.index("Field-line paths: the points of the same lines"):text.index("int ndsm_hip_vecpot_paths(")]
    flat = " ".join(block.replace("*", " ").split())
    for phrase in ("bit for bit what ndsm_hip_vecpot_trace returns",
                   "0, every, 2 every, ... steps for each multiple < n",
                   "always its final state after n steps",
                   "npts(l) = 1 if n = 0, else (n - 1) / every + 2",
                   "exclusive prefix sums of npts in lane order",
                   "offsets[nl] = total",
                   "exact and complete whatever max_points is",
                   "written if and only if k < max_points",
                   "nothing at or beyond max_points is touched",
                   "max_points = 0 is the counting call",
                   "ignored (not written) when G is NULL",
                   "after the snap",
                   "OUTSIDE lines store one point: the seed's bits as given, NaN included",
                   "Nothing is interpolated at a point that is not in the box",
                   "9004 also for every < 1 or max_points < 0"):
        assert phrase in flat, phrase


def test_paths_entries_fail_cleanly_without_a_gpu(lib):
    if lib.ndsm_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    import ndsm_amd
    # a CDLL object of its own (the same loaded library): prototypes set here stay private to this test
    lib = ctypes.CDLL(ndsm_amd.lib_path(), mode=os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, "RTLD_DEEPBIND", 0))
    vp = ctypes.c_void_p
    n, ns, cap = 3 * 8 ** 3, 5, 11
    b = np.linspace(-1.0, 1.0, n)
    g = np.linspace(2.0, 3.0, n)
    seeds = np.linspace(0.1, 0.9, 3 * ns)
    b0, g0, s0 = b.copy(), g.copy(), seeds.copy()
    for name in ENTRIES:
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = ([vp, vp, vp, ctypes.c_int, vp, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int64] + [vp] * 11)

    def outputs():
        """each array with spare slots behind what a call may clear: ends .. nsteps for 2 ns lines, offsets 2 ns + 1
        and 2 more, total and 1 more, the point arrays cap + 2 slots"""
        return [np.full(2 * 3 * ns, np.nan), np.full(2 * ns, np.nan), np.full(2 * ns, np.nan),
                np.full(2 * ns, 7, dtype=np.int32), np.full(2 * ns, 7, dtype=np.int32),
                np.full(2 * ns + 3, 7, dtype=np.int64), np.full(2, 7, dtype=np.int64),
                np.full(3 * (cap + 2), np.nan), np.full(3 * (cap + 2), np.nan), np.full(3 * (cap + 2), np.nan),
                np.full(cap + 2, np.nan)]

    def kept(a):
        return np.all((a == 7) | np.isnan(a)) if a.dtype.kind == "f" else np.all(a == 7)

    def ptrs(out):
        return [vp(a.ctypes.data) for a in out]

    for h in (None, vp(1)):          # a NULL handle, and one the library never made: neither is looked at
        for direction, nl in ((0, 2 * ns), (1, ns), (-1, ns)):
            out = outputs()
            rc = lib.ndsm_hip_vecpot_paths(h, vp(b.ctypes.data), vp(g.ctypes.data), ns, vp(seeds.ctypes.data), 0.5, 100,
                                           direction, 2, cap, *ptrs(out))
            assert rc == 9001
            # the nl lines' slots, nl + 1 offsets, total and exactly cap slots of each point array are cleared; what
            # lies behind them is not touched
            for a, m in zip(out, (3 * nl, nl, nl, nl, nl, nl + 1, 1, 3 * cap, 3 * cap, 3 * cap, cap)):
                assert np.all(a[:m] == 0), direction
                assert kept(a[m:]), direction
        # NULL optional point arrays are skipped; max_points = 0: no point array is looked at
        out = outputs()
        p = ptrs(out)
        assert lib.ndsm_hip_vecpot_paths(h, vp(b.ctypes.data), None, ns, vp(seeds.ctypes.data), 0.5, 100, 0, 1, cap,
                                         *p[:8], None, None, None) == 9001
        assert np.all(out[7][:3 * cap] == 0) and all(kept(a) for a in out[8:])
        out = outputs()
        assert lib.ndsm_hip_vecpot_paths(h, vp(b.ctypes.data), None, ns, vp(seeds.ctypes.data), 0.5, 100, 0, 1, 0,
                                         *ptrs(out)) == 9001
        assert out[6][0] == 0 and np.all(out[5][:2 * ns + 1] == 0) and all(kept(a) for a in out[7:])
        # bad scalars and NULL arrays: still 9001, and no crash
        for ns_, step, mx, direction, every, mp in ((ns, 0.0, 100, 0, 1, cap), (ns, 0.5, 0, 0, 1, cap),
                                                    (ns, 0.5, 100, 3, 1, cap), (-1, 0.5, 100, 0, 1, cap),
                                                    (0, 0.5, 100, 0, 1, cap), (ns, 0.5, 100, 0, 0, cap),
                                                    (ns, 0.5, 100, 0, -2, cap), (ns, 0.5, 100, 0, 1, -1),
                                                    (ns, 0.5, 100, 0, 1, -2 ** 62)):
            out = outputs()
            rc = lib.ndsm_hip_vecpot_paths(h, vp(b.ctypes.data), None, ns_, vp(seeds.ctypes.data), step, mx, direction,
                                           every, mp, *ptrs(out))
            assert rc == 9001, (ns_, step, mx, direction, every, mp)
            assert out[6][0] == 0 and out[6][1] == 7
            if mp < 0:
                assert all(kept(a) for a in out[7:])          # no capacity: no slot of a point array is cleared
        assert lib.ndsm_hip_vecpot_paths(h, None, None, ns, None, 0.5, 100, 0, 1, cap, *[None] * 11) == 9001
        # the device entry never reads or writes through its array arguments on the host; total is a host scalar
        out = outputs()
        rc = lib.ndsm_hip_vecpot_paths_device(h, vp(b.ctypes.data), vp(g.ctypes.data), ns, vp(seeds.ctypes.data), 0.5,
                                              100, 0, 1, cap, *ptrs(out))
        assert rc == 9001
        assert out[6][0] == 0 and out[6][1] == 7
        assert all(kept(a) for k, a in enumerate(out) if k != 6)
        assert lib.ndsm_hip_vecpot_paths_device(h, None, None, ns, None, 0.5, 100, 0, 1, cap, *[None] * 11) == 9001
    assert np.array_equal(b, b0) and np.array_equal(g, g0) and np.array_equal(seeds, s0)
    # the Python layer raises instead
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    sd = np.full((4, 3), 0.5)
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.trace_paths(x, x, x, z, sd)


def test_paths_python_names(lib):
    import ndsm_amd
    for name in ("FieldPaths", "trace_paths", "path_of", "whole_line"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    assert ndsm_amd.FieldPaths._fields == ("lines", "offsets", "points", "b", "g", "integral")
    par = inspect.signature(ndsm_amd.VecPot.paths).parameters
    assert list(par)[1:] == ["b", "seeds", "g", "step", "max_steps", "direction", "every", "max_points", "values",
                             "device"]
    assert ([par[k].default for k in list(par)[3:]] == [None, 0.5, None, "both", 1, None, True, False])
    par = inspect.signature(ndsm_amd.trace_paths).parameters
    assert list(par)[:5] == ["x", "y", "z", "b", "seeds"]
    assert ([par[k].default for k in ("g", "step", "max_steps", "direction", "every", "max_points", "values")] ==
            [None, 0.5, None, "both", 1, None, True])
    # the trace signatures keep their defaults
    par = inspect.signature(ndsm_amd.VecPot.trace).parameters
    assert list(par)[1:] == ["b", "seeds", "g", "step", "max_steps", "direction", "device"]
    assert ndsm_amd.FieldLines._fields == ("ends", "length", "integral", "status", "nsteps", "flh")


def test_paths_arguments_checked_before_any_device_call(lib):
    """bad options are a ValueError and arrays that do not fit an argument error (9002), before the library is
    called"""
    import ndsm_amd
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    sd = np.full((4, 3), 0.5)
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.trace_paths(x, x, x[:7], z, sd)
    with pytest.raises(ValueError):
        ndsm_amd.trace_paths(x, x, x, z, sd, every=0)
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.nshape4 = np.array([8, 8, 8, 3], dtype=np.intc)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library reached: " + name)
    V.L, V.h = NoCalls(), None
    for kw in (dict(step=0.0), dict(step=float("nan")), dict(max_steps=0), dict(max_steps=2.5), dict(direction="up"),
               dict(direction=0), dict(every=0), dict(every=-1), dict(every=1.5), dict(every=None), dict(every=True),
               dict(every="2"), dict(every=float("nan")), dict(every=2 ** 31), dict(max_points=-1),
               dict(max_points=2.5), dict(max_points=True), dict(max_points="7"), dict(max_points=float("inf")),
               dict(max_points=2 ** 41)):
        with pytest.raises(ValueError):
            V.paths(z, sd, **kw)
    for bad in (np.zeros((3, 8, 8, 7)), np.zeros((8, 8, 8, 3))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.paths(bad, sd)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.paths(z, sd, g=bad)
    for bad in (np.zeros(3), np.zeros((4, 2))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.paths(z, bad)
    # no seeds: an empty result, and still no call
    fp = V.paths(z, np.zeros((0, 3)), g=z)
    assert fp.lines.ends.shape == (2, 0, 3) and fp.offsets.tolist() == [0] and fp.offsets.dtype == np.int64
    assert fp.points.shape == fp.b.shape == fp.g.shape == (0, 3) and fp.integral.shape == (0,)
    fp = V.paths(z, np.zeros((0, 3)), direction="forward")
    assert fp.lines.flh is None and fp.b.shape == (0, 3) and fp.g is None and fp.integral is None
    assert V.paths(z, np.zeros((0, 3)), values=False).b is None


def test_path_of_and_whole_line_on_a_hand_made_result():
    import ndsm_amd
    from ndsm_amd import _lib
    # one seed, both directions: forward 0 -> 1 -> 2.5 (two steps), backward 0 -> -1 (one step)
    out = [np.array([[[2.5, 0, 0]], [[-1.0, 0, 0]]]), np.array([[2.5], [1.0]]), np.array([[5.0], [3.0]]),
           np.array([[2], [1]], dtype=np.int32), np.array([[2], [1]], dtype=np.int32)]
    pts = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.5, 0, 0], [0.0, 0, 0], [-1.0, 0, 0]])
    ipt = np.array([0.0, 2.0, 5.0, 0.0, 3.0])
    fp = _lib._field_paths(out, 0, np.array([0, 3, 5], dtype=np.int64), pts, 10 * pts, None, ipt)
    assert ndsm_amd.path_of(fp, 1)[0].tolist() == [[0.0, 0, 0], [-1.0, 0, 0]] and ndsm_amd.path_of(fp, 1)[2] is None
    p, b, g, i = ndsm_amd.whole_line(fp, 0)
    assert p[:, 0].tolist() == [-1.0, 0.0, 1.0, 2.5] and b[:, 0].tolist() == [-10.0, 0.0, 10.0, 25.0] and g is None
    assert i.tolist() == [0.0, 3.0, 5.0, 8.0] and i[-1] == fp.lines.flh[0]
    for bad in (2, -1, 0.5):
        with pytest.raises(IndexError):
            ndsm_amd.path_of(fp, bad)
    with pytest.raises(IndexError):
        ndsm_amd.whole_line(fp, 1)
    one = _lib._field_paths([a[:1] for a in out], 1, np.array([0, 3], dtype=np.int64), pts[:3], None, None, None)
    with pytest.raises(ValueError):
        ndsm_amd.whole_line(one, 0)
