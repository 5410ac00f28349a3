"""CPU tests of the separator entry points (include/ndsm_hip.h, part 2): they are declared with the documented argument
list, exported, reachable from Python with the documented defaults, and fail cleanly - an error code, never a crash,
outputs cleared as the header says, inputs untouched - without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndsm_hip.h")
ENTRIES = ["ndsm_hip_vecpot_separators", "ndsm_hip_vecpot_separators_device"]
ARGS = ["void *h", "const double *B", "int nnulls", "const double *pos", "const int32_t *kind", "const double *normal",
        "int nbr", "const int32_t *pair", "const double *arc", "double radius", "double capture", "double step",
        "int max_steps", "int rounds", "double tol", "int every", "int64_t max_points", "int32_t *state",
        "int32_t *nrounds", "double *coef", "double *width", "int32_t *side", "double *dmin", "double *ends",
        "double *length", "int32_t *status", "int32_t *nsteps", "int64_t *offsets", "int64_t *total", "double *points",
        "double *bpt"]


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_separator_entries_declared_and_exported(lib):
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    import ndsm_amd
    out = subprocess.check_output(["nm", "-D", "--defined-only", ndsm_amd.lib_path()], text=True)
    live = {l.split()[-1] for l in out.splitlines() if re.search(r" T ", l)}
    for name in ENTRIES:
        assert name in live, name
        assert hasattr(lib, name)
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
        args = [" ".join(a.split()) for a in decl.split(",")]
        assert len(args) == 31, args
        if name.endswith("_device"):
            # the same list on device arrays: the names of the arrays carry a d
            args = [re.sub(r"\*d(?=[a-zB])", "*", a) for a in args]
        assert args == ARGS, args
        assert len(getattr(lib, name).argtypes) == 31
    # the kernel layer behind them stays internal
    assert not any(s.startswith("ndsmk_") for s in live)
    kern = open(os.path.join(ROOT, "ndsm_amd", "csrc", "ndsm_kernels.h")).read()
    assert "ndsmk_sep_count" in kern and "ndsmk_sep_fill" in kern
    iface = open(os.path.join(ROOT, "ndsm_amd", "fsrc", "ndsmh_iface.f90")).read()
    assert 'name="ndsmk_sep_count"' in iface and 'name="ndsmk_sep_fill"' in iface
    for k, name in enumerate(("NONE", "FOUND", "FAR", "NO_CROSSING", "GAP", "UNRESOLVED")):
        assert re.search(r"#define NDSM_HIP_SEP_%s +%d\b" % (name, k), text), name
    # the header states the rules
    block = text[text.index("Separator lines: fan brackets between null pairs"):text.index("#define NDSM_HIP_SEP_NONE")]
    flat = " ".join(block.replace("*", " ").split())
    for phrase in ("one wave of 64 lanes",
                   "sg = +1 for kind(m) > 0, -1 for kind(m) < 0",
                   "m != m' and kind(m), kind(m') have strictly opposite signs",
                   "t = i / 63, c = (1 - t) c_a + t c_b, s = (1 - t) s_a + t s_b, n = sqrt(c c + s s)",
                   "Lanes 0 and 63 take a and b unchanged",
                   "pos(m)_d + rho (c e1_d + s e2_d)",
                   "the capture test against m' ALONE",
                   "after every accepted FULL step, not at the seed, not after the exit step",
                   "d2 = (dx dx + dy dy) + dz dz",
                   "g = (w'_0 dx + w'_1 dy) + w'_2 dz",
                   "+1 for g >= 0, -1 for g < 0, 0 when the line has no such point",
                   "i is the lowest lane >= 1 whose class differs from lane 0's",
                   "a <- d_(i - 1), b <- d_(i )",
                   "width = sqrt((c_a - c_b) (c_a - c_b) + (s_a - s_b) (s_a - s_b))",
                   "were both CAPTURED by m'",
                   "one point with pos(m)'s bits, status NDSM_HIP_SKEL_NONE",
                   "bit for bit, fan line 0 (lane 2) of null 0 of ndsm_hip_vecpot_skeleton",
                   "all pairs are checked before anything is written",
                   "nbr == 0 succeeds, sets total = 0 and touches nothing else"):
        assert phrase in flat, phrase


def test_separator_entries_fail_cleanly_without_a_gpu(lib):
    if lib.ndsm_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    import ndsm_amd
    # a CDLL object of its own (the same loaded library): prototypes set here stay private to this test
    lib = ctypes.CDLL(ndsm_amd.lib_path(), mode=os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, "RTLD_DEEPBIND", 0))
    vp = ctypes.c_void_p
    n, nn, nbr, cap = 3 * 8 ** 3, 3, 5, 11
    b = np.linspace(-1.0, 1.0, n)
    pos = np.linspace(0.2, 0.8, 3 * nn)
    kind = np.array([1, -1, 2], dtype=np.int32)
    normal = np.linspace(-1.0, 2.0, 3 * nn)
    pair = np.array([0, 1, 1, 0, 2, 1, 1, 2, 0, 0], dtype=np.int32)
    arc = np.linspace(-1.0, 1.0, 4 * nbr)
    ins = [b, pos, kind, normal, pair, arc]
    before = [a.copy() for a in ins]
    for name in ENTRIES:
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = ([vp, vp, ctypes.c_int, vp, vp, vp, ctypes.c_int, vp, vp] + [ctypes.c_double] * 3 +
                                       [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int64] +
                                       [vp] * 14)
    i32 = np.int32

    def outputs():
        """each array with spare slots behind what a call may clear: state, nrounds, coef, width, side, dmin, ends,
        length, status, nsteps, offsets, total, points, bpt"""
        return [np.full(nbr + 2, 7, dtype=i32), np.full(nbr + 2, 7, dtype=i32), np.full(4 * nbr + 2, np.nan),
                np.full(nbr + 2, np.nan), np.full(nbr + 2, 7, dtype=i32), np.full(2 * nbr + 2, np.nan),
                np.full(3 * nbr + 2, np.nan), np.full(nbr + 2, np.nan), np.full(nbr + 2, 7, dtype=i32),
                np.full(nbr + 2, 7, dtype=i32), np.full(nbr + 3, 7, dtype=np.int64), np.full(2, 7, dtype=np.int64),
                np.full(3 * (cap + 2), np.nan), np.full(3 * (cap + 2), np.nan)]
    cleared = (nbr, nbr, 4 * nbr, nbr, nbr, 2 * nbr, 3 * nbr, nbr, nbr, nbr, nbr + 1, 1, 3 * cap, 3 * cap)
    TOTAL, POINTS, BPT = 11, 12, 13

    def kept(a):
        return np.all((a == 7) | np.isnan(a)) if a.dtype.kind == "f" else np.all(a == 7)

    def ptrs(out):
        return [vp(a.ctypes.data) for a in out]

    def call(entry, h, nnulls=nn, nb=nbr, radius=0.5, capture=0.5, step=0.5, max_steps=100, rounds=10, tol=1e-12,
             every=1, mp=cap, out=None, arrays=True):
        p = ptrs(out) if out is not None else [None] * 14
        i = [vp(a.ctypes.data) for a in ins] if arrays else [None] * 6
        return entry(h, i[0], nnulls, i[1], i[2], i[3], nb, i[4], i[5], radius, capture, step, max_steps, rounds, tol,
                     every, mp, *p)

    for h in (None, vp(1)):          # a NULL handle, and one the library never made: neither is looked at
        out = outputs()
        assert call(lib.ndsm_hip_vecpot_separators, h, out=out) == 9001
        # exactly the nbr, nbr + 1 and cap slots are cleared; what lies behind them is not touched
        for a, m in zip(out, cleared):
            assert np.all(a[:m] == 0) and kept(a[m:])
        # a NULL bpt is skipped; max_points = 0: no point array is looked at
        out = outputs()
        p = ptrs(out)
        p[BPT] = None
        i = [vp(a.ctypes.data) for a in ins]
        assert lib.ndsm_hip_vecpot_separators(h, i[0], nn, i[1], i[2], i[3], nbr, i[4], i[5], 0.5, 0.5, 0.5, 100, 10,
                                              1e-12, 1, cap, *p) == 9001
        assert np.all(out[POINTS][:3 * cap] == 0) and kept(out[BPT])
        out = outputs()
        assert call(lib.ndsm_hip_vecpot_separators, h, mp=0, out=out) == 9001
        assert out[TOTAL][0] == 0 and np.all(out[10][:nbr + 1] == 0) and kept(out[POINTS]) and kept(out[BPT])
        # bad scalars and NULL arrays: still 9001 whatever the arguments, total cleared, and no crash
        for kw in (dict(nnulls=-1), dict(nnulls=0), dict(nb=-1), dict(nb=0), dict(radius=0.0), dict(radius=float("nan")),
                   dict(radius=float("inf")), dict(capture=0.0), dict(capture=-1.0), dict(capture=float("nan")),
                   dict(step=0.0), dict(max_steps=0), dict(rounds=0), dict(tol=-1.0), dict(tol=float("nan")),
                   dict(tol=float("inf")), dict(every=0), dict(mp=-1), dict(mp=-2 ** 62), dict(nb=2 ** 31 - 1)):
            out = outputs()
            small = kw.get("nb", nbr) <= nbr
            assert call(lib.ndsm_hip_vecpot_separators, h, out=out if small else None, **kw) == 9001, kw
            if small:
                assert out[TOTAL][0] == 0 and out[TOTAL][1] == 7, kw
                if kw.get("mp", cap) < 0:
                    assert kept(out[POINTS]) and kept(out[BPT])   # no capacity: no slot of a point array is cleared
                if kw.get("nb", nbr) <= 0:
                    assert all(kept(a) for a in out[:11])         # no brackets: no slot of a bracket array is cleared
        assert call(lib.ndsm_hip_vecpot_separators, h, arrays=False) == 9001
        # the device entry never reads or writes through its array arguments on the host; total is a host scalar
        out = outputs()
        assert call(lib.ndsm_hip_vecpot_separators_device, h, out=out) == 9001
        assert out[TOTAL][0] == 0 and out[TOTAL][1] == 7
        assert all(kept(a) for k, a in enumerate(out) if k != TOTAL)
        assert call(lib.ndsm_hip_vecpot_separators_device, h, arrays=False) == 9001
    assert all(np.array_equal(a, c) for a, c in zip(ins, before))
    # the Python layer raises instead
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    sk = ndsm_amd.Skeleton(np.full((2, 3), 0.5), np.array([1, -1], dtype=np.int32), None, None,
                           np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]), None, np.zeros((2, 10), dtype=np.int32))
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.find_separators(x, x, x, z, skeleton=sk)


def test_separator_python_names(lib):
    import ndsm_amd
    for name in ("Separators", "find_separators", "separator_of"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    assert ndsm_amd.Separators._fields == ("pair", "state", "coef", "width", "side", "dmin", "paths")
    par = inspect.signature(ndsm_amd.VecPot.separators).parameters
    assert list(par)[1:] == ["b", "skeleton", "pairs", "brackets", "radius", "capture", "step", "max_steps", "rounds",
                             "tol", "every", "ring", "values", "device"]
    assert [par[k].default for k in list(par)[2:]] == [None, None, None, 0.5, None, 0.5, None, 10, 1e-12, 1, None, True,
                                                       False]
    par = inspect.signature(ndsm_amd.find_separators).parameters
    assert list(par)[:4] == ["x", "y", "z", "b"]
    assert [par[k].default for k in ("skeleton", "pairs", "brackets", "rounds", "tol", "every")] == [None, None, None, 10,
                                                                                                     1e-12, 1]
    from ndsm_amd import _lib
    assert (_lib.SEP_NONE, _lib.SEP_FOUND, _lib.SEP_FAR, _lib.SEP_NO_CROSSING, _lib.SEP_GAP,
            _lib.SEP_UNRESOLVED) == (0, 1, 2, 3, 4, 5)
    # capture=None means radius
    assert _lib._separator_args(0.7, None, 10, 1e-12) == (0.7, 0.7, 10, 1e-12)
    # the default brackets: every ordered pair of opposite signs, the nring cyclically adjacent arcs of the ring
    ring = _lib._skeleton_ring(4, None)
    pair, arc = _lib._separator_brackets(np.array([1, -2, 0, 2]), ring)
    assert pair.dtype == np.int32 and pair[::4].tolist() == [[0, 1], [1, 0], [1, 3], [3, 1]]
    assert arc.shape == (16, 4) and np.array_equal(arc[:4, :2], ring) and np.array_equal(arc[:4, 2:], ring[[1, 2, 3, 0]])
    assert np.array_equal(arc[4:8], arc[:4])
    pair, arc = _lib._separator_brackets(np.array([1, -2, 0, 2]), ring, [(3, 1)])
    assert pair.tolist() == [[3, 1]] * 4
    # more than 65536 default brackets ask for pairs
    with pytest.raises(ValueError, match="pairs"):
        _lib._separator_brackets(np.array([1, -1] * 40), _lib._skeleton_ring(32, None))
    assert len(_lib._separator_brackets(np.array([1, -1] * 40), _lib._skeleton_ring(32, None), [(0, 1)])[0]) == 32


def test_separator_arguments_checked_before_any_device_call(lib):
    """bad options are a ValueError and arrays that do not fit an argument error (9002), before the library is
    called"""
    import ndsm_amd
    z = np.zeros((3, 8, 8, 8))
    sk = ndsm_amd.Skeleton(np.full((2, 3), 0.5), np.array([1, -1], dtype=np.int32), None, None,
                           np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]), None, np.zeros((2, 10), dtype=np.int32))
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.nshape4 = np.array([8, 8, 8, 3], dtype=np.intc)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library reached: " + name)
    V.L, V.h = NoCalls(), None
    good = (np.array([[0, 1]]), np.array([[1.0, 0.0, 0.0, 1.0]]))
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
               dict(radius=None), dict(radius="1"), dict(radius=True), dict(capture=0), dict(capture=-0.1),
               dict(capture=float("nan")), dict(capture=float("inf")), dict(capture="1"), dict(rounds=0),
               dict(rounds=2.5), dict(rounds=None), dict(rounds=True), dict(tol=-1e-3), dict(tol=float("nan")),
               dict(tol=float("inf")), dict(tol=None), dict(step=0.0), dict(step=float("nan")), dict(max_steps=0),
               dict(max_steps=2.5), dict(every=0), dict(every=1.5), dict(every=None), dict(ring=np.zeros(4)),
               dict(pairs=[0, 1]), dict(pairs=[(0.5, 1.0)]), dict(pairs=[(0, 2)]), dict(pairs=[(-1, 0)]),
               dict(brackets=(good[0], np.zeros((1, 3)))), dict(brackets=(np.array([0, 1]), good[1])),
               dict(brackets=(np.array([[0, 2]]), good[1])), dict(brackets=(np.array([[0.0, 1.0]]), good[1])),
               dict(brackets=good, pairs=[(0, 1)])):
        with pytest.raises(ValueError):
            V.separators(z, skeleton=sk, **kw)
    for bad in (np.zeros((3, 8, 8, 7)), np.zeros((8, 8, 8, 3))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.separators(bad, skeleton=sk)
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        V.separators(z, skeleton=sk._replace(kind=np.array([1, -1, 1], dtype=np.int32)))
    # no brackets: an empty result, and still no call
    for kw in (dict(skeleton=sk._replace(kind=np.array([1, 1], dtype=np.int32))), dict(skeleton=sk, pairs=np.zeros((0, 2), int)),
               dict(skeleton=sk, brackets=(np.zeros((0, 2), dtype=int), np.zeros((0, 4))))):
        sp = V.separators(z, **kw)
        assert isinstance(sp, ndsm_amd.Separators)
        assert sp.pair.shape == (0, 2) and sp.state.shape == (0,) and sp.coef.shape == (0, 4) and sp.dmin.shape == (0, 2)
        assert sp.paths.lines.ends.shape == (0, 3) and sp.paths.offsets.tolist() == [0]
        assert sp.paths.points.shape == sp.paths.b.shape == (0, 3) and ndsm_amd.separator_of(sp, 0, 1) == []
    assert V.separators(z, skeleton=sk, pairs=np.zeros((0, 2), int), values=False).paths.b is None


def test_separator_of_on_a_hand_made_result():
    import ndsm_amd
    from ndsm_amd import _lib
    pair = np.array([[0, 1], [0, 1], [1, 0], [0, 1]], dtype=np.int32)
    state = np.array([1, 3, 1, 1], dtype=np.int32)
    z = np.zeros
    per = [state, z(4, dtype=np.int32), z((4, 4)), z(4), z(4, dtype=np.int32), z((4, 2)), z((4, 3)), z(4),
           z(4, dtype=np.int32), z(4, dtype=np.int32)]
    offsets = np.array([0, 3, 4, 6, 10], dtype=np.int64)
    sp = _lib._separators_tuple(pair, per, offsets, np.arange(30.0).reshape(10, 3), None)
    got = ndsm_amd.separator_of(sp, 0, 1)
    assert [len(p) for p, _b in got] == [3, 4] and got[0][1] is None and got[1][0][0, 0] == 18.0
    assert [len(p) for p, _b in ndsm_amd.separator_of(sp, 1, 0)] == [2] and ndsm_amd.separator_of(sp, 1, 1) == []
    with pytest.raises(IndexError):
        ndsm_amd.separator_of(sp, -1, 0)
