"""CPU tests of the skeleton entry points (include/ndsm_hip.h, part 2): they are declared with the documented argument
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
ENTRIES = ["ndsm_hip_vecpot_skeleton", "ndsm_hip_vecpot_skeleton_device"]
ARGS = ["void *h", "const double *B", "int nnulls", "const double *pos", "const double *jac", "int nring",
        "const double *ring", "double radius", "double capture", "double step", "int max_steps", "int every",
        "int64_t max_points", "int32_t *kind", "double *eig", "double *spine", "double *normal", "double *ends",
        "double *length", "int32_t *status", "int32_t *nsteps", "int32_t *hit", "int64_t *offsets", "int64_t *total",
        "double *points", "double *bpt"]


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_skeleton_entries_declared_and_exported(lib):
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
        assert len(args) == 26, args
        if name.endswith("_device"):
            # the same list on device arrays: the names of the arrays carry a d
            args = [re.sub(r"\*d(?=[a-zB])", "*", a) for a in args]
        assert args == ARGS, args
        assert len(getattr(lib, name).argtypes) == 26
    # the kernel layer behind them stays internal
    assert not any(s.startswith("ndsmk_") for s in live)
    kern = open(os.path.join(ROOT, "ndsm_amd", "csrc", "ndsm_kernels.h")).read()
    assert "ndsmk_skel_count" in kern and "ndsmk_skel_fill" in kern
    iface = open(os.path.join(ROOT, "ndsm_amd", "fsrc", "ndsmh_iface.f90")).read()
    assert 'name="ndsmk_skel_count"' in iface and 'name="ndsmk_skel_fill"' in iface
    assert "#define NDSM_HIP_SKEL_CAPTURED 10" in text and "#define NDSM_HIP_SKEL_NONE 11" in text
    # the header states the rules
    block = text[text.index("Spine-fan skeleton of the nulls and null-to-null connections"):
                 text.index("#define NDSM_HIP_SKEL_CAPTURED")]
    flat = " ".join(block.replace("*", " ").split())
    for phrase in ("s = +1 for det M > 0, -1 for det M < 0",
                   "a = (N00 + N11) + N22",
                   "p = ((mu - a) mu + b) mu - c, p' = (3 mu - 2 a) mu + b",
                   "AT MOST 40 ITERATIONS",
                   "t = a - mu",
                   "the lowest index on a tie",
                   "e2 = w x e1",
                   "kind = -s",
                   "eig = (s mu, s t, c / mu)",
                   "q = 0: pos_d + rho v_d; q = 1: pos_d - rho v_d; q = 2 + j: pos_d + rho (c_j e1_d + s_j e2_d)",
                   "the spine lanes trace with sgn = s, the fan lanes with sgn = -s",
                   "after every accepted FULL step - not at the seed, not after the exit step",
                   "m' = m skipped",
                   "((dx dx + dy dy) + dz dz) <= (capture min(h))^2",
                   "hit[l] = -1",
                   "status NDSM_HIP_SKEL_NONE",
                   "bit for bit those of ndsm_hip_vecpot_paths",
                   "a captured line is bit for bit the first nsteps[l] steps of that line",
                   "nnulls == 0 succeeds, sets total = 0 and touches nothing else"):
        assert phrase in flat, phrase


def test_skeleton_entries_fail_cleanly_without_a_gpu(lib):
    if lib.ndsm_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    import ndsm_amd
    # a CDLL object of its own (the same loaded library): prototypes set here stay private to this test
    lib = ctypes.CDLL(ndsm_amd.lib_path(), mode=os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, "RTLD_DEEPBIND", 0))
    vp = ctypes.c_void_p
    n, nn, nr, cap = 3 * 8 ** 3, 3, 4, 11
    L = 2 + nr
    nl = nn * L
    b = np.linspace(-1.0, 1.0, n)
    pos = np.linspace(0.2, 0.8, 3 * nn)
    jac = np.linspace(-1.0, 2.0, 9 * nn)
    ring = np.linspace(-1.0, 1.0, 2 * nr)
    ins = [b, pos, jac, ring]
    before = [a.copy() for a in ins]
    for name in ENTRIES:
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = ([vp, vp, ctypes.c_int, vp, vp, ctypes.c_int, vp] + [ctypes.c_double] * 3 +
                                       [ctypes.c_int, ctypes.c_int, ctypes.c_int64] + [vp] * 13)

    def outputs():
        """each array with spare slots behind what a call may clear"""
        return [np.full(nn + 2, 7, dtype=np.int32), np.full(3 * nn + 2, np.nan), np.full(3 * nn + 2, np.nan),
                np.full(3 * nn + 2, np.nan), np.full(3 * nl + 2, np.nan), np.full(nl + 2, np.nan),
                np.full(nl + 2, 7, dtype=np.int32), np.full(nl + 2, 7, dtype=np.int32),
                np.full(nl + 2, 7, dtype=np.int32),
                np.full(nl + 3, 7, dtype=np.int64), np.full(2, 7, dtype=np.int64), np.full(3 * (cap + 2), np.nan),
                np.full(3 * (cap + 2), np.nan)]
    cleared = (nn, 3 * nn, 3 * nn, 3 * nn, 3 * nl, nl, nl, nl, nl, nl + 1, 1, 3 * cap, 3 * cap)

    def kept(a):
        return np.all((a == 7) | np.isnan(a)) if a.dtype.kind == "f" else np.all(a == 7)

    def ptrs(out):
        return [vp(a.ctypes.data) for a in out]

    def call(entry, h, nnulls=nn, nring=nr, radius=0.5, capture=0.5, step=0.5, max_steps=100, every=1, mp=cap, out=None,
             arrays=True):
        p = ptrs(out) if out is not None else [None] * 13
        i = [vp(a.ctypes.data) for a in ins] if arrays else [None] * 4
        return entry(h, i[0], nnulls, i[1], i[2], nring, i[3], radius, capture, step, max_steps, every, mp, *p)

    for h in (None, vp(1)):          # a NULL handle, and one the library never made: neither is looked at
        out = outputs()
        assert call(lib.ndsm_hip_vecpot_skeleton, h, out=out) == 9001
        # exactly the nnulls, nl, nl + 1 and cap slots are cleared; what lies behind them is not touched
        for a, m in zip(out, cleared):
            assert np.all(a[:m] == 0) and kept(a[m:])
        # a NULL bpt is skipped; max_points = 0: no point array is looked at
        out = outputs()
        p = ptrs(out)
        assert lib.ndsm_hip_vecpot_skeleton(h, vp(b.ctypes.data), nn, vp(pos.ctypes.data), vp(jac.ctypes.data), nr,
                                            vp(ring.ctypes.data), 0.5, 0.5, 0.5, 100, 1, cap, *p[:12], None) == 9001
        assert np.all(out[11][:3 * cap] == 0) and kept(out[12])
        out = outputs()
        assert call(lib.ndsm_hip_vecpot_skeleton, h, mp=0, out=out) == 9001
        assert out[10][0] == 0 and np.all(out[9][:nl + 1] == 0) and kept(out[11]) and kept(out[12])
        # bad scalars and NULL arrays: still 9001 whatever the arguments, total cleared, and no crash
        for kw in (dict(nnulls=-1), dict(nnulls=0), dict(nring=-1), dict(radius=0.0), dict(radius=float("nan")),
                   dict(radius=float("inf")), dict(capture=-1.0), dict(capture=float("nan")), dict(step=0.0),
                   dict(max_steps=0), dict(every=0), dict(mp=-1), dict(mp=-2 ** 62), dict(nring=2 ** 31 - 1),
                   dict(nnulls=2 ** 31 - 1, nring=0)):
            out = outputs()
            small = kw.get("nnulls", nn) <= nn and kw.get("nring", nr) <= nr
            assert call(lib.ndsm_hip_vecpot_skeleton, h, out=out if small else None, **kw) == 9001, kw
            if small:
                assert out[10][0] == 0 and out[10][1] == 7, kw
                if kw.get("mp", cap) < 0:
                    assert kept(out[11]) and kept(out[12])      # no capacity: no slot of a point array is cleared
                if kw.get("nnulls", nn) <= 0 or kw.get("nring", nr) < 0:
                    assert all(kept(a) for a in out[:10])       # no lines: no slot of a line array is cleared
        assert call(lib.ndsm_hip_vecpot_skeleton, h, arrays=False) == 9001
        # the device entry never reads or writes through its array arguments on the host; total is a host scalar
        out = outputs()
        assert call(lib.ndsm_hip_vecpot_skeleton_device, h, out=out) == 9001
        assert out[10][0] == 0 and out[10][1] == 7
        assert all(kept(a) for k, a in enumerate(out) if k != 10)
        assert call(lib.ndsm_hip_vecpot_skeleton_device, h, arrays=False) == 9001
    assert all(np.array_equal(a, c) for a, c in zip(ins, before))
    # the Python layer raises instead
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.find_skeleton(x, x, x, z, nulls=(np.full((1, 3), 0.5), np.diag([2.0, -1.0, -1.0])[None]))


def test_skeleton_python_names(lib):
    import ndsm_amd
    for name in ("Skeleton", "find_skeleton", "spine_of", "fan_of", "connections"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    assert ndsm_amd.Skeleton._fields == ("position", "kind", "eig", "spine", "normal", "paths", "hit")
    par = inspect.signature(ndsm_amd.VecPot.skeleton).parameters
    assert list(par)[1:] == ["b", "nulls", "radius", "nring", "ring", "capture", "step", "max_steps", "every",
                             "max_points", "values", "device"]
    assert [par[k].default for k in list(par)[2:]] == [None, 0.5, 16, None, None, 0.5, None, 1, None, True, False]
    par = inspect.signature(ndsm_amd.find_skeleton).parameters
    assert list(par)[:4] == ["x", "y", "z", "b"]
    assert ([par[k].default for k in ("nulls", "radius", "nring", "ring", "capture", "step", "max_steps", "every",
                                      "max_points", "values")] == [None, 0.5, 16, None, None, 0.5, None, 1, None, True])
    from ndsm_amd import _lib
    assert (_lib.SKEL_CAPTURED, _lib.SKEL_NONE) == (10, 11)
    # the default ring: the angles 2 pi (j + 1/2) / nring
    R = _lib._skeleton_ring(16, None)
    ang = 2.0 * np.pi * (np.arange(16) + 0.5) / 16
    assert R.shape == (16, 2) and np.array_equal(R, np.stack([np.cos(ang), np.sin(ang)], axis=1))
    assert _lib._skeleton_ring(0, None).shape == (0, 2)
    # capture=None means radius
    assert _lib._skeleton_args(0.7, 4, None, None)[:2] == (0.7, 0.7)
    assert _lib._skeleton_args(0.7, 4, None, 0)[:2] == (0.7, 0.0)


def test_skeleton_arguments_checked_before_any_device_call(lib):
    """bad options are a ValueError and arrays that do not fit an argument error (9002), before the library is
    called"""
    import ndsm_amd
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    nul = (np.full((2, 3), 0.5), np.stack([np.diag([2.0, -1.0, -1.0])] * 2))
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.find_skeleton(x, x, x[:7], z, nulls=nul)
    with pytest.raises(ValueError):
        ndsm_amd.find_skeleton(x, x, x, z, nulls=nul, radius=0.0)
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.nshape4 = np.array([8, 8, 8, 3], dtype=np.intc)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library reached: " + name)
    V.L, V.h = NoCalls(), None
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
               dict(radius=None), dict(radius="1"), dict(radius=True), dict(capture=-0.1), dict(capture=float("nan")),
               dict(capture=float("inf")), dict(capture="1"), dict(nring=-1), dict(nring=2.5), dict(nring=None),
               dict(nring=True), dict(nring=2 ** 21), dict(ring=np.zeros(4)), dict(ring=np.zeros((4, 3))),
               dict(step=0.0), dict(step=float("nan")), dict(max_steps=0), dict(max_steps=2.5), dict(every=0),
               dict(every=1.5), dict(every=None), dict(max_points=-1), dict(max_points=2.5), dict(max_points=2 ** 41)):
        with pytest.raises(ValueError):
            V.skeleton(z, nulls=nul, **kw)
    for bad in (np.zeros((3, 8, 8, 7)), np.zeros((8, 8, 8, 3))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.skeleton(bad, nulls=nul)
    for bad in ((np.zeros(3), nul[1]), (np.zeros((2, 2)), nul[1]), (nul[0], np.zeros((2, 9))), (nul[0], nul[1][:1])):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.skeleton(z, nulls=bad)
    # no nulls: an empty result, and still no call
    sk = V.skeleton(z, nulls=(np.zeros((0, 3)), np.zeros((0, 3, 3))), nring=5)
    assert sk.position.shape == (0, 3) and sk.kind.shape == (0,) and sk.hit.shape == (0, 7)
    assert sk.paths.lines.ends.shape == (0, 7, 3) and sk.paths.offsets.tolist() == [0]
    assert sk.paths.points.shape == sk.paths.b.shape == (0, 3) and ndsm_amd.connections(sk) == []
    assert V.skeleton(z, nulls=(np.zeros((0, 3)), np.zeros((0, 3, 3))), values=False).paths.b is None


def test_connections_on_a_hand_made_result():
    import ndsm_amd
    from ndsm_amd import _lib
    # three nulls, two ring seeds each: null 0's two fan lines end at nulls 2 and 1, null 2's first at null 0; a spine
    # line that is captured is not a connection
    n, nr = 3, 2
    L = 2 + nr
    status = np.full(n * L, 1, dtype=np.int32)
    hit = np.full(n * L, -1, dtype=np.int32)
    for l, m in ((2, 2), (3, 1), (2 * L + 2, 0), (L + 0, 2)):
        status[l], hit[l] = 10, m
    lines = [np.zeros((n * L, 3)), np.zeros(n * L), status, np.zeros(n * L, dtype=np.int32), hit]
    sk = _lib._skeleton_tuple(np.zeros((n, 3)), nr, [np.ones(n, dtype=np.int32)] + [np.zeros((n, 3))] * 3, lines,
                              np.arange(n * L + 1, dtype=np.int64), np.zeros((n * L, 3)), None)
    got = [(m, o, idx.tolist()) for m, o, idx in ndsm_amd.connections(sk)]
    assert got == [(0, 1, [1]), (0, 2, [0]), (2, 0, [0])]
    assert [len(p) for p, _b in ndsm_amd.fan_of(sk, 1)] == [1, 1] and ndsm_amd.spine_of(sk, 2)[0][1] is None
