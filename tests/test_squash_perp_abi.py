"""CPU tests of the perpendicular-squashing-factor entry points (include/ndsm_hip.h): they are declared, exported,
reachable from Python with the documented names and defaults, and fail cleanly - an error code, never a crash, q and
qperp cleared over exactly nseeds slots, inputs untouched - without a GPU; seed_cut, the oblique cut that goes with
them, is host code and is checked in full."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndsm_hip.h")
ENTRIES = ["ndsm_hip_vecpot_squash_perp", "ndsm_hip_vecpot_squash_perp_device"]


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_squash_perp_entries_declared_and_exported(lib):
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    import ndsm_amd
    out = subprocess.check_output(["nm", "-D", "--defined-only", ndsm_amd.lib_path()], text=True)
    live = {l.split()[-1] for l in out.splitlines() if re.search(r" T ", l)}
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in live, name
        assert hasattr(lib, name)
        # the squash entry's fourteen arguments and qperp after q
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)", src, flags=re.S).group(1).split(",")
        assert len(args) == 15, (name, args)
        assert "integrand" in args[3] and "nseeds" in args[4] and "step" in args[6] and "max_steps" in args[7]
        assert re.search(r"\*d?q$", args[8].strip()) and "qperp" in args[9] and "ends" in args[10]
        assert "nsteps" in args[14]
    # the kernel entry behind them stays internal, next to the one it shares its kernel with
    assert not any(s.startswith("ndsmk_") for s in live)
    kern = open(os.path.join(ROOT, "ndsm_amd", "csrc", "ndsm_kernels.h")).read()
    assert re.search(r"\bint\s+ndsmk_squash_perp\s*\(", kern) and re.search(r"\bint\s+ndsmk_squash\s*\(", kern)
    sq = open(os.path.join(ROOT, "ndsm_amd", "csrc", "squash.hip")).read()
    assert "template <bool kHasG, bool kPerp>" in sq
    # the header states the semantics, operand order included
    for phrase in ("me = sqrt((Bx Bx + By By) + Bz Bz) of B_e", "du = (U_x e_x + U_y e_y) + U_z e_z",
                   "Up = U - du e, Vp = V - dv e",
                   "Q-perp = (((puu_F pvv_B + puu_B pvv_F) - 2 (puv_F puv_B)) * me_F) * me_B / |B_s|^2",
                   "does NOT need b_n > 0", "Not clamped to >= 2, as Q is not",
                   "are the bits of ndsm_hip_vecpot_squash on the same\n * arguments"):
        assert phrase in text, phrase


def test_squash_perp_entries_fail_cleanly_without_a_gpu(lib):
    if lib.ndsm_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    import ndsm_amd
    # a CDLL object of its own (the same loaded library): prototypes set here stay private to this test
    lib = ctypes.CDLL(ndsm_amd.lib_path(), mode=os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, "RTLD_DEEPBIND", 0))
    vp = ctypes.c_void_p
    n, ns = 3 * 8 ** 3, 5
    b = np.linspace(-1.0, 1.0, n)
    g = np.linspace(2.0, 3.0, n)
    seeds = np.linspace(0.1, 0.9, 3 * ns)
    b0, g0, s0 = b.copy(), g.copy(), seeds.copy()
    for name in ENTRIES:
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = ([vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_double, ctypes.c_int] +
                                       [vp] * 7)

    def outputs():
        """each with slack behind the slots the entry owns: q and qperp nseeds, the others 2 nseeds (ends 3 each)"""
        return [np.full(ns + 3, np.nan), np.full(ns + 3, np.nan), np.full(2 * 3 * ns + 3, np.nan),
                np.full(2 * ns + 3, np.nan), np.full(2 * ns + 3, np.nan), np.full(2 * ns + 3, 7, dtype=np.int32),
                np.full(2 * ns + 3, 7, dtype=np.int32)]
    owned = [ns, ns, 6 * ns, 2 * ns, 2 * ns, 2 * ns, 2 * ns]

    for h in (None, vp(1)):          # a NULL handle, and one the library never made: neither is looked at
        for integrand, gg in ((0, g), (1, g), (1, b), (0, None)):
            out = outputs()
            rc = lib.ndsm_hip_vecpot_squash_perp(h, vp(b.ctypes.data), None if gg is None else vp(gg.ctypes.data),
                                                 integrand, ns, vp(seeds.ctypes.data), 0.5, 100,
                                                 *[vp(a.ctypes.data) for a in out])
            assert rc == 9001
            for a, m in zip(out, owned):      # exactly the owned slots are cleared
                assert np.all(a[:m] == 0), integrand
                assert np.all((a[m:] == 7) | np.isnan(a[m:])), integrand
        # bad scalars and NULL arrays: still 9001, and no crash
        for args in ((0, ns, 0.0, 100), (0, ns, 0.5, 0), (2, ns, 0.5, 100), (-1, ns, 0.5, 100), (0, -1, 0.5, 100),
                     (0, 0, 0.5, 100)):
            out = outputs()
            rc = lib.ndsm_hip_vecpot_squash_perp(h, vp(b.ctypes.data), None, args[0], args[1], vp(seeds.ctypes.data),
                                                 args[2], args[3], *[vp(a.ctypes.data) for a in out])
            assert rc == 9001, args
            if args[1] <= 0:
                assert all(np.all((a == 7) | np.isnan(a)) for a in out)         # no seeds: nothing is touched
        assert lib.ndsm_hip_vecpot_squash_perp(h, None, None, 0, ns, None, 0.5, 100, *([None] * 7)) == 9001
        # a NULL qperp alone: the others are still cleared
        out = outputs()
        ptrs = [vp(a.ctypes.data) for a in out]
        ptrs[1] = None
        assert lib.ndsm_hip_vecpot_squash_perp(h, vp(b.ctypes.data), None, 0, ns, vp(seeds.ctypes.data), 0.5, 100,
                                               *ptrs) == 9001
        assert np.all(out[0][:ns] == 0) and np.all(np.isnan(out[1])) and np.all(out[6][:2 * ns] == 0)
        # the device entry never reads or writes through its array arguments on the host
        out = outputs()
        rc = lib.ndsm_hip_vecpot_squash_perp_device(h, vp(b.ctypes.data), vp(g.ctypes.data), 1, ns,
                                                    vp(seeds.ctypes.data), 0.5, 100, *[vp(a.ctypes.data) for a in out])
        assert rc == 9001
        assert all(np.all(np.isnan(a)) for a in out[:5]) and np.all(out[5] == 7) and np.all(out[6] == 7)
        assert lib.ndsm_hip_vecpot_squash_perp_device(h, None, None, 0, ns, None, 0.5, 100, *([None] * 7)) == 9001
    assert np.array_equal(b, b0) and np.array_equal(g, g0) and np.array_equal(seeds, s0)
    # the Python layer raises instead
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    sd = np.full((4, 3), 0.5)
    for kw in ({}, dict(twist=True), dict(g=z, integrand=1)):
        with pytest.raises(ndsm_amd.NdsmHipError):
            ndsm_amd.perpendicular_squashing(x, x, x, z, sd, **kw)


def test_squash_perp_python_names(lib):
    import ndsm_amd
    for name in ("QPerpMap", "perpendicular_squashing", "seed_cut"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    assert ndsm_amd.QPerpMap._fields == ("q", "q_perp", "twist", "ends", "length", "integral", "status", "nsteps")
    par = inspect.signature(ndsm_amd.VecPot.squashing_perp).parameters
    assert list(par)[1:] == ["b", "seeds", "g", "integrand", "twist", "step", "max_steps", "device"]
    assert (par["g"].default, par["integrand"].default, par["twist"].default, par["step"].default,
            par["max_steps"].default, par["device"].default) == (None, 0, False, 0.5, None, False)
    par = inspect.signature(ndsm_amd.perpendicular_squashing).parameters
    assert list(par)[:5] == ["x", "y", "z", "b", "seeds"]
    assert (par["g"].default, par["integrand"].default, par["twist"].default, par["step"].default,
            par["max_steps"].default) == (None, 0, False, 0.5, None)
    assert list(inspect.signature(ndsm_amd.VecPot.seed_cut).parameters)[1:] == ["origin", "e1", "e2", "n1", "n2"]
    assert list(inspect.signature(ndsm_amd.seed_cut).parameters) == ["x", "y", "z", "origin", "e1", "e2", "n1", "n2"]
    # what was there is unchanged
    assert ndsm_amd.QMap._fields == ("q", "twist", "ends", "length", "integral", "status", "nsteps")
    par = inspect.signature(ndsm_amd.VecPot.squashing).parameters
    assert list(par)[1:] == ["b", "seeds", "g", "integrand", "twist", "step", "max_steps", "device"]
    assert (par["g"].default, par["integrand"].default, par["twist"].default, par["step"].default,
            par["max_steps"].default, par["device"].default) == (None, 0, False, 0.5, None, False)
    assert list(inspect.signature(ndsm_amd.squashing_factor).parameters) == [
        "x", "y", "z", "b", "seeds", "g", "integrand", "twist", "step", "max_steps", "lib"]


def test_seed_cut():
    import ndsm_amd
    x, y, z = 0.25 + 0.1 * np.arange(6), -0.4 + 0.07 * np.arange(9), 1.1 + 0.13 * np.arange(5)
    o, e1, e2 = np.array([0.3, -0.3, 1.2]), np.array([0.4, 0.2, 0.0]), np.array([-0.1, 0.1, 0.4])
    s = ndsm_amd.seed_cut(x, y, z, o, e1, e2, 4, 3)
    assert s.shape == (12, 3) and s.dtype == np.float64
    g = s.reshape(3, 4, 3)
    # origin + s e1 + t e2, s fastest (seed_plane's ordering), s and t equally spaced from 0 to 1
    for j in range(3):
        for i in range(4):
            assert np.allclose(g[j, i], o + (i / 3.0) * e1 + (j / 2.0) * e2, rtol=0, atol=1e-15)
    assert np.array_equal(g[0, 0], o) and np.array_equal(g[0, -1], o + e1) and np.array_equal(g[-1, 0], o + e2)
    assert np.array_equal(g[-1, -1], o + e1 + e2)
    # the mesh-aligned cut is the special case
    lo = np.array([x[0], y[0], z[0]])
    hi = lo + np.array([(len(q) - 1.0) * (q[1] - q[0]) for q in (x, y, z)])
    plane = ndsm_amd.seed_plane(x, y, z, 2, 1.3, 5, 4)
    cut = ndsm_amd.seed_cut(x, y, z, [lo[0], lo[1], 1.3], [hi[0] - lo[0], 0, 0], [0, hi[1] - lo[1], 0], 5, 4)
    assert np.allclose(cut, plane, rtol=0, atol=1e-15)
    # a single point per direction is the origin; lists and tuples are taken; points outside the box are allowed
    assert ndsm_amd.seed_cut(x, y, z, o, e1, e2, 1, 1).tolist() == [o.tolist()]
    assert ndsm_amd.seed_cut(x, y, z, o, e1, e2, 1, 3).shape == (3, 3)
    far = ndsm_amd.seed_cut(x, y, z, (9.0, 9.0, 9.0), [1, 0, 0], [0, 1, 0], 2, 2)
    assert far.shape == (4, 3) and np.all(far >= 9.0)
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.x, V.y, V.z = x, y, z
    assert np.array_equal(V.seed_cut(o, e1, e2, 5, 2), ndsm_amd.seed_cut(x, y, z, o, e1, e2, 5, 2))
    for bad in (dict(n1=0), dict(n2=0), dict(n1=-2), dict(n2=2.5), dict(origin=[0.0, 1.0]), dict(e1=[0.0, np.nan, 1.0]),
                dict(e2=[0.0, np.inf, 1.0]), dict(e1=np.zeros((3, 3))), dict(origin="abc"), dict(e2=None)):
        kw = dict(origin=o, e1=e1, e2=e2, n1=3, n2=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            ndsm_amd.seed_cut(x, y, z, **kw)


def test_squash_perp_arguments_checked_before_any_device_call(lib):
    """bad options are a ValueError and arrays that do not fit an argument error (9002), before the library is
    called"""
    import ndsm_amd
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    sd = np.full((4, 3), 0.5)
    with pytest.raises(ValueError):
        ndsm_amd.perpendicular_squashing(x, x, x, z, sd, g=z, twist=True)
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.perpendicular_squashing(x, x, x[:7], z, sd)
    # VecPot itself: a handle object whose library would fail the test if it were reached
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.nshape4 = np.array([8, 8, 8, 3], dtype=np.intc)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library reached: " + name)
    V.L, V.h = NoCalls(), None
    for kw in (dict(step=0.0), dict(step=-0.5), dict(step=float("nan")), dict(step=float("inf")), dict(max_steps=0),
               dict(max_steps=-3), dict(max_steps=2.5), dict(integrand=2), dict(integrand=-1), dict(integrand=None),
               dict(integrand=0.5), dict(integrand=True), dict(g=z, twist=True), dict(g=z, integrand=1, twist=True)):
        with pytest.raises(ValueError):
            V.squashing_perp(z, sd, **kw)
    for bad in (np.zeros((3, 8, 8, 7)), np.zeros((2, 8, 8, 8)), np.zeros((8, 8, 8, 3))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.squashing_perp(bad, sd)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.squashing_perp(bad, sd, twist=True)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.squashing_perp(z, sd, g=bad)
    for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((3, 4, 3))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.squashing_perp(z, bad)
    # no seeds: an empty QPerpMap, and still no call
    for kw in ({}, dict(g=z, integrand=1), dict(twist=True)):
        m = V.squashing_perp(z, np.zeros((0, 3)), **kw)
        assert isinstance(m, ndsm_amd.QPerpMap)
        assert m.q.shape == (0,) and m.q_perp.shape == (0,) and m.ends.shape == (2, 0, 3) and m.length.shape == (2, 0)
        assert m.status.dtype == np.int32 and m.nsteps.dtype == np.int32 and m.status.shape == (2, 0)
        assert (m.twist is None) == ("twist" not in kw)
        if "twist" in kw:
            assert m.twist.shape == (0,)
