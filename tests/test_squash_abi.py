"""CPU tests of the squashing-factor entry points (include/ndsm_hip.h, part 2): they are declared, exported,
reachable from Python with the documented defaults, and fail cleanly - an error code, never a crash, outputs
cleared, inputs untouched - without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndsm_hip.h")
ENTRIES = ["ndsm_hip_vecpot_squash", "ndsm_hip_vecpot_squash_device"]


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_squash_entries_declared_and_exported(lib):
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    import ndsm_amd
    out = subprocess.check_output(["nm", "-D", "--defined-only", ndsm_amd.lib_path()], text=True)
    live = {l.split()[-1] for l in out.splitlines() if re.search(r" T ", l)}
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in live, name
        assert hasattr(lib, name)
    # the kernel behind them stays internal
    assert not any(s.startswith("ndsmk_squash") for s in live)
    kern = open(os.path.join(ROOT, "ndsm_amd", "csrc", "ndsm_kernels.h")).read()
    assert re.search(r"\bint\s+ndsmk_squash\s*\(", kern)
    # fourteen arguments, in the documented order
    for name in ENTRIES:
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)", src, flags=re.S).group(1).split(",")
        assert len(args) == 14, (name, args)
        assert "integrand" in args[3] and "nseeds" in args[4] and "step" in args[6] and "max_steps" in args[7]
        assert "q" in args[8] and "ends" in args[9] and "nsteps" in args[13]
    # the header states the semantics, and that the end points are not those of trace
    for phrase in ("Scott, Pontin & Hornig", "two\n *              refinements, always two", "integrand  0", "U0",
                   "END POINTS THEREFORE DIFFER", "Not clamped to >= 2", "|B|^2 / |B_a B_c|", "d/dy = (e0 + fz (e1 - e0)) / h_y"):
        assert phrase in text, phrase
    # the trace kernel's file is restated, not changed or shared
    sq = open(os.path.join(ROOT, "ndsm_amd", "csrc", "squash.hip")).read()
    assert "squash_k" in sq and "trace.hip" not in re.sub(r"//.*", "", sq)
    assert " squash " in open(os.path.join(ROOT, "ndsm_amd", "Makefile")).read()


def test_squash_entries_fail_cleanly_without_a_gpu(lib):
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
        getattr(lib, name).argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_double, ctypes.c_int] + [vp] * 6

    def outputs():
        """each with slack behind the slots the entry owns: q nseeds, the others 2 nseeds (ends 3 each)"""
        return [np.full(ns + 3, np.nan), np.full(2 * 3 * ns + 3, np.nan), np.full(2 * ns + 3, np.nan),
                np.full(2 * ns + 3, np.nan), np.full(2 * ns + 3, 7, dtype=np.int32),
                np.full(2 * ns + 3, 7, dtype=np.int32)]
    owned = [ns, 6 * ns, 2 * ns, 2 * ns, 2 * ns, 2 * ns]

    for h in (None, vp(1)):          # a NULL handle, and one the library never made: neither is looked at
        for integrand, gg in ((0, g), (1, g), (1, b), (0, None)):
            out = outputs()
            rc = lib.ndsm_hip_vecpot_squash(h, vp(b.ctypes.data), None if gg is None else vp(gg.ctypes.data), integrand,
                                            ns, vp(seeds.ctypes.data), 0.5, 100, *[vp(a.ctypes.data) for a in out])
            assert rc == 9001
            for a, m in zip(out, owned):      # exactly the owned slots are cleared
                assert np.all(a[:m] == 0), integrand
                assert np.all((a[m:] == 7) | np.isnan(a[m:])), integrand
        # bad scalars and NULL arrays: still 9001, and no crash
        for args in ((0, ns, 0.0, 100), (0, ns, 0.5, 0), (2, ns, 0.5, 100), (-1, ns, 0.5, 100), (0, -1, 0.5, 100),
                     (0, 0, 0.5, 100)):
            out = outputs()
            rc = lib.ndsm_hip_vecpot_squash(h, vp(b.ctypes.data), None, args[0], args[1], vp(seeds.ctypes.data), args[2],
                                            args[3], *[vp(a.ctypes.data) for a in out])
            assert rc == 9001, args
        assert lib.ndsm_hip_vecpot_squash(h, None, None, 0, ns, None, 0.5, 100, None, None, None, None, None,
                                          None) == 9001
        # the device entry never reads or writes through its array arguments on the host
        out = outputs()
        rc = lib.ndsm_hip_vecpot_squash_device(h, vp(b.ctypes.data), vp(g.ctypes.data), 1, ns, vp(seeds.ctypes.data),
                                               0.5, 100, *[vp(a.ctypes.data) for a in out])
        assert rc == 9001
        assert np.all(np.isnan(out[0])) and np.all(np.isnan(out[1])) and np.all(out[4] == 7)
        assert lib.ndsm_hip_vecpot_squash_device(h, None, None, 0, ns, None, 0.5, 100, None, None, None, None, None,
                                                 None) == 9001
    assert np.array_equal(b, b0) and np.array_equal(g, g0) and np.array_equal(seeds, s0)
    # the Python layer raises instead
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    sd = np.full((4, 3), 0.5)
    for kw in ({}, dict(twist=True), dict(g=z, integrand=1)):
        with pytest.raises(ndsm_amd.NdsmHipError):
            ndsm_amd.squashing_factor(x, x, x, z, sd, **kw)


def test_squash_python_names(lib):
    import ndsm_amd
    for name in ("QMap", "squashing_factor", "seed_plane"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    assert ndsm_amd.QMap._fields == ("q", "twist", "ends", "length", "integral", "status", "nsteps")
    par = inspect.signature(ndsm_amd.VecPot.squashing).parameters
    assert list(par)[1:] == ["b", "seeds", "g", "integrand", "twist", "step", "max_steps", "device"]
    assert (par["g"].default, par["integrand"].default, par["twist"].default, par["step"].default,
            par["max_steps"].default, par["device"].default) == (None, 0, False, 0.5, None, False)
    par = inspect.signature(ndsm_amd.squashing_factor).parameters
    assert list(par)[:5] == ["x", "y", "z", "b", "seeds"]
    assert (par["g"].default, par["integrand"].default, par["twist"].default, par["step"].default,
            par["max_steps"].default) == (None, 0, False, 0.5, None)
    assert list(inspect.signature(ndsm_amd.VecPot.seed_plane).parameters)[1:] == ["axis", "value", "n1", "n2"]
    assert list(inspect.signature(ndsm_amd.seed_plane).parameters) == ["x", "y", "z", "axis", "value", "n1", "n2"]
    # existing signatures are unchanged
    par = inspect.signature(ndsm_amd.VecPot.trace).parameters
    assert list(par)[1:] == ["b", "seeds", "g", "step", "max_steps", "direction", "device"]
    assert (par["g"].default, par["step"].default, par["max_steps"].default, par["direction"].default,
            par["device"].default) == (None, 0.5, None, "both", False)
    assert ndsm_amd.FieldLines._fields == ("ends", "length", "integral", "status", "nsteps", "flh")


def test_seed_plane():
    import ndsm_amd
    x, y, z = 0.25 + 0.1 * np.arange(6), -0.4 + 0.07 * np.arange(9), 1.1 + 0.13 * np.arange(5)
    lo = [q[0] for q in (x, y, z)]
    hi = [q[0] + (len(q) - 1.0) * (q[1] - q[0]) for q in (x, y, z)]
    for axis, (a1, a2) in ((0, (1, 2)), (1, (0, 2)), (2, (0, 1))):
        s = ndsm_amd.seed_plane(x, y, z, axis, 0.5 * (lo[axis] + hi[axis]), 4, 3)
        assert s.shape == (12, 3) and s.dtype == np.float64
        assert np.all(s[:, axis] == 0.5 * (lo[axis] + hi[axis]))
        g = s.reshape(3, 4, 3)
        assert np.all(g[:, 0, a1] == lo[a1]) and np.all(g[:, -1, a1] == hi[a1])       # face to face, a1 fastest
        assert np.all(g[0, :, a2] == lo[a2]) and np.all(g[-1, :, a2] == hi[a2])
        assert np.all(np.diff(g[0, :, a1]) > 0) and np.all(np.diff(g[:, 0, a2]) > 0)
        assert np.all((s >= lo) & (s <= hi))
    assert ndsm_amd.seed_plane(x, y, z, 2, z[0], 1, 1).tolist() == [[x[0], y[0], z[0]]]
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.x, V.y, V.z = x, y, z
    assert np.array_equal(V.seed_plane(1, 0.0, 5, 2), ndsm_amd.seed_plane(x, y, z, 1, 0.0, 5, 2))
    for bad in (dict(axis=3), dict(axis=-1), dict(axis="x"), dict(n1=0), dict(n2=2.5)):
        kw = dict(axis=0, value=0.5, n1=3, n2=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            ndsm_amd.seed_plane(x, y, z, **kw)


def test_squash_arguments_checked_before_any_device_call(lib):
    """bad options are a ValueError and arrays that do not fit an argument error (9002), before the library is
    called"""
    import ndsm_amd
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    sd = np.full((4, 3), 0.5)
    with pytest.raises(ValueError):
        ndsm_amd.squashing_factor(x, x, x, z, sd, g=z, twist=True)
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.squashing_factor(x, x, x[:7], z, sd)
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
            V.squashing(z, sd, **kw)
    for bad in (np.zeros((3, 8, 8, 7)), np.zeros((2, 8, 8, 8)), np.zeros((8, 8, 8, 3))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.squashing(bad, sd)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.squashing(bad, sd, twist=True)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.squashing(z, sd, g=bad)
    for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((3, 4, 3))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.squashing(z, bad)
    # no seeds: an empty QMap, and still no call
    for kw in ({}, dict(g=z, integrand=1), dict(twist=True)):
        m = V.squashing(z, np.zeros((0, 3)), **kw)
        assert m.q.shape == (0,) and m.ends.shape == (2, 0, 3) and m.length.shape == (2, 0)
        assert m.status.dtype == np.int32 and m.nsteps.dtype == np.int32 and m.status.shape == (2, 0)
        assert (m.twist is None) == ("twist" not in kw)
        if "twist" in kw:
            assert m.twist.shape == (0,)
