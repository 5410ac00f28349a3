"""CPU tests of the entry points of the optimization method with a measurement term (include/ndsm_hip.h, part 2): the
two symbols are declared and exported, the header's prototypes are the ones the Python binding declares, the Python
names are there with the documented defaults, and without a GPU both entries fail cleanly - 9001 whatever the
arguments, never a crash, hist and info cleared, inputs untouched."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndsm_hip.h")
ENTRIES = ["ndsm_hip_vecpot_optimize_obs", "ndsm_hip_vecpot_optimize_obs_device"]
KINDS = "ppp" + "pppp" + "di" + "iii" + "ddd" + "pip"


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def header_kinds(name):
    """'p' (pointer or array), 'i' (int) or 'd' (double) per parameter of the header's prototype"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    kinds = []
    for a in (" ".join(a.split()) for a in decl.split(",")):
        if "*" in a or "[" in a:
            kinds.append("p")
        elif re.match(r"(const )?int \w+$", a):
            kinds.append("i")
        elif re.match(r"(const )?double \w+$", a):
            kinds.append("d")
        else:
            raise AssertionError((name, a))
    return "".join(kinds)


def ctypes_kinds(fn):
    out = []
    for t in fn.argtypes:
        if t is ctypes.c_int:
            out.append("i")
        elif t is ctypes.c_double:
            out.append("d")
        else:
            assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), t
            out.append("p")
    return "".join(out)


def test_optimize_obs_entries_declared_exported_and_bound(lib):
    import ndsm_amd
    out = subprocess.check_output(["nm", "-D", "--defined-only", ndsm_amd.lib_path()], text=True)
    live = {l.split()[-1] for l in out.splitlines() if re.search(r" T ", l)}
    for name in ENTRIES:
        assert name in live, name
        assert hasattr(lib, name)
        assert header_kinds(name) == KINDS, (name, header_kinds(name))
        assert ctypes_kinds(getattr(lib, name)) == KINDS, name
    # the kernels behind them stay internal
    assert not any(s.startswith("ndsmk_") for s in live)
    text = open(HEADER).read()
    for phrase in ("Measurement errors", "Wiegelmann & Inhester", "Bobs", "wm", "L_m", "free", "2 / h_z", "rim"):
        assert phrase in text, phrase
    kernels = open(os.path.join(ROOT, "ndsm_amd", "csrc", "ndsm_kernels.h")).read()
    for name in ("ndsmk_optimize_obs_begin", "ndsmk_optimize_obs_tries", "ndsmk_optimize_obs_row"):
        assert name in kernels, name
    assert "optimize_obs" in open(os.path.join(ROOT, "ndsm_amd", "Makefile")).read().split("HIPSRC")[1].split("\n")[0]


def test_optimize_obs_python_names(lib):
    import ndsm_amd
    for name in ("measurement_weight", "force_free_optimize_obs"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    par = inspect.signature(ndsm_amd.VecPot.optimize_obs).parameters
    names = ["b", "bobs", "wm", "nu", "free", "w", "start", "niter_max", "check", "tol", "dt0", "dt_min", "hist_rows"]
    assert list(par)[1:14] == names
    assert [par[k].default for k in names[1:] + ["device"]] == [None, None, 0.01, True, None, "potential", 10000, 50,
                                                               1e-4, None, None, None, False]
    assert par["vc_tol"].default == 1e-10 and par["ms"].default == 5
    # what the two calls share has the defaults of optimize()
    old = inspect.signature(ndsm_amd.VecPot.optimize).parameters
    assert all(par[k].default == old[k].default for k in old if k != "self")
    one = inspect.signature(ndsm_amd.force_free_optimize_obs).parameters
    assert list(one)[:4] == ["x", "y", "z", "b"] and list(one)[4:16] == names[1:]
    assert [one[k].default for k in names[1:]] == [par[k].default for k in names[1:]]
    mw = inspect.signature(ndsm_amd.measurement_weight).parameters
    assert list(mw) == ["bobs", "floor"] and mw["floor"].default == 0.0


def test_optimize_obs_entries_fail_cleanly_without_a_gpu(lib):
    if lib.ndsm_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    import ndsm_amd
    # a CDLL object of its own (the same loaded library): prototypes set here stay private to this test
    L = ctypes.CDLL(ndsm_amd.lib_path(), mode=os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, "RTLD_DEEPBIND", 0))
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    for name in ENTRIES:
        fn = getattr(L, name)
        fn.restype = ci
        fn.argtypes = [{"p": vp, "i": ci, "d": cd}[k] for k in header_kinds(name)]
    n = 8 ** 3
    b, w = np.linspace(-1.0, 1.0, 3 * n), np.linspace(0.5, 1.5, n)
    bobs, wm = np.linspace(-2.0, 2.0, 3 * 64), np.linspace(0.1, 1.0, 3 * 64)
    keep = [v.copy() for v in (b, w, bobs, wm)]
    ioptc, ropt = np.zeros(16, dtype=np.intc), np.zeros(16)
    nan, inf = float("nan"), float("inf")

    def p(v):
        return None if v is None else vp(v.ctypes.data)

    good = (0.1, 1, 0, 10, 5, 1e-4, 1e-3, 1e-9, 4)      # nu free start niter check tol dt0 dt_min rows
    cases = [good, (0.0, 0, 1, 10, 5, 0.0, 1e-3, 0.0, 2)]
    for pos, bad in ((0, -1.0), (0, nan), (0, inf), (1, 2), (1, -1), (2, 2), (3, 0), (4, 0), (5, -1.0), (5, nan),
                     (6, 0.0), (6, inf), (7, -1.0), (7, nan), (8, 1)):
        cases.append(good[:pos] + (bad,) + good[pos + 1:])
    for h in (None, vp(1)):          # a NULL handle, and one the library never made: neither is looked at
        for name in ENTRIES:
            fn = getattr(L, name)
            for args in cases:
                rows = args[8]
                hist, info = np.full((4, 7), nan), np.full(3, 77, dtype=np.intc)
                for wt, cf in ((w, wm), (None, None)):
                    rc = fn(h, p(ioptc), p(ropt), p(b), p(wt), p(bobs), p(cf), *args[:8], p(hist), rows, p(info))
                    assert rc == 9001, (name, args)
                    # what lives on the host in both entries is cleared: the rows the call was given, and info
                    assert np.all(info == 0) and np.all(hist[:rows] == 0.0) and np.all(np.isnan(hist[rows:]))
            for rows in (0, -3):     # no rows to clear, and none touched
                hist, info = np.full((4, 7), nan), np.full(3, 77, dtype=np.intc)
                assert fn(h, p(ioptc), p(ropt), p(b), p(w), p(bobs), p(wm), *good[:8], p(hist), rows, p(info)) == 9001
                assert np.all(info == 0) and np.all(np.isnan(hist))
            assert fn(h, p(ioptc), p(ropt), None, None, None, None, *good[:8], None, 4, None) == 9001
    for v, k in zip((b, w, bobs, wm), keep):
        assert np.array_equal(v, k)
    assert not ioptc.any() and not ropt.any()
    # the Python layer raises instead
    x = np.linspace(0, 1, 8)
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.force_free_optimize_obs(x, x, x, np.zeros((3, 8, 8, 8)))


def test_optimize_obs_arguments_checked_before_any_device_call(lib):
    """arrays that do not fit are an argument error (9002) and bad options a ValueError, before the library is
    called"""
    import ndsm_amd
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.nshape4 = np.array([8, 7, 6, 3], dtype=np.intc)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library reached: " + name)
    V.L, V.h = NoCalls(), None
    z, w, pl = np.zeros((3, 6, 7, 8)), np.ones((6, 7, 8)), np.ones((3, 7, 8))
    for bad in (np.zeros((3, 6, 7, 7)), np.zeros((6, 7, 8)), np.zeros(3 * 6 * 7 * 8)):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.optimize_obs(bad, pl, pl, w=w)
    for bad in (np.ones((8, 7, 6)), np.ones((3, 6, 7, 8)), np.ones(6 * 7 * 8), np.ones((7, 8))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.optimize_obs(z, pl, pl, w=bad)
    for bad in (np.ones((3, 8, 7)), np.ones((7, 8)), np.ones((7, 8, 3)), np.ones((3, 6, 7, 8)), np.ones(3 * 7 * 8)):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.optimize_obs(z, bad, pl)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.optimize_obs(z, pl, bad)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.optimize_obs(z, None, bad)
    for kw in (dict(nu=-0.1), dict(nu=float("nan")), dict(nu=float("inf")), dict(free=2), dict(free=-1),
               dict(free="yes"), dict(free=None), dict(niter_max=0), dict(niter_max=2.5), dict(check=0),
               dict(check=-1), dict(tol=-1e-3), dict(tol=float("nan")), dict(tol=float("inf")), dict(dt0=0.0),
               dict(dt0=-1.0), dict(dt0=float("inf")), dict(dt0=float("nan")), dict(dt_min=-1.0),
               dict(dt_min=float("nan")), dict(hist_rows=1), dict(hist_rows=2.5), dict(start="zero"), dict(start=0),
               dict(start=None)):
        with pytest.raises(ValueError):
            V.optimize_obs(z, pl, pl, w=w, **kw)
