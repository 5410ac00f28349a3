"""CPU tests of the resampling and cascade entry points (include/ndsm_hip.h): the four symbols are declared and
exported, the header's prototypes are the ones the Python binding declares, the launcher behind them stays internal, the
Python names are there with the documented defaults, without a GPU every entry fails cleanly - 9001 whatever the
arguments, never a crash, hist and info cleared, B and dst untouched - and VecPot.optimize_cascade checks its arguments
before it reaches the library."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndsm_hip.h")
KINDS = {"ndsm_hip_resample": "ppiipp", "ndsm_hip_resample_device": "ppiipp",
         "ndsm_hip_vecpot_optimize_cascade": "pi" + "pp" + "pp" + "ipid" + "ppp" + "ip",
         "ndsm_hip_vecpot_optimize_cascade_device": "pi" + "pp" + "pp" + "ipid" + "ppp" + "ip"}


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


def test_cascade_entries_declared_exported_and_bound(lib):
    import ndsm_amd
    out = subprocess.check_output(["nm", "-D", "--defined-only", ndsm_amd.lib_path()], text=True)
    live = {l.split()[-1] for l in out.splitlines() if re.search(r" T ", l)}
    for name, kinds in KINDS.items():
        assert name in live, name
        assert hasattr(lib, name)
        assert header_kinds(name) == kinds, (name, header_kinds(name))
        assert ctypes_kinds(getattr(lib, name)) == kinds, name
    # the launchers behind them stay internal
    assert not any(s.startswith("ndsmk_") for s in live)
    kernels = open(os.path.join(ROOT, "ndsm_amd", "csrc", "ndsm_kernels.h")).read()
    assert "ndsmk_resample" in kernels and "ndsmk_resample" not in open(HEADER).read()
    assert "resample" in open(os.path.join(ROOT, "ndsm_amd", "Makefile")).read().split("HIPSRC")[1].split("\n")[0]
    assert "__launch_bounds__" in open(os.path.join(ROOT, "ndsm_amd", "csrc", "resample.hip")).read()
    text = open(HEADER).read()
    for phrase in ("Coarse-to-fine cascade", "hat average", "linear interpolation", "nlevels", "same box", "k = 0 plane"):
        assert phrase in text, phrase


def test_cascade_python_names(lib):
    import ndsm_amd
    for name in ("resample", "cascade_shapes", "force_free_cascade"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    par = inspect.signature(ndsm_amd.VecPot.optimize_cascade).parameters
    names = ["coarser", "b", "w", "start", "niter_max", "check", "tol", "dt0", "dt_min", "hist_rows"]
    assert list(par)[1:11] == names
    shared = names[2:]
    assert [par[k].default for k in shared + ["device"]] == [None, "potential", 10000, 50, 1e-4, None, None, None, False]
    single = inspect.signature(ndsm_amd.VecPot.optimize).parameters
    assert list(par)[11:] == list(single)[10:]                       # the solve options and device, as optimize()
    assert [par[k].default for k in list(par)[11:]] == [single[k].default for k in list(single)[10:]]
    one = inspect.signature(ndsm_amd.force_free_cascade).parameters
    assert list(one)[:6] == ["x", "y", "z", "b", "levels", "shapes"] and list(one)[6:14] == shared
    assert one["levels"].default == 3 and one["shapes"].default is None
    assert [one[k].default for k in shared] == [par[k].default for k in shared]
    rs = inspect.signature(ndsm_amd.resample).parameters
    assert list(rs) == ["a", "shape", "mode", "device", "lib"]
    assert (rs["mode"].default, rs["device"].default, rs["lib"].default) == ("linear", False, None)
    cs = inspect.signature(ndsm_amd.cascade_shapes).parameters
    assert list(cs) == ["shape", "levels", "min_nodes"] and cs["min_nodes"].default == 4


def test_cascade_entries_fail_cleanly_without_a_gpu(lib):
    if lib.ndsm_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    import ndsm_amd
    # a CDLL object of its own (the same loaded library): prototypes set here stay private to this test
    L = ctypes.CDLL(ndsm_amd.lib_path(), mode=os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, "RTLD_DEEPBIND", 0))
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    for name in KINDS:
        fn = getattr(L, name)
        fn.restype = ci
        fn.argtypes = [{"p": vp, "i": ci, "d": cd}[k] for k in header_kinds(name)]
    nan, inf = float("nan"), float("inf")

    def p(v):
        return None if v is None else vp(v.ctypes.data)

    # ---- resample: good and bad arguments alike
    src = np.linspace(-1.0, 1.0, 2 * 6 * 5 * 4)
    keep = src.copy()
    for name in ("ndsm_hip_resample", "ndsm_hip_resample_device"):
        fn = getattr(L, name)
        for ns, nd, ncomp, mode in (((6, 5, 4), (3, 3, 4), 2, 1), ((6, 5, 4), (11, 5, 4), 2, 0), ((6, 5, 4), (7, 5, 4), 2, 1),
                                    ((6, 5, 4), (3, 3, 4), 0, 1), ((6, 5, 4), (3, 3, 4), 2, 5), ((6, 5, 1), (3, 3, 4), 2, 0),
                                    ((0, 0, 0), (-1, 2, 2), 2, 0)):
            s3, d3 = np.array(ns, dtype=np.intc), np.array(nd, dtype=np.intc)
            dst = np.full(4096, 3.25)
            assert fn(p(s3), p(d3), ncomp, mode, p(src), p(dst)) == 9001, (name, ns, nd, ncomp, mode)
            assert (dst == 3.25).all()
        assert fn(None, None, 1, 0, None, None) == 9001
    assert np.array_equal(src, keep)

    # ---- the cascade
    n = 8 ** 3
    b, w = np.linspace(-1.0, 1.0, 3 * n), np.linspace(0.5, 1.5, n)
    keep = [v.copy() for v in (b, w)]
    ioptc, ropt = np.zeros(16, dtype=np.intc), np.zeros(16)
    for hs in ((None, None), (vp(1), vp(2)), (vp(1), None)):   # NULL handles, and ones the library never made
        harray = (vp * 2)(*hs)
        for name in ("ndsm_hip_vecpot_optimize_cascade", "ndsm_hip_vecpot_optimize_cascade_device"):
            fn = getattr(L, name)
            #            start niter   check tol   dt0           dt_min       rows
            for args in ((0, (10, 20), 5, 1e-4, (1e-3, 4e-3), (1e-9, 4e-9), 4), (1, (10, 20), 5, 0.0, (1e-3, 4e-3), (0.0, 0.0), 2),
                         (2, (10, 20), 5, 1e-4, (1e-3, 4e-3), (1e-9, 4e-9), 4), (0, (10, 0), 5, 1e-4, (1e-3, 4e-3), (1e-9, 4e-9), 4),
                         (0, (10, 20), 0, 1e-4, (1e-3, 4e-3), (1e-9, 4e-9), 4), (0, (10, 20), 5, nan, (1e-3, 4e-3), (1e-9, 4e-9), 4),
                         (0, (10, 20), 5, 1e-4, (1e-3, 0.0), (1e-9, 4e-9), 4), (0, (10, 20), 5, 1e-4, (inf, 4e-3), (1e-9, 4e-9), 4),
                         (0, (10, 20), 5, 1e-4, (1e-3, 4e-3), (-1.0, 4e-9), 4), (0, (10, 20), 5, 1e-4, (1e-3, 4e-3), (1e-9, nan), 4),
                         (0, (10, 20), 5, 1e-4, (1e-3, 4e-3), (1e-9, 4e-9), 1)):
                start, nit, check, tol, d0, dm, rows = args
                nit_a, d0_a, dm_a = np.array(nit, dtype=np.intc), np.array(d0), np.array(dm)
                for wt in (w, None):
                    hist, info = np.full(2 * 4 * 6 + 5, nan), np.full((2, 3), 77, dtype=np.intc)
                    rc = fn(harray, 2, p(ioptc), p(ropt), p(b), p(wt), start, p(nit_a), check, tol, p(d0_a), p(dm_a),
                            p(hist), rows, p(info))
                    assert rc == 9001, (name, args)
                    # what lives on the host in both entries is cleared: the rows the call was given, and info
                    assert np.all(info == 0) and np.all(hist[:2 * rows * 6] == 0.0) and np.all(np.isnan(hist[2 * rows * 6:]))
            nit_a, d0_a, dm_a = np.array((10, 20), dtype=np.intc), np.array((1e-3, 4e-3)), np.array((1e-9, 4e-9))
            for rows, nl in ((0, 2), (-3, 2), (4, 0), (4, -1)):     # no rows or no levels to clear, and none touched
                hist, info = np.full((2, 4, 6), nan), np.full((2, 3), 77, dtype=np.intc)
                assert fn(harray, nl, p(ioptc), p(ropt), p(b), p(w), 0, p(nit_a), 5, 1e-4, p(d0_a), p(dm_a), p(hist), rows,
                          p(info)) == 9001
                assert np.all(np.isnan(hist)) and np.all(info == (0 if nl >= 1 else 77))
            assert fn(None, 2, p(ioptc), p(ropt), None, None, 0, None, 5, 1e-4, None, None, None, 4, None) == 9001
    for v, k in zip((b, w), keep):
        assert np.array_equal(v, k)
    assert not ioptc.any() and not ropt.any()
    # the Python layer raises instead
    x = np.linspace(0, 1, 9)
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.force_free_cascade(x, x, x, np.zeros((3, 9, 9, 9)), levels=2)
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.resample(np.zeros((9, 9, 9)), (5, 5, 5), mode="average")


def fake_handle(shape_xyz, box=((0.0, 1.0), (0.0, 1.0), (0.0, 1.0)), ngrids=0):
    import ndsm_amd

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library reached: " + name)
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.nshape4 = np.array(list(shape_xyz) + [3], dtype=np.intc)
    V.x, V.y, V.z = (np.linspace(lo, hi, n) for (lo, hi), n in zip(box, shape_xyz))
    V.ngrids = ngrids
    V.L, V.h = NoCalls(), None
    return V


def test_cascade_arguments_checked_before_any_device_call(lib):
    """arrays that do not fit are an argument error (9002) and bad options or levels a ValueError, before the library
    is called"""
    import ndsm_amd
    V, C1, C2 = fake_handle((9, 7, 5)), fake_handle((5, 4, 5)), fake_handle((4, 4, 4))
    z, w = np.zeros((3, 5, 7, 9)), np.ones((5, 7, 9))
    for bad in (np.zeros((3, 5, 7, 8)), np.zeros((5, 7, 9)), np.zeros((3, 5, 4, 5))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.optimize_cascade([C1], bad, w)
    for bad in (np.ones((9, 7, 5)), np.ones((3, 5, 7, 9)), np.ones((5, 4, 5))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.optimize_cascade([C1], z, bad)
    for kw in (dict(niter_max=0), dict(niter_max=2.5), dict(niter_max=[5, 0]), dict(niter_max=[5, 5, 5]), dict(niter_max=[5]),
               dict(check=0), dict(check=-1), dict(tol=-1e-3), dict(tol=float("nan")), dict(tol=float("inf")), dict(dt0=0.0),
               dict(dt0=[1e-3, -1.0]), dict(dt0=[1e-3]), dict(dt0=float("inf")), dict(dt0=[float("nan"), 1e-3]),
               dict(dt_min=-1.0), dict(dt_min=[0.0, float("nan")]), dict(dt_min=[0.0, 0.0, 0.0]), dict(hist_rows=1),
               dict(hist_rows=2.5), dict(start="zero"), dict(start=0), dict(start=None)):
        with pytest.raises(ValueError):
            V.optimize_cascade([C1], z, w, **kw)
    with pytest.raises(ValueError):
        C1.optimize_cascade([V], np.zeros((3, 5, 4, 5)))                     # a coarser level that is larger
    with pytest.raises(ValueError):
        V.optimize_cascade([C2, C1], z)                                      # ... further down the list
    with pytest.raises(ValueError):
        V.optimize_cascade([fake_handle((5, 4, 5), box=((0.0, 1.0), (0.0, np.nextafter(1.0, 2.0)), (0.0, 1.0)))], z)
    minus = fake_handle((5, 4, 5))
    minus.x[0] = -0.0                                                        # equal as a number: bit for bit it is not
    with pytest.raises(ValueError):
        V.optimize_cascade([minus], z)
    with pytest.raises(ValueError):
        V.optimize_cascade([None], z)
    for kw in (dict(mode="cubic"), dict(shape=(5, 7)), dict(shape=(5, 7, 10), mode="average"), dict(shape=(5, 1, 9))):
        with pytest.raises(ValueError):
            ndsm_amd.resample(w, **dict(dict(shape=(5, 7, 9), lib=V.L), **kw))
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.resample(np.ones((7, 9)), (7, 9, 1), lib=V.L)
