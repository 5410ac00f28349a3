"""CPU tests of the entry points of the weighted restriction and of the cascade of the measurement fit
(include/ndsm_hip.h): the four symbols are declared and exported, the header's prototypes are the ones the Python binding
declares, the launcher behind them stays internal, the Python names are there with the documented defaults, without a
GPU every entry fails cleanly - 9001 whatever the arguments, never a crash, hist and info cleared, B, dst and wdst
untouched - and the Python layer checks its arguments before it reaches the library."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_cascade_abi import ctypes_kinds, fake_handle, header_kinds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndsm_hip.h")
_OBC = "pi" + "pp" + "pppp" + "pi" + "ipid" + "ppp" + "ip"
KINDS = {"ndsm_hip_resample_weighted": "ppipppp", "ndsm_hip_resample_weighted_device": "ppipppp",
         "ndsm_hip_vecpot_optimize_obs_cascade": _OBC, "ndsm_hip_vecpot_optimize_obs_cascade_device": _OBC}


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_obs_cascade_entries_declared_exported_and_bound(lib):
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
    text = open(HEADER).read()
    assert "ndsmk_resample_weighted" in kernels and "ndsmk_resample_weighted" not in text
    hip = open(os.path.join(ROOT, "ndsm_amd", "csrc", "resample.hip")).read()
    assert "resample_weighted_k" in hip and hip.count("__launch_bounds__(256)") == 3
    for phrase in ("Cascade of the measurement fit", "Confidence-weighted restriction", "FINITE", "den > 0.0",
                   "NOT normalised axis by axis", "freed nodes keep the interpolated values"):
        assert phrase in text, phrase
    # the single-level entry no longer lists the cascade among what is missing
    assert "it needs Bobs and wm per level" not in text


def test_obs_cascade_python_names(lib):
    import ndsm_amd
    for name in ("resample_weighted", "force_free_obs_cascade"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    par = inspect.signature(ndsm_amd.VecPot.optimize_obs_cascade).parameters
    casc = inspect.signature(ndsm_amd.VecPot.optimize_cascade).parameters
    obs = inspect.signature(ndsm_amd.VecPot.optimize_obs).parameters
    assert list(par)[1:8] == ["coarser", "b", "bobs", "wm", "nu", "free", "w"]
    assert list(par)[8:] == list(casc)[4:]                           # start .. device, as optimize_cascade()
    assert [par[k].default for k in list(par)[8:]] == [casc[k].default for k in list(casc)[4:]]
    assert [par[k].default for k in ("bobs", "wm", "nu", "free", "w")] == [obs[k].default for k in ("bobs", "wm", "nu", "free", "w")]
    assert [par[k].default for k in ("bobs", "wm", "nu", "free", "w")] == [None, None, 0.01, True, None]
    one = inspect.signature(ndsm_amd.force_free_obs_cascade).parameters
    plain = inspect.signature(ndsm_amd.force_free_cascade).parameters
    assert list(one)[:6] == ["x", "y", "z", "b", "levels", "shapes"] and list(one)[6:11] == ["bobs", "wm", "nu", "free", "w"]
    assert list(one)[11:] == list(plain)[7:]
    assert one["levels"].default == 3 and one["shapes"].default is None
    assert [one[k].default for k in list(one)[6:]] == [par[k].default for k in list(one)[6:-1]] + [None]
    rs = inspect.signature(ndsm_amd.resample_weighted).parameters
    assert list(rs) == ["a", "wa", "shape", "device", "lib"]
    assert (rs["device"].default, rs["lib"].default) == (False, None)


def test_obs_cascade_entries_fail_cleanly_without_a_gpu(lib):
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

    # ---- the weighted restriction: good and bad arguments alike
    src, wsrc = np.linspace(-1.0, 1.0, 2 * 6 * 5 * 4), np.linspace(0.0, 1.0, 2 * 6 * 5 * 4)
    keep = [src.copy(), wsrc.copy()]
    for name in ("ndsm_hip_resample_weighted", "ndsm_hip_resample_weighted_device"):
        fn = getattr(L, name)
        for ns, nd, ncomp in (((6, 5, 4), (3, 3, 4), 2), ((6, 5, 4), (6, 5, 4), 2), ((6, 5, 4), (7, 5, 4), 2), ((6, 5, 4), (3, 3, 4), 0),
                              ((6, 5, 1), (3, 3, 4), 2), ((6, 5, 4), (3, 1, 4), 2), ((0, 0, 0), (-1, 2, 2), 2)):
            s3, d3 = np.array(ns, dtype=np.intc), np.array(nd, dtype=np.intc)
            dst, wdst = np.full(4096, 3.25), np.full(4096, -1.5)
            assert fn(p(s3), p(d3), ncomp, p(src), p(wsrc), p(dst), p(wdst)) == 9001, (name, ns, nd, ncomp)
            assert (dst == 3.25).all() and (wdst == -1.5).all()
        assert fn(None, None, 1, None, None, None, None) == 9001
    assert np.array_equal(src, keep[0]) and np.array_equal(wsrc, keep[1])

    # ---- the cascade
    n = 8 ** 3
    b, w = np.linspace(-1.0, 1.0, 3 * n), np.linspace(0.5, 1.5, n)
    bobs, wm = np.linspace(-2.0, 2.0, 3 * 64), np.linspace(0.1, 1.0, 3 * 64)
    keep = [v.copy() for v in (b, w, bobs, wm)]
    ioptc, ropt = np.zeros(16, dtype=np.intc), np.zeros(16)
    good = dict(nu=(0.01, 0.1), free=1, start=0, nit=(10, 20), check=5, tol=1e-4, d0=(1e-3, 4e-3), dm=(1e-9, 4e-9), rows=4)
    for hs in ((None, None), (vp(1), vp(2)), (vp(1), None)):   # NULL handles, and ones the library never made
        harray = (vp * 2)(*hs)
        for name in ("ndsm_hip_vecpot_optimize_obs_cascade", "ndsm_hip_vecpot_optimize_obs_cascade_device"):
            fn = getattr(L, name)
            for kw in (dict(), dict(free=0, start=1, tol=0.0, dm=(0.0, 0.0), rows=2), dict(free=2), dict(free=-1),
                       dict(nu=(-0.01, 0.1)), dict(nu=(0.01, nan)), dict(nu=(inf, 0.1)), dict(start=2), dict(nit=(10, 0)),
                       dict(check=0), dict(tol=nan), dict(d0=(1e-3, 0.0)), dict(dm=(1e-9, nan)), dict(rows=1)):
                a = dict(good, **kw)
                nu_a, nit_a = np.array(a["nu"]), np.array(a["nit"], dtype=np.intc)
                d0_a, dm_a = np.array(a["d0"]), np.array(a["dm"])
                for wt, wmt in ((w, wm), (None, None)):
                    hist, info = np.full(2 * 4 * 7 + 5, nan), np.full((2, 3), 77, dtype=np.intc)
                    rc = fn(harray, 2, p(ioptc), p(ropt), p(b), p(wt), p(bobs), p(wmt), p(nu_a), a["free"], a["start"],
                            p(nit_a), a["check"], a["tol"], p(d0_a), p(dm_a), p(hist), a["rows"], p(info))
                    assert rc == 9001, (name, kw)
                    # what lives on the host in both entries is cleared: the rows the call was given, and info
                    rows = a["rows"]
                    assert np.all(info == 0) and np.all(hist[:2 * rows * 7] == 0.0) and np.all(np.isnan(hist[2 * rows * 7:]))
            nu_a, nit_a = np.array(good["nu"]), np.array(good["nit"], dtype=np.intc)
            d0_a, dm_a = np.array(good["d0"]), np.array(good["dm"])
            for rows, nl in ((0, 2), (-3, 2), (4, 0), (4, -1)):     # no rows or no levels to clear, and none touched
                hist, info = np.full((2, 4, 7), nan), np.full((2, 3), 77, dtype=np.intc)
                assert fn(harray, nl, p(ioptc), p(ropt), p(b), p(w), p(bobs), p(wm), p(nu_a), 1, 0, p(nit_a), 5, 1e-4,
                          p(d0_a), p(dm_a), p(hist), rows, p(info)) == 9001
                assert np.all(np.isnan(hist)) and np.all(info == (0 if nl >= 1 else 77))
            assert fn(None, 2, p(ioptc), p(ropt), None, None, None, None, None, 1, 0, None, 5, 1e-4, None, None, None, 4,
                      None) == 9001
    for v, k in zip((b, w, bobs, wm), keep):
        assert np.array_equal(v, k)
    assert not ioptc.any() and not ropt.any()
    # the Python layer raises instead
    x = np.linspace(0, 1, 9)
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.force_free_obs_cascade(x, x, x, np.zeros((3, 9, 9, 9)), levels=2)
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.resample_weighted(np.zeros((9, 9, 9)), np.ones((9, 9, 9)), (5, 5, 5))


def test_obs_cascade_arguments_checked_before_any_device_call(lib):
    """arrays that do not fit are an argument error (9002) and bad options or levels a ValueError, before the library
    is called"""
    import ndsm_amd
    V, C1, C2 = fake_handle((9, 7, 5)), fake_handle((5, 4, 5)), fake_handle((4, 4, 4))
    z, w, pl = np.zeros((3, 5, 7, 9)), np.ones((5, 7, 9)), np.ones((3, 7, 9))
    for bad in (np.zeros((3, 5, 7, 8)), np.zeros((5, 7, 9)), np.zeros((3, 5, 4, 5))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.optimize_obs_cascade([C1], bad, w=w)
    for bad in (np.ones((9, 7, 5)), np.ones((3, 5, 7, 9)), np.ones((5, 4, 5))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.optimize_obs_cascade([C1], z, w=bad)
    for bad in (np.ones((3, 9, 7)), np.ones((7, 9)), np.ones((3, 4, 5)), np.ones((3, 1, 7, 9))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.optimize_obs_cascade([C1], z, bobs=bad)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.optimize_obs_cascade([C1], z, bobs=pl, wm=bad)
    for kw in (dict(nu=-0.1), dict(nu=float("nan")), dict(nu=float("inf")), dict(nu=[0.01, -1.0]), dict(nu=[0.01]),
               dict(nu=[0.01, 0.1, 0.1]), dict(nu=[0.01, float("nan")]), dict(free=2), dict(free="yes"), dict(free=None),
               dict(niter_max=0), dict(niter_max=[5, 0]), dict(niter_max=[5, 5, 5]), dict(check=0), dict(tol=-1e-3),
               dict(tol=float("nan")), dict(dt0=0.0), dict(dt0=[1e-3]), dict(dt_min=-1.0), dict(dt_min=[0.0, 0.0, 0.0]),
               dict(hist_rows=1), dict(start="zero"), dict(start=0)):
        with pytest.raises(ValueError):
            V.optimize_obs_cascade([C1], z, bobs=pl, wm=pl, **dict(dict(w=w), **kw))
    with pytest.raises(ValueError):
        C1.optimize_obs_cascade([V], np.zeros((3, 5, 4, 5)))                 # a coarser level that is larger
    with pytest.raises(ValueError):
        V.optimize_obs_cascade([C2, C1], z)                                  # ... further down the list
    with pytest.raises(ValueError):
        V.optimize_obs_cascade([fake_handle((5, 4, 5), box=((0.0, 1.0), (0.0, np.nextafter(1.0, 2.0)), (0.0, 1.0)))], z)
    with pytest.raises(ValueError):
        V.optimize_obs_cascade([None], z)
    for kw in (dict(shape=(5, 7)), dict(shape=(5, 7, 10)), dict(shape=(5, 1, 9)), dict(shape=(6, 7, 9))):
        with pytest.raises(ValueError):
            ndsm_amd.resample_weighted(w, w, **dict(dict(shape=(5, 7, 9), lib=V.L), **kw))
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.resample_weighted(np.ones((7, 9)), np.ones((7, 9)), (7, 9, 1), lib=V.L)
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.resample_weighted(w, np.ones((5, 7, 8)), (5, 7, 9), lib=V.L)
