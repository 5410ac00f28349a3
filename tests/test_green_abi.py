"""CPU tests of the Green's-function entry points (include/ndsm_hip.h, "Open-box potential field"): the six symbols are
declared and exported, the header's prototypes are the ones the Python binding declares, the launchers behind them stay
internal, the Python names are there with the documented defaults, without a GPU every entry fails cleanly - 9001
whatever the arguments, never a crash, the outputs untouched - and the Python layer checks its arguments before it
reaches the library."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_cascade_abi import ROOT, HEADER, header_kinds, ctypes_kinds, fake_handle

SRC = "ppp" + "d" + "p"                       # nsrc, xs, ys, zs, bz
KINDS = {"ndsm_hip_green_points": SRC + "ipp", "ndsm_hip_green_points_device": SRC + "ipp",
         "ndsm_hip_green_box": SRC + "pppp" + "ip", "ndsm_hip_green_box_device": SRC + "pppp" + "ip",
         "ndsm_hip_vecpot_open": "ppp" + SRC + "pp", "ndsm_hip_vecpot_open_device": "ppp" + SRC + "pp"}


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_green_entries_declared_exported_and_bound(lib):
    import ndsm_amd
    out = subprocess.check_output(["nm", "-D", "--defined-only", ndsm_amd.lib_path()], text=True)
    live = {l.split()[-1] for l in out.splitlines() if re.search(r" T ", l)}
    for name, kinds in KINDS.items():
        assert name in live, name
        assert hasattr(lib, name)
        assert header_kinds(name) == kinds, (name, header_kinds(name))
        assert ctypes_kinds(getattr(lib, name)) == kinds, name
    assert not any(s.startswith("ndsmk_") for s in live)
    kernels = open(os.path.join(ROOT, "ndsm_amd", "csrc", "ndsm_kernels.h")).read()
    for name in ("ndsmk_green_points", "ndsmk_green_box", "ndsmk_green_fits"):
        assert name in kernels and name not in open(HEADER).read()
    assert "green" in open(os.path.join(ROOT, "ndsm_amd", "Makefile")).read().split("HIPSRC")[1].split("\n")[0].split()
    assert "__launch_bounds__" in open(os.path.join(ROOT, "ndsm_amd", "csrc", "green.hip")).read()
    text = open(HEADER).read()
    for phrase in ("Open-box potential field", "6.283185307179586", "NS = min(64, ceil(npix / 4096))", "punctured",
                   "bilinear", "bit for bit"):
        assert phrase in text, phrase


def test_green_python_names(lib):
    import ndsm_amd
    for name in ("green_field_points", "magnetogram_field", "potential_open"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    gp = inspect.signature(ndsm_amd.green_field_points).parameters
    assert list(gp)[:6] == ["xs", "ys", "zs", "bz", "pts", "device"] and gp["device"].default is False
    mf = inspect.signature(ndsm_amd.magnetogram_field).parameters
    assert list(mf)[:9] == ["x", "y", "z", "bz", "xs", "ys", "zs", "which", "device"]
    assert [mf[k].default for k in ("xs", "ys", "zs", "which", "device")] == [None, None, None, "faces", False]
    so = inspect.signature(ndsm_amd.VecPot.solve_open).parameters
    assert list(so)[1:5] == ["bz", "xs", "ys", "zs"] and [so[k].default for k in ("xs", "ys", "zs")] == [None] * 3
    solve = inspect.signature(ndsm_amd.VecPot.solve).parameters
    assert list(so)[5:] == list(solve)[2:]                                    # solve's options, in solve's order
    assert [so[k].default for k in list(so)[5:]] == [solve[k].default for k in list(solve)[2:]]
    po = inspect.signature(ndsm_amd.potential_open).parameters
    assert list(po)[:7] == ["x", "y", "z", "bz", "xs", "ys", "zs"]


def test_green_entries_fail_cleanly_without_a_gpu(lib):
    if lib.ndsm_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    import ndsm_amd
    L = ctypes.CDLL(ndsm_amd.lib_path(), mode=os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, "RTLD_DEEPBIND", 0))
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    for name in KINDS:
        fn = getattr(L, name)
        fn.restype = ci
        fn.argtypes = [{"p": vp, "i": ci, "d": cd}[k] for k in header_kinds(name)]

    def p(v):
        return None if v is None else vp(v.ctypes.data)

    xs, ys, bz = np.arange(5.0), np.arange(4.0), np.linspace(-1.0, 1.0, 20)
    x, y, z = np.arange(3.0), np.arange(3.0), np.arange(3.0)
    pts = np.linspace(0.0, 2.0, 12)
    keep = [v.copy() for v in (xs, ys, bz, x, y, z, pts)]
    back = xs[::-1].copy()
    for suffix in ("", "_device"):
        fn = getattr(L, "ndsm_hip_green_points" + suffix)
        for ns, sx, npts, zs in (((5, 4), xs, 4, 0.0), ((1, 4), xs, 4, 0.0), ((5, 4), back, 4, 0.0), ((5, 4), xs, -1, 0.0),
                                 ((5, 4), xs, 0, 0.0), ((0, -3), xs, 4, float("nan")), ((5, 4), xs, 2 ** 31 - 1, 0.0)):
            B = np.full(12, 3.25)
            assert fn(p(np.array(ns, dtype=np.intc)), p(sx), p(ys), zs, p(bz), npts, p(pts), p(B)) == 9001, (suffix, ns, npts)
            assert (B == 3.25).all()
        assert fn(None, None, None, 0.0, None, 4, None, None) == 9001
        fn = getattr(L, "ndsm_hip_green_box" + suffix)
        for ns, n3, which, zs in (((5, 4), (3, 3, 3), 0, 0.0), ((5, 4), (3, 3, 3), 1, 0.0), ((5, 4), (3, 3, 3), 2, 0.0),
                                  ((5, 4), (3, 1, 3), 0, 0.0), ((5, 4), (3, 3, 3), 0, 0.5), ((1, 1), (0, 0, 0), -1, 0.0),
                                  ((5, 4), (2 ** 30, 2 ** 30, 2 ** 30), 1, 0.0)):
            B = np.full(81, 3.25)
            rc = fn(p(np.array(ns, dtype=np.intc)), p(xs), p(ys), zs, p(bz), p(np.array(n3, dtype=np.intc)), p(x), p(y), p(z),
                    which, p(B))
            assert rc == 9001, (suffix, ns, n3, which)
            assert (B == 3.25).all()
        assert fn(None, None, None, 0.0, None, None, None, None, None, 0, None) == 9001
        fn = getattr(L, "ndsm_hip_vecpot_open" + suffix)
        ioptc, ropt = np.zeros(16, dtype=np.intc), np.zeros(16)
        for h in (None, vp(1)):                                  # NULL, and a handle the library never made
            for ns in ((5, 4), (1, 1)):
                A, B = np.full(81, 1.5), np.full(81, 3.25)
                assert fn(h, p(ioptc), p(ropt), p(np.array(ns, dtype=np.intc)), p(xs), p(ys), 0.0, p(bz), p(A), p(B)) == 9001
                assert (A == 1.5).all() and (B == 3.25).all()
            assert fn(h, p(ioptc), p(ropt), None, None, None, 0.0, None, None, None) == 9001
        assert not ioptc.any() and not ropt.any()
    for v, k in zip((xs, ys, bz, x, y, z, pts), keep):
        assert np.array_equal(v, k)
    # the Python layer raises instead
    with pytest.raises(ndsm_amd.NdsmHipError, match="9001"):
        ndsm_amd.green_field_points(xs, ys, 0.0, bz.reshape(4, 5), pts.reshape(4, 3))
    with pytest.raises(ndsm_amd.NdsmHipError, match="9001"):
        ndsm_amd.magnetogram_field(x, y, z, bz.reshape(4, 5), xs=xs, ys=ys)
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.potential_open(x, y, z, bz.reshape(4, 5), xs=xs, ys=ys)


def test_green_arguments_checked_before_any_device_call(lib):
    """what the library would answer with 9004, and arrays that do not fit their mesh, are a ValueError before the
    library is called"""
    import ndsm_amd
    V = fake_handle((9, 7, 5))
    xs, ys, bz = np.arange(5.0), np.arange(4.0), np.zeros((4, 5))
    x, y, z = np.arange(3.0), np.arange(3.0), np.arange(3.0)
    pts = np.zeros((4, 3))
    for kw in (dict(xs=xs[:1]), dict(ys=ys[:1]), dict(xs=xs[::-1]), dict(ys=np.zeros(4)), dict(bz=bz.T), dict(bz=bz[0]),
               dict(bz=np.zeros((4, 5, 1))), dict(xs=np.array([0.0, np.nan, 2, 3, 4])), dict(pts=np.zeros((4, 2))),
               dict(pts=np.zeros(3)), dict(pts=np.zeros((3, 4)))):
        with pytest.raises(ValueError):
            ndsm_amd.green_field_points(**dict(dict(xs=xs, ys=ys, zs=0.0, bz=bz, pts=pts, lib=V.L), **kw))
    for kw in (dict(which="sides"), dict(which=0), dict(xs=xs[:1]), dict(ys=ys[::-1]), dict(bz=bz.T), dict(zs=0.5),
               dict(x=x[:1]), dict(z=z[:1]), dict(xs=None), dict(ys=None)):
        with pytest.raises(ValueError):
            ndsm_amd.magnetogram_field(**dict(dict(x=x, y=y, z=z, bz=bz, xs=xs, ys=ys, lib=V.L), **kw))
    for kw in (dict(xs=xs[:1]), dict(ys=ys[::-1]), dict(bz=bz.T), dict(zs=V.z[0] + 0.5), dict(bz=np.zeros((7, 8)))):
        with pytest.raises(ValueError):
            V.solve_open(**dict(dict(bz=bz, xs=xs, ys=ys), **kw))
        with pytest.raises(ValueError):
            ndsm_amd.potential_open(V.x, V.y, V.z, **dict(dict(bz=bz, xs=xs, ys=ys, lib=V.L), **kw))
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        V.solve_open(np.zeros((7, 9)), a_init=np.zeros((3, 5, 7, 8)))
