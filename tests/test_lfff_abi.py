"""CPU tests of the constant-alpha force-free entry points (include/ndsm_hip.h, "Linear force-free field"): the four
symbols are declared and exported, the header's prototypes are the ones the Python binding declares, the launchers
behind them stay internal, the Python names are there with the documented defaults, without a GPU every entry fails
cleanly - 9001 whatever the arguments, never a crash, the outputs untouched - and the Python layer checks its arguments
before it reaches the library."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_cascade_abi import ROOT, HEADER, header_kinds, ctypes_kinds, fake_handle

SRC = "ppp" + "d" + "p" + "d"                  # nsrc, xs, ys, zs, bz, alpha
KINDS = {"ndsm_hip_lfff_points": SRC + "ipp", "ndsm_hip_lfff_points_device": SRC + "ipp",
         "ndsm_hip_lfff_box": SRC + "pppp" + "ip", "ndsm_hip_lfff_box_device": SRC + "pppp" + "ip"}


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_lfff_entries_declared_exported_and_bound(lib):
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
    for name in ("ndsmk_lfff_points", "ndsmk_lfff_box"):
        assert name in kernels and name not in open(HEADER).read()
    hip = open(os.path.join(ROOT, "ndsm_amd", "csrc", "green.hip")).read()
    # one all-pairs kernel over three pair terms, and the fold: no other __global__ function
    assert re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", hip) == ["pairs_k", "fold_k"]
    assert "template <class Term>\n__global__" in hip
    assert sorted(re.findall(r"^struct (\w+Term) \{", hip, re.M)) == ["ApTerm", "GreenTerm", "LfffTerm"]
    assert all("pairs_k<%s>" % term in hip for term in ("ApTerm", "GreenTerm", "LfffTerm")) and "sincos(" in hip
    text = open(HEADER).read()
    for phrase in ("Linear force-free field", "Chiu & Hilton", "sz = sin(alpha w)", "u = alpha (q / R2)",
                   "e = sz - (ww / r2) sr", "f = (w / r) cr - cz", "A hazard", "not unique", "For finite bz only"):
        assert phrase in text, phrase


def test_lfff_python_names(lib):
    import ndsm_amd
    for name in ("lfff_field_points", "linear_force_free_field", "best_alpha"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    lp = inspect.signature(ndsm_amd.lfff_field_points).parameters
    assert list(lp)[:7] == ["xs", "ys", "zs", "bz", "alpha", "pts", "device"] and lp["device"].default is False
    assert all(lp[k].default is inspect.Parameter.empty for k in list(lp)[:6])
    lf = inspect.signature(ndsm_amd.linear_force_free_field).parameters
    assert list(lf)[:10] == ["x", "y", "z", "bz", "alpha", "xs", "ys", "zs", "which", "device"]
    assert [lf[k].default for k in ("xs", "ys", "zs", "which", "device")] == [None, None, None, "volume", False]
    assert lf["alpha"].default is inspect.Parameter.empty
    ba = inspect.signature(ndsm_amd.best_alpha).parameters
    assert list(ba) == ["x", "y", "b", "bz_min"] and ba["bz_min"].default == 0.0


def test_best_alpha_uses_the_differences_of_boundary_alpha(lib):
    import ndsm_amd
    rng = np.random.default_rng(0)
    x, y = np.cumsum(rng.uniform(0.5, 1.5, 9)), np.cumsum(rng.uniform(0.5, 1.5, 7))     # unequal spacings
    b = rng.uniform(-1.0, 1.0, (3, 2, 7, 9))
    b[2, 0, 3, 4] = 0.01
    for bz_min in (0.0, 0.2):
        a0 = ndsm_amd.boundary_alpha(x, y, b, bz_min)                   # Jz / Bz, 0 where |Bz| < bz_min
        use = np.abs(b[2, 0]) >= bz_min
        jz = a0 * b[2, 0]
        want = float(np.sum(jz[use] * b[2, 0][use])) / float(np.sum(b[2, 0][use] ** 2))
        got = ndsm_amd.best_alpha(x, y, b, bz_min)
        assert abs(got - want) <= 1e-13 * (1.0 + abs(want)), (bz_min, got, want)
    assert ndsm_amd.best_alpha(x, y, b) == ndsm_amd.best_alpha(x, y, b, 0.0)
    assert ndsm_amd.best_alpha(x, y, b, 0.0) != ndsm_amd.best_alpha(x, y, b, 0.2)


def test_lfff_entries_fail_cleanly_without_a_gpu(lib):
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
    nan, inf = float("nan"), float("inf")
    for suffix in ("", "_device"):
        fn = getattr(L, "ndsm_hip_lfff_points" + suffix)
        for ns, sx, npts, zs, al in (((5, 4), xs, 4, 0.0, 0.5), ((1, 4), xs, 4, 0.0, 0.5), ((5, 4), back, 4, 0.0, -2.0),
                                     ((5, 4), xs, -1, 0.0, 0.0), ((5, 4), xs, 0, 0.0, 1.0), ((0, -3), xs, 4, nan, 1.0),
                                     ((5, 4), xs, 2 ** 31 - 1, 0.0, 1.0), ((5, 4), xs, 4, 0.0, nan),
                                     ((5, 4), xs, 4, 0.0, inf), ((5, 4), xs, 4, 0.0, -inf)):
            B = np.full(12, 3.25)
            rc = fn(p(np.array(ns, dtype=np.intc)), p(sx), p(ys), zs, p(bz), al, npts, p(pts), p(B))
            assert rc == 9001, (suffix, ns, npts, al)
            assert (B == 3.25).all()
        assert fn(None, None, None, 0.0, None, 1.0, 4, None, None) == 9001
        fn = getattr(L, "ndsm_hip_lfff_box" + suffix)
        for ns, n3, which, zs, al in (((5, 4), (3, 3, 3), 0, 0.0, 0.5), ((5, 4), (3, 3, 3), 1, 0.0, -0.5),
                                      ((5, 4), (3, 3, 3), 2, 0.0, 0.5), ((5, 4), (3, 1, 3), 0, 0.0, 0.5),
                                      ((5, 4), (3, 3, 3), 0, 0.5, 0.5), ((1, 1), (0, 0, 0), -1, 0.0, 0.5),
                                      ((5, 4), (2 ** 30, 2 ** 30, 2 ** 30), 1, 0.0, 0.5), ((5, 4), (3, 3, 3), 1, 0.0, nan),
                                      ((5, 4), (3, 3, 3), 0, 0.0, inf)):
            B = np.full(81, 3.25)
            rc = fn(p(np.array(ns, dtype=np.intc)), p(xs), p(ys), zs, p(bz), al, p(np.array(n3, dtype=np.intc)), p(x), p(y),
                    p(z), which, p(B))
            assert rc == 9001, (suffix, ns, n3, which, al)
            assert (B == 3.25).all()
        assert fn(None, None, None, 0.0, None, 1.0, None, None, None, None, 0, None) == 9001
    for v, k in zip((xs, ys, bz, x, y, z, pts), keep):
        assert np.array_equal(v, k)
    # the Python layer raises instead
    with pytest.raises(ndsm_amd.NdsmHipError, match="9001"):
        ndsm_amd.lfff_field_points(xs, ys, 0.0, bz.reshape(4, 5), 0.5, pts.reshape(4, 3))
    with pytest.raises(ndsm_amd.NdsmHipError, match="9001"):
        ndsm_amd.linear_force_free_field(x, y, z, bz.reshape(4, 5), 0.5, xs=xs, ys=ys)


def test_lfff_arguments_checked_before_any_device_call(lib):
    """what the library would answer with 9004, and arrays that do not fit their mesh, are a ValueError before the
    library is called"""
    import ndsm_amd
    V = fake_handle((9, 7, 5))
    xs, ys, bz = np.arange(5.0), np.arange(4.0), np.zeros((4, 5))
    x, y, z = np.arange(3.0), np.arange(3.0), np.arange(3.0)
    pts = np.zeros((4, 3))
    bad_alpha = (dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=-float("inf")), dict(alpha=None),
                 dict(alpha=np.array([0.5, 0.5])), dict(alpha="x"))
    for kw in (dict(xs=xs[:1]), dict(ys=ys[:1]), dict(xs=xs[::-1]), dict(ys=np.zeros(4)), dict(bz=bz.T), dict(bz=bz[0]),
               dict(bz=np.zeros((4, 5, 1))), dict(xs=np.array([0.0, np.nan, 2, 3, 4])), dict(pts=np.zeros((4, 2))),
               dict(pts=np.zeros(3)), dict(pts=np.zeros((3, 4)))) + bad_alpha:
        with pytest.raises(ValueError):
            ndsm_amd.lfff_field_points(**dict(dict(xs=xs, ys=ys, zs=0.0, bz=bz, alpha=0.5, pts=pts, lib=V.L), **kw))
    for kw in (dict(which="sides"), dict(which=1), dict(xs=xs[:1]), dict(ys=ys[::-1]), dict(bz=bz.T), dict(zs=0.5),
               dict(x=x[:1]), dict(z=z[:1]), dict(xs=None), dict(ys=None)) + bad_alpha:
        with pytest.raises(ValueError):
            ndsm_amd.linear_force_free_field(**dict(dict(x=x, y=y, z=z, bz=bz, alpha=0.5, xs=xs, ys=ys, lib=V.L), **kw))
