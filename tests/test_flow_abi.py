"""CPU tests of the flow entry points (include/ndsm_hip.h, "Flow inversion and boundary fluxes"): the eight symbols are
declared and exported, the header's prototypes are the ones the Python binding declares, the launchers behind them stay
internal, the header states the semantics' key phrases, without a GPU every entry fails cleanly - 9001 whatever the
arguments, never a crash, the outputs untouched -, the Python names are there with the documented defaults, and the
Python layer checks its options before it reaches the library."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_cascade_abi import ROOT, HEADER, ctypes_kinds

MESH = "ppp"                                   # nsrc, xs, ys
KINDS = {"ndsm_hip_flow_fit": MESH + "pp" + "did" + "ppp", "ndsm_hip_flow_fit_device": MESH + "pp" + "did" + "ppp",
         "ndsm_hip_green_ap_points": MESH + "pipp", "ndsm_hip_green_ap_points_device": MESH + "pipp",
         "ndsm_hip_green_ap_plane": MESH + "pp", "ndsm_hip_green_ap_plane_device": MESH + "pp",
         "ndsm_hip_flow_flux": MESH + "pppp" + "p", "ndsm_hip_flow_flux_device": MESH + "pppp" + "p"}


def header_kinds(name):
    """test_cascade_abi.header_kinds with int32_t pointers: 'p', 'i' or 'd' per parameter of the header's prototype"""
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


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_flow_entries_declared_exported_and_bound(lib):
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
    for name in ("ndsmk_flow_fit", "ndsmk_flow_flux", "ndsmk_flow_fits", "ndsmk_green_ap_points", "ndsmk_green_ap_plane"):
        assert name in kernels and name not in open(HEADER).read()
    iface = open(os.path.join(ROOT, "ndsm_amd", "fsrc", "ndsmh_iface.f90")).read()
    for name in ("ndsmk_flow_fit", "ndsmk_flow_flux", "ndsmk_flow_fits", "ndsmk_green_ap_points", "ndsmk_green_ap_plane"):
        assert 'name="%s"' % name in iface, name
    assert "flow" in open(os.path.join(ROOT, "ndsm_amd", "Makefile")).read().split("HIPSRC")[1].split("\n")[0].split()
    src = open(os.path.join(ROOT, "ndsm_amd", "csrc", "flow.hip")).read()
    assert "__launch_bounds__" in src and "flow_prep_k" in src and "flow_fit_k" in src
    assert "atomic" not in src.replace("No atomics", "") and not re.search(r"\basm\b", src)
    text = open(HEADER).read()
    for phrase in ("Flow inversion and boundary fluxes", "Schuck 2008", "Berger & Field 1984", "clipped, not padded",
                   "b ascending outer, a ascending inner", "d_k = 1.0 / sqrt(G_kk)", "Gs_kl = (G_kl d_k) d_l",
                   "-(D x') - Bx", "without pivoting", "the aperture problem", "punctured", "second order in h",
                   "(-dy) t and dx t", "h_sh = -2.0 ((Apx Vx + Apy Vy) Bz)", "s_em = (Bx Bx + By By) Vz",
                   "without 4 pi", "NB = min(nsy, 2048)", "same bits from both"):
        assert phrase in text, phrase


def test_flow_python_names(lib):
    import ndsm_amd
    for name in ("flow_fit", "plane_vector_potential", "plane_vector_potential_points", "boundary_fluxes", "Flow",
                 "Fluxes"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    ff = inspect.signature(ndsm_amd.flow_fit).parameters
    assert list(ff)[:8] == ["xs", "ys", "b0", "b1", "dt", "r", "rcond", "device"]
    assert [ff[k].default for k in ("r", "rcond", "device")] == [5, 1e-10, False]
    pv = inspect.signature(ndsm_amd.plane_vector_potential).parameters
    assert list(pv)[:4] == ["xs", "ys", "bz", "device"] and pv["device"].default is False
    pp = inspect.signature(ndsm_amd.plane_vector_potential_points).parameters
    assert list(pp)[:5] == ["xs", "ys", "bz", "pts", "device"] and pp["device"].default is False
    bf = inspect.signature(ndsm_amd.boundary_fluxes).parameters
    assert list(bf)[:7] == ["xs", "ys", "b", "v", "ap", "status", "device"]
    assert [bf[k].default for k in ("ap", "status", "device")] == [None, None, False]
    assert ndsm_amd.Flow._fields == ("v", "coef", "status")
    assert ndsm_amd.Fluxes._fields == ("dens", "helicity", "energy", "flux")


def test_flow_entries_fail_cleanly_without_a_gpu(lib):
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

    xs, ys = np.arange(5.0), np.arange(4.0)
    b0, b1, ap, bz, pts = np.linspace(-1, 1, 60), np.linspace(1, 2, 60), np.linspace(0, 1, 40), np.ones(20), np.ones(8)
    back = xs[::-1].copy()
    keep = [v.copy() for v in (xs, ys, b0, b1, ap, bz, pts)]
    for suffix in ("", "_device"):
        fn = getattr(L, "ndsm_hip_flow_fit" + suffix)
        for ns, sx, dt, r, rc in (((5, 4), xs, 1.0, 2, 0.0), ((2, 4), xs, 1.0, 2, 0.0), ((5, 4), back, 1.0, 2, 0.0),
                                  ((5, 4), xs, 0.0, 2, 0.0), ((5, 4), xs, float("nan"), 0, 2.0), ((5, 4), xs, 1.0, 17, -1.0),
                                  ((0, -3), xs, 1.0, 2, 0.0), ((2 ** 30, 2 ** 30), xs, 1.0, 2, 0.0)):
            V, C, S = np.full(60, 3.25), np.full(180, 3.25), np.full(20, 7, dtype=np.int32)
            got = fn(p(np.array(ns, dtype=np.intc)), p(sx), p(ys), p(b0), p(b1), dt, r, rc, p(V), p(C), p(S))
            assert got == 9001, (suffix, ns, dt, r, rc)
            assert (V == 3.25).all() and (C == 3.25).all() and (S == 7).all()
        assert fn(None, None, None, None, None, 1.0, 2, 0.0, None, None, None) == 9001
        fn = getattr(L, "ndsm_hip_green_ap_points" + suffix)
        for ns, npts in (((5, 4), 4), ((1, 4), 4), ((5, 4), -1), ((5, 4), 0), ((5, 4), 2 ** 31 - 1)):
            A = np.full(8, 3.25)
            assert fn(p(np.array(ns, dtype=np.intc)), p(xs), p(ys), p(bz), npts, p(pts), p(A)) == 9001, (suffix, ns, npts)
            assert (A == 3.25).all()
        assert fn(None, None, None, None, 4, None, None) == 9001
        fn = getattr(L, "ndsm_hip_green_ap_plane" + suffix)
        for ns in ((5, 4), (1, 4), (2 ** 30, 2 ** 30)):
            A = np.full(40, 3.25)
            assert fn(p(np.array(ns, dtype=np.intc)), p(xs), p(ys), p(bz), p(A)) == 9001, (suffix, ns)
            assert (A == 3.25).all()
        assert fn(None, None, None, None, None) == 9001
        fn = getattr(L, "ndsm_hip_flow_flux" + suffix)
        for ns in ((5, 4), (1, 4), (2 ** 30, 2 ** 30)):
            D, out = np.full(80, 3.25), np.full(8, 3.25)
            assert fn(p(np.array(ns, dtype=np.intc)), p(xs), p(ys), p(b0), p(b1), p(ap), p(D), p(out)) == 9001, (suffix, ns)
            assert (D == 3.25).all() and (out == 3.25).all()
        assert fn(None, None, None, None, None, None, None, None) == 9001
    for v, k in zip((xs, ys, b0, b1, ap, bz, pts), keep):
        assert np.array_equal(v, k)
    # the Python layer raises instead
    b = b0.reshape(3, 4, 5)
    with pytest.raises(ndsm_amd.NdsmHipError, match="9001"):
        ndsm_amd.flow_fit(xs, ys, b, b, 1.0)
    with pytest.raises(ndsm_amd.NdsmHipError, match="9001"):
        ndsm_amd.plane_vector_potential(xs, ys, bz.reshape(4, 5))
    with pytest.raises(ndsm_amd.NdsmHipError, match="9001"):
        ndsm_amd.plane_vector_potential_points(xs, ys, bz.reshape(4, 5), pts.reshape(4, 2))
    with pytest.raises(ndsm_amd.NdsmHipError, match="9001"):
        ndsm_amd.boundary_fluxes(xs, ys, b, b, ap=ap.reshape(2, 4, 5))
    with pytest.raises(ndsm_amd.NdsmHipError, match="9001"):
        ndsm_amd.boundary_fluxes(xs, ys, b, b)


class NoLibrary:
    """stands in for the library: any call is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("the library was reached: " + name)


def test_flow_options_checked_before_any_library_call():
    """what the library would answer with 9004, and arrays that do not fit their mesh, are a ValueError before the
    library is called"""
    import ndsm_amd
    L = NoLibrary()
    xs, ys = np.arange(5.0), np.arange(4.0)
    b, bz, ap, pts = np.zeros((3, 4, 5)), np.zeros((4, 5)), np.zeros((2, 4, 5)), np.zeros((6, 2))
    base = dict(xs=xs, ys=ys, b0=b, b1=b, dt=1.0, lib=L)
    for kw in (dict(dt=0.0), dict(dt=float("nan")), dict(dt=float("inf")), dict(r=0), dict(r=17), dict(r=2.5),
               dict(rcond=-1e-3), dict(rcond=1.0), dict(rcond=float("nan")), dict(xs=xs[:2]), dict(ys=ys[:2]),
               dict(xs=xs[::-1]), dict(ys=np.zeros(4)), dict(b0=b[:2]), dict(b1=np.zeros((3, 5, 4))), dict(b0=bz)):
        with pytest.raises(ValueError):
            ndsm_amd.flow_fit(**dict(base, **kw))
    for kw in (dict(xs=xs[:1]), dict(ys=ys[::-1]), dict(bz=bz.T), dict(bz=b)):
        with pytest.raises(ValueError):
            ndsm_amd.plane_vector_potential(**dict(dict(xs=xs, ys=ys, bz=bz, lib=L), **kw))
        with pytest.raises(ValueError):
            ndsm_amd.plane_vector_potential_points(**dict(dict(xs=xs, ys=ys, bz=bz, pts=pts, lib=L), **kw))
    for bad in (np.zeros((6, 3)), np.zeros(2), np.zeros((2, 6))):
        with pytest.raises(ValueError):
            ndsm_amd.plane_vector_potential_points(xs, ys, bz, bad, lib=L)
    for kw in (dict(xs=xs[:1]), dict(ys=ys[::-1]), dict(b=bz), dict(v=b[:2]), dict(ap=b), dict(ap=bz),
               dict(status=np.zeros((5, 4))), dict(status=np.zeros(20))):
        with pytest.raises(ValueError):
            ndsm_amd.boundary_fluxes(**dict(dict(xs=xs, ys=ys, b=b, v=b, ap=ap, lib=L), **kw))
