"""CPU tests of the nonlinear force-free entry points (include/ndsm_hip.h, part 2): the six symbols are declared and
exported, the header's prototypes are the ones the Python binding declares, the Python names are there with the
documented defaults, and without a GPU every entry fails cleanly - 9001 whatever the arguments, never a crash, the
host-side outputs cleared, inputs untouched."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndsm_hip.h")
ENTRIES = ["ndsm_hip_vecpot_alpha_map", "ndsm_hip_vecpot_alpha_map_device", "ndsm_hip_vecpot_solve_current",
           "ndsm_hip_vecpot_solve_current_device", "ndsm_hip_vecpot_nlfff", "ndsm_hip_vecpot_nlfff_device"]


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


def test_nlfff_entries_declared_exported_and_bound(lib):
    import ndsm_amd
    out = subprocess.check_output(["nm", "-D", "--defined-only", ndsm_amd.lib_path()], text=True)
    live = {l.split()[-1] for l in out.splitlines() if re.search(r" T ", l)}
    want = {"alpha_map": "ppp" + "idi" + "pp", "solve_current": "ppp" + "ppp",
            "nlfff": "ppp" + "pp" + "iii" + "dd" + "i" + "ppp" + "pp"}
    for name in ENTRIES:
        assert name in live, name
        assert hasattr(lib, name)
        kinds = header_kinds(name)
        assert kinds == want[name[len("ndsm_hip_vecpot_"):].replace("_device", "")], (name, kinds)
        assert ctypes_kinds(getattr(lib, name)) == kinds, name
    # the kernels behind them stay internal
    assert not any(s.startswith("ndsmk_") for s in live)
    text = open(HEADER).read()
    for phrase in ("Grad-Rubin", "polarity", "bilinear", "hist", "niter_out", "NDSM_HIP_TRACE_ZLO", "start"):
        assert phrase in text, phrase
    # the kernel layer and the Fortran interface know the map
    assert "ndsmk_alpha_map" in open(os.path.join(ROOT, "ndsm_amd", "csrc", "ndsm_kernels.h")).read()
    assert "alphamap" in open(os.path.join(ROOT, "ndsm_amd", "Makefile")).read()


def test_nlfff_python_names(lib):
    import ndsm_amd
    for name in ("boundary_alpha", "map_alpha", "vector_potential_current", "force_free_field"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    par = inspect.signature(ndsm_amd.VecPot.alpha_map).parameters
    assert list(par)[1:] == ["b", "alpha0", "polarity", "step", "max_steps", "device"]
    assert [par[k].default for k in ("polarity", "step", "max_steps", "device")] == [1, 0.5, None, False]
    par = inspect.signature(ndsm_amd.VecPot.solve_current).parameters
    assert list(par)[1:4] == ["b", "j", "a_init"] and par["vc_tol"].default == 1e-10 and par["device"].default is False
    par = inspect.signature(ndsm_amd.VecPot.force_free).parameters
    assert list(par)[1:10] == ["b", "alpha0", "polarity", "start", "a_init", "niter_max", "tol", "step", "max_steps"]
    assert [par[k].default for k in ("polarity", "start", "a_init", "niter_max", "tol", "step", "max_steps", "device")] \
        == [1, "potential", None, 20, 0.0, 0.5, None, False]
    assert list(inspect.signature(ndsm_amd.force_free_field).parameters)[:5] == ["x", "y", "z", "b", "alpha0"]
    assert list(inspect.signature(ndsm_amd.map_alpha).parameters)[:5] == ["x", "y", "z", "b", "alpha0"]
    assert list(inspect.signature(ndsm_amd.vector_potential_current).parameters)[:5] == ["x", "y", "z", "b", "j"]


def test_boundary_alpha_is_plain_numpy():
    """alpha0 = (d_x B_y - d_y B_x) / B_z on k = 0 with np.gradient(edge_order=2), 0 where |B_z| < bz_min: exact for
    a field quadratic in x and y, on unequal spacings too"""
    import ndsm_amd
    x, y = np.linspace(0.2, 1.3, 9), np.linspace(-0.4, 0.5, 7)
    Y, X = np.meshgrid(y, x, indexing="ij")
    b = np.zeros((3, 4, 7, 9))
    b[0, 0] = 0.5 * Y * Y - X
    b[1, 0] = X * X + 0.25 * Y
    b[2, 0] = np.where(X > 0.6, 2.0, 1e-4)
    b[:, 1:] = np.nan                                   # only the lower face is looked at
    got = ndsm_amd.boundary_alpha(x, y, b, 1e-3)
    want = np.where(X > 0.6, (2.0 * X - Y) / 2.0, 0.0)
    assert got.shape == (7, 9)
    assert np.abs(got - want).max() <= 1e-13
    assert np.all(got[X <= 0.6] == 0.0)


def test_nlfff_entries_fail_cleanly_without_a_gpu(lib):
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
    b, a, j = np.linspace(-1.0, 1.0, 3 * n), np.linspace(2.0, 3.0, 3 * n), np.linspace(0.0, 1.0, 3 * n)
    a0 = np.linspace(0.5, 1.5, 64)
    keep = [v.copy() for v in (b, a, j, a0)]
    ioptc, ropt = np.zeros(16, dtype=np.intc), np.zeros(16)

    def p(v):
        return None if v is None else vp(v.ctypes.data)

    for h in (None, vp(1)):          # a NULL handle, and one the library never made: neither is looked at
        for dev in ("", "_device"):
            alpha, status = np.full(n, np.nan), np.full(n, 7, dtype=np.int32)
            fn = getattr(L, "ndsm_hip_vecpot_alpha_map" + dev)
            for pol, step, ms in ((1, 0.5, 100), (0, 0.5, 100), (1, 0.0, 100), (1, float("nan"), 100), (-1, 0.5, 0)):
                assert fn(h, p(b), p(a0), pol, step, ms, p(alpha), p(status)) == 9001
            assert fn(h, None, None, 1, 0.5, 100, None, None) == 9001
            # (nothing sizes the outputs without a live handle: they are left alone)
            assert np.all(np.isnan(alpha)) and np.all(status == 7)
            fn = getattr(L, "ndsm_hip_vecpot_solve_current" + dev)
            assert fn(h, p(ioptc), p(ropt), p(j), p(a), p(b)) == 9001
            assert fn(h, p(ioptc), p(ropt), None, None, None) == 9001
            fn = getattr(L, "ndsm_hip_vecpot_nlfff" + dev)
            for pol, start, nit, tol, step, ms in ((1, 0, 3, 0.0, 0.5, 100), (2, 0, 3, 0.0, 0.5, 100),
                                                    (1, 5, 3, 0.0, 0.5, 100), (1, 0, 3, -1.0, 0.5, 100),
                                                    (1, 0, 3, float("inf"), 0.5, 100), (1, 0, 3, 0.0, -0.5, 100),
                                                    (1, 1, 3, 0.0, 0.5, -2)):
                alpha, status = np.full(n, np.nan), np.full(n, 7, dtype=np.int32)
                hist, niter = np.full((3, 4), np.nan), ci(77)
                rc = fn(h, p(ioptc), p(ropt), p(b), p(a0), pol, start, nit, tol, step, ms, p(a), p(alpha), p(status),
                        p(hist), ctypes.byref(niter))
                assert rc == 9001, (pol, start, nit, tol, step, ms)
                # what lives on the host in both entries is cleared
                assert niter.value == 0 and np.all(hist == 0.0)
                assert np.all(np.isnan(alpha)) and np.all(status == 7)
            for nit in (0, -4):      # no rows to clear, and none touched
                hist, niter = np.full((3, 4), np.nan), ci(77)
                rc = fn(h, p(ioptc), p(ropt), p(b), p(a0), 1, 0, nit, 0.0, 0.5, 100, p(a), p(alpha), p(status), p(hist),
                        ctypes.byref(niter))
                assert rc == 9001 and niter.value == 0 and np.all(np.isnan(hist))
            assert fn(h, p(ioptc), p(ropt), None, None, 1, 0, 3, 0.0, 0.5, 100, None, None, None, None, None) == 9001
    for v, w in zip((b, a, j, a0), keep):
        assert np.array_equal(v, w)
    # the Python layer raises instead
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.map_alpha(x, x, x, z, np.zeros((8, 8)))
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.vector_potential_current(x, x, x, z, z)
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.force_free_field(x, x, x, z, np.zeros((8, 8)))


def test_nlfff_arguments_checked_before_any_device_call(lib):
    """arrays that do not fit are an argument error (9002) and bad options a ValueError, before the library is
    called"""
    import ndsm_amd
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.nshape4 = np.array([8, 7, 6, 3], dtype=np.intc)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library reached: " + name)
    V.L, V.h = NoCalls(), None
    z, a0 = np.zeros((3, 6, 7, 8)), np.zeros((7, 8))
    for bad in (np.zeros((3, 6, 7, 7)), np.zeros((6, 7, 8))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.alpha_map(bad, a0)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.force_free(bad, a0)
    for bad in (np.zeros((8, 7)), np.zeros(56), np.zeros((6, 7, 8))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.alpha_map(z, bad)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.force_free(z, bad)
    for kw in (dict(step=0.0), dict(step=float("nan")), dict(max_steps=0), dict(max_steps=2.5)):
        with pytest.raises(ValueError):
            V.alpha_map(z, a0, **kw)
        with pytest.raises(ValueError):
            V.force_free(z, a0, **kw)
    for start in ("zero", 0, None):
        with pytest.raises(ValueError):
            V.force_free(z, a0, start=start)
