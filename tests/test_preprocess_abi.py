"""CPU tests of the magnetogram-preprocessing entry points (include/ndsm_hip.h): the two symbols are declared and
exported, the header's prototypes are the ones the Python binding declares, the Python names are there with the
documented defaults, and without a GPU both entries fail cleanly - 9001 whatever the arguments, never a crash, hist and
info cleared, inputs untouched."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndsm_hip.h")
ENTRIES = ["ndsm_hip_vecpot_preprocess", "ndsm_hip_vecpot_preprocess_device"]
KINDS = "pppp" + "ii" + "ddd" + "pip"
MU = (1, 1, 1e-3, 1e-2, 1e-2)


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


def test_preprocess_entries_declared_exported_and_bound(lib):
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
    for phrase in ("Magnetogram preprocessing", "Wiegelmann, Inhester & Sakurai", "mu3h", "hist_rows", "dt_min",
                   "stop reason", "Lambda", "torque", "17 doubles"):
        assert phrase in text, phrase
    kernels = open(os.path.join(ROOT, "ndsm_amd", "csrc", "ndsm_kernels.h")).read()
    for name in ("ndsmk_preprocess_work_bytes", "ndsmk_preprocess_begin", "ndsmk_preprocess_tries", "ndsmk_preprocess_row"):
        assert name in kernels, name
    assert "preprocess" in open(os.path.join(ROOT, "ndsm_amd", "Makefile")).read().split("HIPSRC")[1].split("\n")[0]


def test_preprocess_python_names(lib):
    import ndsm_amd
    for name in ("preprocess_magnetogram", "magnetogram_balance"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    par = inspect.signature(ndsm_amd.VecPot.preprocess).parameters
    names = ["bm", "obs", "mu", "niter_max", "check", "tol", "dt0", "dt_min", "hist_rows", "device"]
    assert list(par)[1:] == names
    assert [par[k].default for k in names[1:]] == [None, MU, 10000, 50, 1e-4, None, None, None, False]
    one = inspect.signature(ndsm_amd.preprocess_magnetogram).parameters
    assert list(one)[:4] == ["x", "y", "z", "bm"] and list(one)[4:12] == names[1:9]
    assert [one[k].default for k in names[1:9]] == [par[k].default for k in names[1:9]]
    assert list(inspect.signature(ndsm_amd.magnetogram_balance).parameters) == ["hist"]
    assert "not tuned on real data" in " ".join(ndsm_amd.VecPot.preprocess.__doc__.lower().split())
    assert "not tuned on real data" in " ".join(ndsm_amd.preprocess_magnetogram.__doc__.lower().split())


def test_preprocess_entries_fail_cleanly_without_a_gpu(lib):
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
    n = 8 * 7
    b, obs = np.linspace(-1.0, 1.0, 3 * n), np.linspace(0.5, 1.5, 3 * n)
    mu = np.array(MU, dtype=np.float64)
    keep = [v.copy() for v in (b, obs, mu)]
    nan, inf = float("nan"), float("inf")

    def p(v):
        return None if v is None else vp(v.ctypes.data)

    for h in (None, vp(1)):          # a NULL handle, and one the library never made: neither is looked at
        for name in ENTRIES:
            fn = getattr(L, name)
            #            niter check tol  dt0   dt_min rows
            for args in ((10, 5, 1e-4, 1e-2, 1e-8, 4), (10, 5, 0.0, 1e-2, 0.0, 2), (0, 5, 1e-4, 1e-2, 1e-8, 4),
                         (10, 0, 1e-4, 1e-2, 1e-8, 4), (10, 5, -1.0, 1e-2, 1e-8, 4), (10, 5, nan, 1e-2, 1e-8, 4),
                         (10, 5, 1e-4, 0.0, 1e-8, 4), (10, 5, 1e-4, inf, 1e-8, 4), (10, 5, 1e-4, 1e-2, -1.0, 4),
                         (10, 5, 1e-4, 1e-2, nan, 4), (10, 5, 1e-4, 1e-2, 1e-8, 1)):
                rows = args[5]
                for ob in (obs, None):
                    for m in (mu, np.array([1.0, -1.0, nan, inf, 0.0])):
                        hist, info = np.full((4, 17), nan), np.full(3, 77, dtype=np.intc)
                        rc = fn(h, p(b), p(ob), p(m), *args[:5], p(hist), rows, p(info))
                        assert rc == 9001, (name, args)
                        # what lives on the host in both entries is cleared: the rows the call was given, and info
                        assert np.all(info == 0) and np.all(hist[:rows] == 0.0) and np.all(np.isnan(hist[rows:]))
            for rows in (0, -3):     # no rows to clear, and none touched
                hist, info = np.full((4, 17), nan), np.full(3, 77, dtype=np.intc)
                assert fn(h, p(b), p(obs), p(mu), 10, 5, 1e-4, 1e-2, 1e-8, p(hist), rows, p(info)) == 9001
                assert np.all(info == 0) and np.all(np.isnan(hist))
            assert fn(h, None, None, None, 10, 5, 1e-4, 1e-2, 1e-8, None, 4, None) == 9001
    for v, k in zip((b, obs, mu), keep):
        assert np.array_equal(v, k)
    # the Python layer raises instead
    x = np.linspace(0, 1, 8)
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.preprocess_magnetogram(x, x, x, np.ones((3, 8, 8)))


def test_preprocess_arguments_checked_before_any_device_call(lib):
    """arrays that do not fit are an argument error (9002) and bad options a ValueError, before the library is
    called"""
    import ndsm_amd
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.nshape4 = np.array([8, 7, 6, 3], dtype=np.intc)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library reached: " + name)
    V.L, V.h = NoCalls(), None
    z = np.zeros((3, 7, 8))
    for bad in (np.zeros((3, 8, 7)), np.zeros((3, 6, 7, 8)), np.zeros((7, 8)), np.zeros(3 * 7 * 8)):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.preprocess(bad)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.preprocess(z, obs=bad)
    for kw in (dict(niter_max=0), dict(niter_max=2.5), dict(check=0), dict(check=-1), dict(tol=-1e-3),
               dict(tol=float("nan")), dict(tol=float("inf")), dict(dt0=0.0), dict(dt0=-1.0), dict(dt0=float("inf")),
               dict(dt0=float("nan")), dict(dt_min=-1.0), dict(dt_min=float("nan")), dict(hist_rows=1),
               dict(hist_rows=2.5), dict(mu=(1, 1, 1, 1)), dict(mu=(1, 1, -1e-3, 1, 1)),
               dict(mu=(1, 1, 1, float("nan"), 1)), dict(mu=(float("inf"), 1, 1, 1, 1))):
        with pytest.raises(ValueError):
            V.preprocess(z, **kw)
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.preprocess_magnetogram(np.zeros(8), np.zeros(7), np.zeros(6), np.zeros((3, 8, 7)))
