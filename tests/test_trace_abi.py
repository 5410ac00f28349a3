"""CPU tests of the field-line tracing entry points (include/ndsm_hip.h, part 2): they are declared, exported,
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
ENTRIES = ["ndsm_hip_vecpot_trace", "ndsm_hip_vecpot_trace_device"]
STATUS = {"XLO": 1, "XHI": 2, "YLO": 3, "YHI": 4, "ZLO": 5, "ZHI": 6, "NULL": 7, "UNFINISHED": 8, "OUTSIDE": 9}


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_trace_entries_declared_and_exported(lib):
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
    assert not any(s.startswith("ndsmk_trace") for s in live)
    # ten named status codes, all distinct, the same in the header, the kernel layer and Python
    from ndsm_amd import _lib
    kern = open(os.path.join(ROOT, "ndsm_amd", "csrc", "ndsm_kernels.h")).read()
    for key, val in STATUS.items():
        assert re.search(r"#define\s+NDSM_HIP_TRACE_%s\s+%d\b" % (key, val), src), key
        assert re.search(r"\bNDSMK_TRACE_%s\s*=\s*%d\b" % (key, val), kern), key
        assert getattr(_lib, "TRACE_" + key) == val
    assert len(set(STATUS.values())) == 9
    # the header states the semantics
    for phrase in ("clamp(floor(", "RK4", "REDONE", "max_steps", "NDSM_HIP_TRACE_OUTSIDE", "kappa"):
        assert phrase in text, phrase


def test_trace_entries_fail_cleanly_without_a_gpu(lib):
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
        getattr(lib, name).argtypes = [vp, vp, vp, ctypes.c_int, vp, ctypes.c_double, ctypes.c_int, ctypes.c_int] + [vp] * 5

    def outputs():
        return [np.full(2 * 3 * ns, np.nan), np.full(2 * ns, np.nan), np.full(2 * ns, np.nan),
                np.full(2 * ns, 7, dtype=np.int32), np.full(2 * ns, 7, dtype=np.int32)]

    for h in (None, vp(1)):          # a NULL handle, and one the library never made: neither is looked at
        for direction, nl in ((0, 2 * ns), (1, ns), (-1, ns)):
            out = outputs()
            rc = lib.ndsm_hip_vecpot_trace(h, vp(b.ctypes.data), vp(g.ctypes.data), ns, vp(seeds.ctypes.data), 0.5, 100,
                                           direction, *[vp(a.ctypes.data) for a in out])
            assert rc == 9001
            for a in out:                # the nl lines' slots are cleared, what lies behind them is not touched
                m = nl * (3 if a.size == 6 * ns else 1)
                assert np.all(a[:m] == 0), direction
                assert np.all((a[m:] == 7) | np.isnan(a[m:])), direction
        # bad scalars and NULL arrays: still 9001, and no crash
        for args in ((ns, 0.0, 100, 0), (ns, 0.5, 0, 0), (ns, 0.5, 100, 3), (-1, 0.5, 100, 0), (0, 0.5, 100, 0)):
            out = outputs()
            rc = lib.ndsm_hip_vecpot_trace(h, vp(b.ctypes.data), None, args[0], vp(seeds.ctypes.data), args[1], args[2],
                                           args[3], *[vp(a.ctypes.data) for a in out])
            assert rc == 9001, args
        assert lib.ndsm_hip_vecpot_trace(h, None, None, ns, None, 0.5, 100, 0, None, None, None, None, None) == 9001
        # the device entry never reads or writes through its array arguments on the host
        out = outputs()
        rc = lib.ndsm_hip_vecpot_trace_device(h, vp(b.ctypes.data), vp(g.ctypes.data), ns, vp(seeds.ctypes.data), 0.5,
                                              100, 0, *[vp(a.ctypes.data) for a in out])
        assert rc == 9001
        assert np.all(np.isnan(out[0])) and np.all(out[3] == 7)
        assert lib.ndsm_hip_vecpot_trace_device(h, None, None, ns, None, 0.5, 100, 0, None, None, None, None,
                                                None) == 9001
    assert np.array_equal(b, b0) and np.array_equal(g, g0) and np.array_equal(seeds, s0)
    # the Python layer raises instead
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    sd = np.full((4, 3), 0.5)
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.trace_field_lines(x, x, x, z, sd)
    for gauge in ("devore", "coulomb"):
        with pytest.raises(ndsm_amd.NdsmHipError):
            ndsm_amd.field_line_helicity(x, x, x, z, sd, gauge=gauge)


def test_trace_python_names(lib):
    import ndsm_amd
    for name in ("FieldLines", "trace_field_lines", "field_line_helicity"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    assert ndsm_amd.FieldLines._fields == ("ends", "length", "integral", "status", "nsteps", "flh")
    par = inspect.signature(ndsm_amd.VecPot.trace).parameters
    assert list(par)[1:] == ["b", "seeds", "g", "step", "max_steps", "direction", "device"]
    assert (par["g"].default, par["step"].default, par["max_steps"].default, par["direction"].default,
            par["device"].default) == (None, 0.5, None, "both", False)
    par = inspect.signature(ndsm_amd.trace_field_lines).parameters
    assert list(par)[:5] == ["x", "y", "z", "b", "seeds"]
    assert (par["g"].default, par["step"].default, par["max_steps"].default, par["direction"].default) == \
        (None, 0.5, None, "both")
    for fn, first in ((ndsm_amd.field_line_helicity, ["x", "y", "z", "b", "seeds", "gauge", "a"]),
                      (ndsm_amd.VecPot.field_line_helicity, ["self", "b", "seeds", "gauge", "a"])):
        par = inspect.signature(fn).parameters
        assert list(par)[:len(first)] == first
        assert (par["gauge"].default, par["a"].default, par["step"].default, par["max_steps"].default,
                par["direction"].default, par["vc_tol"].default) == ("devore", None, 0.5, None, "both", 1e-10)
    # the default max_steps scales with the box: ceil(4 (nx + ny + nz) / step)
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.nshape4 = np.array([10, 12, 14, 3], dtype=np.intc)
    assert V.default_max_steps() == 288 and V.default_max_steps(0.37) == int(np.ceil(4 * 36 / 0.37))
    # existing signatures keep their defaults
    par = inspect.signature(ndsm_amd.VecPot.helicity).parameters
    assert par["gauge"].default == "coulomb" and par["project"].default is False
    assert ndsm_amd.Helicity._fields[:3] == ("ierr", "H_R", "H_J")


def test_trace_arguments_checked_before_any_device_call(lib):
    """bad options are a ValueError and arrays that do not fit an argument error (9002), before the library is
    called"""
    import ndsm_amd
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    sd = np.full((4, 3), 0.5)
    with pytest.raises(ValueError):
        ndsm_amd.field_line_helicity(x, x, x, z, sd, gauge="both")
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.trace_field_lines(x, x, x[:7], z, sd)
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.field_line_helicity(x, x, x[:7], z, sd)
    # VecPot itself: a handle object whose library would fail the test if it were reached
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.nshape4 = np.array([8, 8, 8, 3], dtype=np.intc)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library reached: " + name)
    V.L, V.h = NoCalls(), None
    for kw in (dict(step=0.0), dict(step=-0.5), dict(step=float("nan")), dict(step=float("inf")), dict(max_steps=0),
               dict(max_steps=-3), dict(max_steps=2.5), dict(direction="up"), dict(direction=1), dict(direction=None)):
        with pytest.raises(ValueError):
            V.trace(z, sd, **kw)
        with pytest.raises(ValueError):
            V.field_line_helicity(z, sd, **kw)
    for gauge in ("both", "Devore", None):
        with pytest.raises(ValueError):
            V.field_line_helicity(z, sd, gauge=gauge)
    for bad in (np.zeros((3, 8, 8, 7)), np.zeros((2, 8, 8, 8)), np.zeros((8, 8, 8, 3))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.trace(bad, sd)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.trace(z, sd, g=bad)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.field_line_helicity(bad, sd)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.field_line_helicity(z, sd, a=bad)
    for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((3, 4, 3))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.trace(z, bad)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.field_line_helicity(z, bad)
    # no seeds: empty results, and still no call
    fl = V.trace(z, np.zeros((0, 3)))
    assert fl.ends.shape == (2, 0, 3) and fl.status.dtype == np.int32 and fl.flh.shape == (0,)
    assert V.trace(z, np.zeros((0, 3)), direction="forward").flh is None
