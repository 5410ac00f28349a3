"""CPU tests of the DeVore-gauge entry points (include/ndsm_hip.h, part 2): they are declared, exported, reachable
from Python with the documented defaults, and fail cleanly - an error code, never a crash, B and B_p untouched -
without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndsm_hip.h")
ENTRIES = ["ndsm_hip_vecpot_devore", "ndsm_hip_vecpot_devore_device"]


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_devore_entries_declared_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    import ndsm_amd
    out = subprocess.check_output(["nm", "-D", "--defined-only", ndsm_amd.lib_path()], text=True)
    live = {l.split()[-1] for l in out.splitlines() if re.search(r" T ", l)}
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in live, name
        assert hasattr(lib, name)
    # the kernels behind them stay internal
    assert not any(s.startswith("ndsmk_devore") for s in live)


def test_devore_entries_fail_cleanly_without_a_gpu(lib):
    if lib.ndsm_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    import ndsm_amd
    # a CDLL object of its own (the same loaded library): prototypes set here stay private to this test
    lib = ctypes.CDLL(ndsm_amd.lib_path(), mode=os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, "RTLD_DEEPBIND", 0))
    vp = ctypes.c_void_p
    b = np.linspace(-1.0, 1.0, 3 * 8 ** 3)
    bp = np.linspace(2.0, 3.0, 3 * 8 ** 3)
    b0, bp0 = b.copy(), bp.copy()
    a = np.full(3 * 8 ** 3, 7.0)
    ap = np.full(3 * 8 ** 3, 5.0)
    for name in ENTRIES:
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [vp] * 6
    for h in (None, vp(1)):          # a NULL handle, and one the library never made: neither is looked at
        for name in ENTRIES:
            out = np.full(8, np.nan)
            rc = getattr(lib, name)(h, vp(b.ctypes.data), vp(bp.ctypes.data), vp(a.ctypes.data), vp(ap.ctypes.data),
                                    vp(out.ctypes.data))
            assert rc == 9001, name
            assert np.all(out == 0.0), name      # the result slots are cleared, never left as they came
            out = np.full(8, np.nan)
            rc = getattr(lib, name)(h, None, None, None, None, vp(out.ctypes.data))
            assert rc == 9001 and np.all(out == 0.0), name
    assert np.array_equal(b, b0) and np.array_equal(bp, bp0) and np.all(a == 7.0) and np.all(ap == 5.0)
    # the Python layer raises instead
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.devore_potentials(x, x, x, z, z)
    for gauge in ("devore", "both"):
        with pytest.raises(ndsm_amd.NdsmHipError):
            ndsm_amd.relative_helicity(x, x, x, z, gauge=gauge)


def test_devore_python_names(lib):
    import ndsm_amd
    assert "devore_potentials" in ndsm_amd.__all__ and callable(ndsm_amd.devore_potentials)
    assert callable(ndsm_amd.VecPot.devore)
    for fn in (ndsm_amd.VecPot.helicity, ndsm_amd.relative_helicity):
        par = inspect.signature(fn).parameters
        assert "gauge" in par and par["gauge"].default == "coulomb", fn
        assert par["project"].default is False, fn          # the keywords before it keep their defaults
    par = inspect.signature(ndsm_amd.VecPot.devore).parameters
    assert list(par)[1:3] == ["b", "bp"] and par["device"].default is False
    par = inspect.signature(ndsm_amd.devore_potentials).parameters
    assert list(par)[:5] == ["x", "y", "z", "b", "bp"]
    # the Helicity tuple keeps its fields
    assert ndsm_amd.Helicity._fields == ("ierr", "H_R", "H_J", "E", "E_p", "E_free", "recon_max", "recon_rms",
                                         "divB_max", "divA_max", "A", "A_p", "B_p")


def test_devore_arguments_checked_before_any_device_call(lib):
    """an unknown gauge is a ValueError and a field that does not match the mesh an argument error (9002), both
    before the library is called"""
    import ndsm_amd
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    with pytest.raises(ValueError):
        ndsm_amd.relative_helicity(x, x, x, z, gauge="temporal")
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.devore_potentials(x, x, x[:7], z, z)
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.relative_helicity(x, x, x[:7], z, gauge="devore")
    # VecPot itself: a handle object whose library would fail the test if it were reached
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.nshape4 = np.array([8, 8, 8, 3], dtype=np.intc)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library reached: " + name)
    V.L, V.h = NoCalls(), None
    for gauge in ("Coulomb", "devor", None, "both "):
        with pytest.raises(ValueError):
            V.helicity(z, gauge=gauge)
    for bad in (np.zeros((3, 8, 8, 7)), np.zeros((2, 8, 8, 8)), np.zeros((8, 8, 8, 3))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.devore(bad, z)
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.devore(z, bad)
        for gauge in ("devore", "both"):
            with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
                V.helicity(bad, gauge=gauge)
