"""CPU tests of the current-carrying-field entry points (include/ndsm_hip.h, part 2): they are declared,
exported, reachable from Python, and fail cleanly - an error code, never a crash - without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndsm_hip.h")
ENTRIES = ["ndsm_hip_vecpot_solve_field", "ndsm_hip_vecpot_solve_field_device", "ndsm_hip_vecpot_helicity",
           "ndsm_hip_vecpot_helicity_device"]


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_field_entries_declared_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    import ndsm_amd
    out = subprocess.check_output(["nm", "-D", "--defined-only", ndsm_amd.lib_path()], text=True)
    live = {l.split()[-1] for l in out.splitlines() if re.search(r" T ", l)}
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in live, name
        assert hasattr(lib, name)


def test_field_entries_fail_cleanly_without_a_gpu(lib):
    if lib.ndsm_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    import ndsm_amd
    # a CDLL object of its own (the same loaded library): prototypes set here stay private to this test
    lib = ctypes.CDLL(ndsm_amd.lib_path(), mode=os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, "RTLD_DEEPBIND", 0))
    vp = ctypes.c_void_p
    ioptc = np.zeros(16, dtype=np.intc)
    ropt = np.zeros(16)
    a, b, c, d = (np.zeros(3 * 8 ** 3) for _ in range(4))
    out = np.full(8, np.nan)
    for name in ENTRIES:
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [vp] * (5 if "solve_field" in name else 8)
    ip, dp = vp(ioptc.ctypes.data), vp(ropt.ctypes.data)
    for h in (None, vp(1)):          # a NULL handle, and one the library never made: neither is looked at
        assert lib.ndsm_hip_vecpot_solve_field(h, ip, dp, vp(a.ctypes.data), vp(b.ctypes.data)) == 9001
        assert lib.ndsm_hip_vecpot_solve_field_device(h, ip, dp, vp(a.ctypes.data), vp(b.ctypes.data)) == 9001
        for name in ("ndsm_hip_vecpot_helicity", "ndsm_hip_vecpot_helicity_device"):
            rc = getattr(lib, name)(h, ip, dp, vp(b.ctypes.data), vp(a.ctypes.data), vp(c.ctypes.data),
                                    vp(d.ctypes.data), vp(out.ctypes.data))
            assert rc == 9001, name
            assert np.all(out == 0.0), name      # the result slots are cleared, never left as they came
    assert lib.ndsm_hip_vecpot_solve_field(None, ip, dp, None, None) == 9001
    assert not np.any(a) and not np.any(b)
    # the Python layer raises instead
    x = np.linspace(0, 1, 8)
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.vector_potential_field(x, x, x, np.zeros((3, 8, 8, 8)))
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.relative_helicity(x, x, x, np.zeros((3, 8, 8, 8)))


def test_field_python_names(lib):
    import ndsm_amd
    for name in ("vector_potential_field", "relative_helicity", "Helicity"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name), name
    assert callable(ndsm_amd.VecPot.solve_field) and callable(ndsm_amd.VecPot.helicity)
    assert ndsm_amd.Helicity._fields[:10] == ("ierr", "H_R", "H_J", "E", "E_p", "E_free", "recon_max", "recon_rms",
                                              "divB_max", "divA_max")


def test_field_one_shot_rejects_a_wrong_shape(lib):
    """a field that does not match the mesh is an argument error before any device call"""
    import ndsm_amd
    x = np.linspace(0, 1, 8)
    for fn in (ndsm_amd.vector_potential_field, ndsm_amd.relative_helicity):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            fn(x, x, x[:7], np.zeros((3, 8, 8, 8)))
