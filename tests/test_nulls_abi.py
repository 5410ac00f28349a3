"""CPU tests of the null-point entry points (include/ndsm_hip.h, part 2): they are declared, exported, reachable from
Python with the documented defaults, and fail cleanly - an error code, never a crash, owned outputs cleared, slack and
inputs untouched - without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndsm_hip.h")
ENTRIES = ["ndsm_hip_vecpot_nulls", "ndsm_hip_vecpot_nulls_device"]


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_nulls_entries_declared_and_exported(lib):
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
    assert not any(s.startswith("ndsmk_nulls") for s in live)
    kern = open(os.path.join(ROOT, "ndsm_amd", "csrc", "ndsm_kernels.h")).read()
    assert re.search(r"\bint\s+ndsmk_nulls\s*\(", kern)
    # eleven arguments, in the documented order
    for name in ENTRIES:
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)", src, flags=re.S).group(1).split(",")
        assert len(args) == 11, (name, args)
        assert "max_nulls" in args[2] and "counts" in args[3] and "cell" in args[4] and "pos" in args[5]
        assert "jac" in args[6] and "det" in args[7] and "resid" in args[8] and "sign" in args[9] and "iters" in args[10]
        assert "int64_t" in args[3] and "int64_t" in args[4] and "int32_t" in args[9]
    # the header states the semantics: the constants, the starts, the guards and the sign convention
    for phrase in ("AT MOST 20 ITERATIONS", "|f_d - 1/2| <= 2.5", "max_d |delta_d| <= 2^-40",
                   "-2^-30 <= f_d <= 1 + 2^-30", "NINE STARTS", "(1/2, 1/2, 1/2)", "x fastest and z slowest",
                   "all > 0 or all < 0", "a zero corner never excludes a cell", "A cell with a NaN",
                   "det = (J00 A00 + J01 A10) + J02 A20", "three quotients, no",
                   "sign = +1 for det M < 0 (a positive null: two eigenvalues with positive real part",
                   "-1 for det M > 0, 0 otherwise", "pos_d = lo_d + (c_d + f_d) h_d",
                   "ascending cell", "32 * (number of the start", "At most one null per cell"):
        assert phrase in text, phrase
    nu = open(os.path.join(ROOT, "ndsm_amd", "csrc", "nulls.hip")).read()
    assert "node_code_k" in nu and "newton_k" in nu and "asm" not in re.sub(r"//.*", "", nu)
    assert " nulls " in open(os.path.join(ROOT, "ndsm_amd", "Makefile")).read()
    # line.hpp's inlines are added to, not edited: the kernels of trace and squash still find theirs
    line = open(os.path.join(ROOT, "ndsm_amd", "csrc", "line.hpp")).read()
    for fn in ("line_cell", "line_gather", "line_lerp3", "line_lerp3_grad", "line_lerp3_fgrad", "line_first_face"):
        assert re.search(r"\b" + fn + r"\s*\(", line), fn


def test_nulls_entries_fail_cleanly_without_a_gpu(lib):
    if lib.ndsm_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    import ndsm_amd
    # a CDLL object of its own (the same loaded library): prototypes set here stay private to this test
    lib = ctypes.CDLL(ndsm_amd.lib_path(), mode=os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, "RTLD_DEEPBIND", 0))
    vp = ctypes.c_void_p
    n, cap = 3 * 8 ** 3, 5
    b = np.linspace(-1.0, 1.0, n)
    b0 = b.copy()
    for name in ENTRIES:
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [vp, vp, ctypes.c_int] + [vp] * 8

    def outputs():
        """counts, then the seven record arrays, each with slack behind the slots the entry owns"""
        return [np.full(2 + 3, 7, dtype=np.int64), np.full(cap + 3, 7, dtype=np.int64), np.full(3 * cap + 3, np.nan),
                np.full(9 * cap + 3, np.nan), np.full(cap + 3, np.nan), np.full(cap + 3, np.nan),
                np.full(cap + 3, 7, dtype=np.int32), np.full(cap + 3, 7, dtype=np.int32)]
    owned = [2, cap, 3 * cap, 9 * cap, cap, cap, cap, cap]

    for h in (None, vp(1)):          # a NULL handle, and one the library never made: neither is looked at
        out = outputs()
        rc = lib.ndsm_hip_vecpot_nulls(h, vp(b.ctypes.data), cap, *[vp(a.ctypes.data) for a in out])
        assert rc == 9001
        for a, m in zip(out, owned):      # exactly the owned slots are cleared
            assert np.all(a[:m] == 0)
            assert np.all((a[m:] == 7) | np.isnan(a[m:]))
        # count only: the two counts are cleared, no record array is touched
        out = outputs()
        rc = lib.ndsm_hip_vecpot_nulls(h, vp(b.ctypes.data), 0, *[vp(a.ctypes.data) for a in out])
        assert rc == 9001 and np.all(out[0][:2] == 0) and np.all(out[0][2:] == 7)
        for a in out[1:]:
            assert np.all((a == 7) | np.isnan(a))
        # a bad scalar and NULL arrays: still 9001, and no crash
        out = outputs()
        assert lib.ndsm_hip_vecpot_nulls(h, vp(b.ctypes.data), -1, *[vp(a.ctypes.data) for a in out]) == 9001
        assert np.all(out[0][:2] == 0) and np.all(out[1] == 7)
        assert lib.ndsm_hip_vecpot_nulls(h, None, cap, None, None, None, None, None, None, None, None) == 9001
        assert lib.ndsm_hip_vecpot_nulls(h, None, 2 ** 31 - 1, None, None, None, None, None, None, None, None) == 9001
        # the device entry never reads or writes through its record arrays on the host; counts is a host array
        out = outputs()
        rc = lib.ndsm_hip_vecpot_nulls_device(h, vp(b.ctypes.data), cap, *[vp(a.ctypes.data) for a in out])
        assert rc == 9001
        assert np.all(out[0][:2] == 0) and np.all(out[0][2:] == 7)
        assert np.all(out[1] == 7) and np.all(np.isnan(out[2])) and np.all(np.isnan(out[3])) and np.all(out[7] == 7)
        assert lib.ndsm_hip_vecpot_nulls_device(h, None, cap, None, None, None, None, None, None, None, None) == 9001
    assert np.array_equal(b, b0)
    # the Python layer raises instead
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    for kw in ({}, dict(max_nulls=0), dict(merge=None)):
        with pytest.raises(ndsm_amd.NdsmHipError):
            ndsm_amd.find_nulls(x, x, x, z, **kw)


def test_nulls_python_names(lib):
    import ndsm_amd
    for name in ("Nulls", "find_nulls"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    assert ndsm_amd.Nulls._fields == ("position", "cell", "jacobian", "sign", "spiral", "eigenvalues", "spine", "fan",
                                      "det", "residual", "ncandidates", "nfound")
    par = inspect.signature(ndsm_amd.VecPot.nulls).parameters
    assert list(par)[1:] == ["b", "max_nulls", "merge", "device"]
    assert (par["max_nulls"].default, par["merge"].default, par["device"].default) == (4096, 1e-6, False)
    par = inspect.signature(ndsm_amd.find_nulls).parameters
    assert list(par)[:4] == ["x", "y", "z", "b"]
    assert (par["max_nulls"].default, par["merge"].default) == (4096, 1e-6)
    # existing signatures are unchanged
    par = inspect.signature(ndsm_amd.VecPot.squashing).parameters
    assert list(par)[1:] == ["b", "seeds", "g", "integrand", "twist", "step", "max_steps", "device"]
    par = inspect.signature(ndsm_amd.VecPot.trace).parameters
    assert list(par)[1:] == ["b", "seeds", "g", "step", "max_steps", "direction", "device"]
    assert ndsm_amd.QMap._fields == ("q", "twist", "ends", "length", "integral", "status", "nsteps")


def test_nulls_arguments_checked_before_any_device_call(lib):
    """bad options are a ValueError and arrays that do not fit an argument error (9002), before the library is
    called"""
    import ndsm_amd
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.find_nulls(x, x, x[:7], z)
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.nshape4 = np.array([8, 8, 8, 3], dtype=np.intc)

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library reached: " + name)
    V.L, V.h = NoCalls(), None
    for kw in (dict(max_nulls=-1), dict(max_nulls=2.5), dict(max_nulls=None), dict(max_nulls=True),
               dict(max_nulls=2 ** 31), dict(max_nulls=float("inf")), dict(max_nulls=float("nan")),
               dict(max_nulls=2 ** 24 + 1), dict(merge=-1.0), dict(merge=float("nan")), dict(merge=float("inf")),
               dict(merge="1e-6"), dict(merge=True)):
        with pytest.raises(ValueError):
            V.nulls(z, **kw)
    for bad in (np.zeros((3, 8, 8, 7)), np.zeros((2, 8, 8, 8)), np.zeros((8, 8, 8, 3))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.nulls(bad)


def test_nulls_python_typing_of_records():
    """the host-side typing (numpy.linalg.eig of the returned Jacobian) and the merge of records"""
    from ndsm_amd import _lib
    M = np.array([[1.0, -3.0, 0.0], [3.0, 1.0, 0.0], [0.0, 0.0, -2.0]])
    pos = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5 + 1e-9], [0.7, 0.5, 0.5]])
    rec = [np.array([3, 9, 11], dtype=np.int64), pos, np.stack([M, M, -M]), np.array([-20.0, -20.0, 20.0]),
           np.zeros(3), np.array([1, 1, -1], dtype=np.int32), np.array([2, 2, 2], dtype=np.int32)]
    raw = _lib._nulls_tuple(rec, 5, 3, None)
    assert len(raw.cell) == 3 and raw.ncandidates == 5 and raw.nfound == 3
    got = _lib._nulls_tuple(rec, 5, 3, 1e-6)
    assert got.cell.tolist() == [3, 11] and got.sign.tolist() == [1, -1] and got.nfound == 3
    assert got.spiral.tolist() == [True, True]
    assert got.eigenvalues[0][0] == -2.0 and got.eigenvalues[1][0] == 2.0
    assert np.allclose(np.abs(got.spine), [[0, 0, 1], [0, 0, 1]])
    assert got.fan.shape == (2, 2, 3) and got.position.shape == (2, 3) and got.jacobian.shape == (2, 3, 3)
    empty = _lib._nulls_tuple([a[:0] for a in rec], 0, 0, 1e-6)
    assert empty.position.shape == (0, 3) and empty.spine.shape == (0, 3) and empty.fan.shape == (0, 2, 3)
    assert empty.spiral.shape == (0,) and empty.eigenvalues.shape == (0, 3)
