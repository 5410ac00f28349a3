"""CPU tests of the dip entry points (include/ndsm_hip.h, ndsm_hip_vecpot_dips): they are declared, exported, reachable
from Python with the documented defaults, and fail cleanly - an error code, never a crash, owned outputs cleared, slack
and inputs untouched - without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndsm_hip.h")
ENTRIES = ["ndsm_hip_vecpot_dips", "ndsm_hip_vecpot_dips_device"]


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_dips_entries_declared_and_exported(lib):
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
    assert not any(s.startswith("ndsmk_dips") for s in live)
    kern = open(os.path.join(ROOT, "ndsm_amd", "csrc", "ndsm_kernels.h")).read()
    assert re.search(r"\bint\s+ndsmk_dips\s*\(", kern)
    # eleven arguments, in the documented order
    for name in ENTRIES:
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)", src, flags=re.S).group(1).split(",")
        assert len(args) == 11, (name, args)
        assert "B" in args[1] and "plane_only" in args[2] and "max_dips" in args[3] and "counts" in args[4]
        assert "edge" in args[5] and "pos" in args[6] and "bpt" in args[7] and "grad" in args[8]
        assert "curv" in args[9] and "flag" in args[10]
        assert "int64_t" in args[3] and "int64_t" in args[4] and "int64_t" in args[5] and "int32_t" in args[10]
        assert re.search(r"\bint\s+plane_only", args[2])
    # the header states the semantics: the gradient, the edges, the crossing rule, the interpolation, the record
    for phrase in ("node = i + nx (j + ny k)", "centred inside and 3-point one-sided", "exactly its operand order",
                   "edge e = 3 node + d", "has no edge d", "(a > 0) != (b > 0)", "A zero or NaN counts",
                   "exactly one edge of each family", "t = a / (a - b): one quotient, no reciprocal",
                   "q_t = q(p) + t (q(p') - q(p))", "pos_d = lo_d + (i_d + t) h_d, the sum formed first",
                   "curv = B_x,t G_x,t + B_y,t G_y,t", "is left out, not rounded in", "a DIP iff curv > 0, strict",
                   "no separate rule", "BALD PATCH, k = 0 and d != 2", "(crossings, dips, bald patches)",
                   "exact whatever the capacity", "ascending edge", "no atomic append, no sort",
                   "only truncates", "still returns 0", "counts[1] == counts[2]", "that carry flag bit 0",
                   "fewer than 3 nodes"):
        assert phrase in text, phrase
    di = open(os.path.join(ROOT, "ndsm_amd", "csrc", "dips.hip")).read()
    assert "dip_vote_k" in di and "dip_fill_k" in di and "scan64" in di and "ddq(" in di
    assert "asm" not in re.sub(r"//.*", "", di) and "atomic" not in re.sub(r"//.*", "", di)
    assert " dips " in open(os.path.join(ROOT, "ndsm_amd", "Makefile")).read()


def test_dips_entries_fail_cleanly_without_a_gpu(lib):
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
        getattr(lib, name).argtypes = [vp, vp, ctypes.c_int, ctypes.c_int64] + [vp] * 7

    def outputs():
        """counts, then the six record arrays, each with slack behind the slots the entry owns"""
        return [np.full(3 + 3, 7, dtype=np.int64), np.full(cap + 3, 7, dtype=np.int64), np.full(3 * cap + 3, np.nan),
                np.full(3 * cap + 3, np.nan), np.full(3 * cap + 3, np.nan), np.full(cap + 3, np.nan),
                np.full(cap + 3, 7, dtype=np.int32)]
    owned = [3, cap, 3 * cap, 3 * cap, 3 * cap, cap, cap]

    def ptrs(out):
        return [vp(a.ctypes.data) for a in out]

    for h in (None, vp(1)):          # a NULL handle, and one the library never made: neither is looked at
        for plane in (0, 1):
            out = outputs()
            rc = lib.ndsm_hip_vecpot_dips(h, vp(b.ctypes.data), plane, cap, *ptrs(out))
            assert rc == 9001
            for a, m in zip(out, owned):      # exactly the owned slots are cleared
                assert np.all(a[:m] == 0)
                assert np.all((a[m:] == 7) | np.isnan(a[m:]))
        # count only: the three counts are cleared, no record array is touched
        out = outputs()
        rc = lib.ndsm_hip_vecpot_dips(h, vp(b.ctypes.data), 0, 0, *ptrs(out))
        assert rc == 9001 and np.all(out[0][:3] == 0) and np.all(out[0][3:] == 7)
        for a in out[1:]:
            assert np.all((a == 7) | np.isnan(a))
        # bad scalars and NULL arrays: still 9001, and no crash
        out = outputs()
        assert lib.ndsm_hip_vecpot_dips(h, vp(b.ctypes.data), 0, -1, *ptrs(out)) == 9001
        assert np.all(out[0][:3] == 0) and np.all(out[1] == 7)
        out = outputs()
        assert lib.ndsm_hip_vecpot_dips(h, vp(b.ctypes.data), 2, 0, *ptrs(out)) == 9001
        assert np.all(out[0][:3] == 0) and np.all(out[1] == 7)
        assert lib.ndsm_hip_vecpot_dips(h, None, 0, cap, None, None, None, None, None, None, None) == 9001
        assert lib.ndsm_hip_vecpot_dips(h, None, 1, 2 ** 62, None, None, None, None, None, None, None) == 9001
        # the device entry never reads or writes through its record arrays on the host; counts is a host array
        out = outputs()
        rc = lib.ndsm_hip_vecpot_dips_device(h, vp(b.ctypes.data), 0, cap, *ptrs(out))
        assert rc == 9001
        assert np.all(out[0][:3] == 0) and np.all(out[0][3:] == 7)
        assert np.all(out[1] == 7) and np.all(np.isnan(out[2])) and np.all(np.isnan(out[5])) and np.all(out[6] == 7)
        assert lib.ndsm_hip_vecpot_dips_device(h, None, 0, cap, None, None, None, None, None, None, None) == 9001
    assert np.array_equal(b, b0)
    # the Python layer raises instead
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    for kw in ({}, dict(max_dips=0), dict(plane_only=True)):
        with pytest.raises(ndsm_amd.NdsmHipError):
            ndsm_amd.find_dips(x, x, x, z, **kw)
    with pytest.raises(ndsm_amd.NdsmHipError):
        ndsm_amd.bald_patches(x, x, x, z)


def test_dips_python_names(lib):
    import ndsm_amd
    for name in ("Dips", "find_dips", "bald_patches"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    assert ndsm_amd.Dips._fields == ("position", "edge", "axis", "node", "b", "grad", "curv", "kappa", "bald",
                                     "ncrossings", "ndips", "nbald")
    par = inspect.signature(ndsm_amd.VecPot.dips).parameters
    assert list(par)[1:] == ["b", "plane_only", "max_dips", "device"]
    assert (par["plane_only"].default, par["max_dips"].default, par["device"].default) == (False, None, False)
    par = inspect.signature(ndsm_amd.find_dips).parameters
    assert list(par)[:4] == ["x", "y", "z", "b"]
    assert (par["plane_only"].default, par["max_dips"].default) == (False, None)
    par = inspect.signature(ndsm_amd.bald_patches).parameters
    assert list(par)[:4] == ["x", "y", "z", "b"] and "plane_only" not in par and par["max_dips"].default is None
    par = inspect.signature(ndsm_amd.VecPot.bald_patch_lines).parameters
    assert list(par)[1:4] == ["b", "dips", "lift"] and par["lift"].default == 1e-3
    assert par[list(par)[-1]].kind == inspect.Parameter.VAR_KEYWORD
    # existing signatures are unchanged
    par = inspect.signature(ndsm_amd.VecPot.nulls).parameters
    assert list(par)[1:] == ["b", "max_nulls", "merge", "device"]
    par = inspect.signature(ndsm_amd.VecPot.paths).parameters
    assert list(par)[1:] == ["b", "seeds", "g", "step", "max_steps", "direction", "every", "max_points", "values",
                             "device"]


def test_dips_arguments_checked_before_any_device_call(lib):
    """bad options are a ValueError and arrays that do not fit an argument error (9002), before the library is
    called"""
    import ndsm_amd
    from ndsm_amd import _lib
    x = np.linspace(0, 1, 8)
    z = np.zeros((3, 8, 8, 8))
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.find_dips(x, x, x[:7], z)
    V = ndsm_amd.VecPot.__new__(ndsm_amd.VecPot)
    V.nshape4 = np.array([8, 8, 8, 3], dtype=np.intc)
    V.x = V.y = V.z = x

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library reached: " + name)
    V.L, V.h = NoCalls(), None
    for kw in (dict(max_dips=-1), dict(max_dips=2.5), dict(max_dips=True), dict(max_dips="4"),
               dict(max_dips=float("inf")), dict(max_dips=float("nan")), dict(max_dips=2 ** 40 + 1),
               dict(plane_only=1), dict(plane_only=None), dict(plane_only="yes"), dict(plane_only=2)):
        with pytest.raises(ValueError):
            V.dips(z, **kw)
        with pytest.raises(ValueError):
            ndsm_amd.find_dips(x, x, x, z, **kw)
    for bad in (np.zeros((3, 8, 8, 7)), np.zeros((2, 8, 8, 8)), np.zeros((8, 8, 8, 3))):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.dips(bad)
    empty = _lib._dips_tuple([np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)),
                              np.zeros(0), np.zeros(0, dtype=np.int32)], [4, 0, 0], 8, 8)
    for kw in (dict(lift=-1.0), dict(lift=float("nan")), dict(lift=True), dict(lift="1e-3"), dict(direction="forward")):
        with pytest.raises(ValueError):
            V.bald_patch_lines(z, empty, **kw)


def test_dips_python_tuple_of_records():
    """the host-side part of the Dips tuple: axis, node, kappa and bald from the raw records, and the seeds of
    bald_patch_lines"""
    from ndsm_amd import _lib
    nx, ny = 5, 4
    edge = np.array([3 * (2 + nx * (1 + ny * 0)) + 0, 3 * (4 + nx * (3 + ny * 0)) + 2, 3 * (1 + nx * (2 + ny * 3)) + 1],
                    dtype=np.int64)
    pos = np.arange(9.0).reshape(3, 3)
    bpt = np.array([[3.0, 4.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    rec = [edge, pos, bpt, np.ones((3, 3)), np.array([50.0, 3.0, 1.0]), np.array([1, 0, 0], dtype=np.int32)]
    got = _lib._dips_tuple(rec, np.array([9, 3, 1]), nx, ny)
    assert got.axis.tolist() == [0, 2, 1] and got.node.tolist() == [[2, 1, 0], [4, 3, 0], [1, 2, 3]]
    assert got.kappa.tolist() == [2.0, 3.0, 0.25] and got.bald.tolist() == [True, False, False]
    assert (got.ncrossings, got.ndips, got.nbald) == (9, 3, 1) and got.bald.dtype == bool
    seeds = _lib._bald_seeds(got, 1e-3, 0.5)
    assert seeds.shape == (1, 3) and seeds[0].tolist() == [0.0, 1.0, 2.0 + 1e-3 * 0.5]
    empty = _lib._dips_tuple([a[:0] for a in rec], np.zeros(3, dtype=np.int64), nx, ny)
    assert empty.position.shape == (0, 3) and empty.node.shape == (0, 3) and empty.kappa.shape == (0,)
    assert _lib._bald_seeds(empty, 1e-3, 0.5).shape == (0, 3)
