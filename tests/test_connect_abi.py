"""CPU tests of the partition and connectivity entry points (include/ndsm_hip.h, "Flux partitioning and connectivity"):
the four symbols are declared and exported, the header's prototypes are the ones the Python binding declares, the
launchers behind them stay internal, the header states the semantics' key phrases, the new sources hold no atomic and no
assembly, without a GPU every entry fails cleanly - 9001 whatever the arguments, never a crash, counts cleared, the other
arrays untouched -, the Python names are there with the documented defaults, and the Python layer checks its options
before it reaches the library."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_cascade_abi import ROOT, HEADER

MESH = "ppp"                                   # nsrc, xs, ys
KINDS = {"ndsm_hip_partition": MESH + "pdl" + "p" * 8, "ndsm_hip_partition_device": MESH + "pdl" + "p" * 8,
         "ndsm_hip_vecpot_connect": "ppp" + "idil" + "p" * 9, "ndsm_hip_vecpot_connect_device": "ppp" + "idil" + "p" * 9}
CTYPES = {"p": ctypes.c_void_p, "i": ctypes.c_int, "d": ctypes.c_double, "l": ctypes.c_int64}


def header_kinds(name):
    """'p' (pointer or array), 'i' (int), 'l' (int64_t) or 'd' (double) per parameter of the header's prototype"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    kinds = []
    for a in (" ".join(a.split()) for a in decl.split(",")):
        if "*" in a or "[" in a:
            kinds.append("p")
        elif re.match(r"(const )?int \w+$", a):
            kinds.append("i")
        elif re.match(r"(const )?int64_t \w+$", a):
            kinds.append("l")
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
        elif t is ctypes.c_int64:
            out.append("l")
        elif t is ctypes.c_double:
            out.append("d")
        else:
            assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), t
            out.append("p")
    return "".join(out)


@pytest.fixture(scope="module")
def lib():
    import ndsm_amd
    if not os.path.exists(ndsm_amd.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ndsm_amd"), "-j", "8"])
    return ndsm_amd.load_library()


def test_connect_entries_declared_exported_and_bound(lib):
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
    iface = open(os.path.join(ROOT, "ndsm_amd", "fsrc", "ndsmh_iface.f90")).read()
    for name in ("ndsmk_partition", "ndsmk_partition_fits", "ndsmk_connect"):
        assert name in kernels and name not in open(HEADER).read()
        assert 'name="%s"' % name in iface, name
    make = open(os.path.join(ROOT, "ndsm_amd", "Makefile")).read()
    sources = make.split("HIPSRC")[1].split("\n")[0].split()
    assert "partition" in sources and "connect" in sources and "csrc/keysum.hpp" in make
    for name in ("partition.hip", "connect.hip", "keysum.hpp"):
        src = open(os.path.join(ROOT, "ndsm_amd", "csrc", name)).read()
        assert "atomic" not in src.replace("No atomics", "").lower(), name
        assert not re.search(r"\basm\b", src) and "rocprim" not in src.lower() and "hipcub" not in src.lower(), name
        if name != "keysum.hpp":
            assert "__launch_bounds__" in src and "keysum.hpp" in src, name
    walk = open(os.path.join(ROOT, "ndsm_amd", "csrc", "connect.hip")).read()
    assert "line_walk<false, false>" in walk and "tr_rk4" not in walk          # no new text of the walk
    text = open(HEADER).read()
    for phrase in ("Flux partitioning and connectivity", "Barnes, Longcope & Leka 2005", "The keyed sum",
                   "Lane l of 64 adds the ranks l, l + 64", "v[l] = v[l] + v[l + d] for l < d, d = 32, 16, ... 1",
                   "a lone -0.0 becomes +0.0", "IN iff fabs(bz) > thr", "A NaN is not in", "no padding and no wrap",
                   "equal values go", "smallest pixel index", "in ascending root index", "0.5 hx on both end rows",
                   "sx = sum f xs[i]", "NDSM_HIP_CONNECT_NONE", "not from the label", "BIT FOR BIT",
                   "clamp((int)floor((x - lo_x) / h_x + 0.5), 0, nx - 1)", "c = -status", "ascending a, then ascending c",
                   "fabs(B_z(p)) w(p)", "ONE-SIDED", "A label outside 1 .. K counts as 0"):
        assert phrase in text, phrase
    assert re.search(r"#define NDSM_HIP_CONNECT_NONE \(-9\)", text)


def test_connect_python_names(lib):
    import ndsm_amd
    for name in ("Patches", "partition_magnetogram", "Connectivity", "find_connectivity", "connectivity_matrix"):
        assert name in ndsm_amd.__all__ and hasattr(ndsm_amd, name)
    pm = inspect.signature(ndsm_amd.partition_magnetogram).parameters
    assert list(pm)[:6] == ["xs", "ys", "bz", "thr", "max_patches", "device"]
    assert [pm[k].default for k in ("thr", "max_patches", "device")] == [0.0, None, False]
    cn = inspect.signature(ndsm_amd.VecPot.connectivity).parameters
    assert list(cn)[1:] == ["b", "label", "K", "thr", "step", "max_steps", "max_pairs", "device"]
    assert [cn[k].default for k in list(cn)[2:]] == [None, None, 0.0, 0.5, None, None, False]
    fc = inspect.signature(ndsm_amd.find_connectivity).parameters
    assert list(fc)[:10] == ["x", "y", "z", "b", "label", "K", "thr", "step", "max_steps", "max_pairs"]
    cm = inspect.signature(ndsm_amd.connectivity_matrix).parameters
    assert list(cm) == ["conn", "K", "symmetric"] and cm["symmetric"].default is False
    assert ndsm_amd.Patches._fields == ("label", "root", "sign", "npix", "flux", "sx", "sy", "centroid", "nin", "K")
    assert ndsm_amd.Connectivity._fields == ("dest", "ends", "length", "status", "pa", "pc", "nlines", "pflux", "ntraced",
                                             "npairs", "label", "K")
    from ndsm_amd import _lib
    assert _lib.CONNECT_NONE == -9
    # the matrix: one-sided, the last column everything that did not land on a patch, the symmetric mean on request
    conn = ndsm_amd.Connectivity(None, None, None, None, np.array([1, 1, 1, 2, 2]), np.array([-6, 0, 2, 1, 2]),
                                 np.array([1, 1, 1, 1, 1]), np.array([1.0, 2.0, 4.0, 8.0, 16.0]), 5, 5, None, 2)
    assert np.array_equal(ndsm_amd.connectivity_matrix(conn), [[0.0, 4.0, 3.0], [8.0, 16.0, 0.0]])
    assert np.array_equal(ndsm_amd.connectivity_matrix(conn, symmetric=True), [[0.0, 6.0, 3.0], [6.0, 16.0, 0.0]])
    assert np.array_equal(ndsm_amd.connectivity_matrix(conn, K=1), [[0.0, 7.0]])


def test_connect_entries_fail_cleanly_without_a_gpu(lib):
    if lib.ndsm_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    import ndsm_amd
    L = ctypes.CDLL(ndsm_amd.lib_path(), mode=os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, "RTLD_DEEPBIND", 0))
    vp = ctypes.c_void_p
    for name in KINDS:
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [CTYPES[k] for k in header_kinds(name)]

    def p(v):
        return None if v is None else vp(v.ctypes.data)

    xs, ys, bz = np.arange(5.0), np.arange(4.0), np.linspace(-1, 1, 20)
    back = xs[::-1].copy()
    keep = [v.copy() for v in (xs, ys, bz)]
    for suffix in ("", "_device"):
        fn = getattr(L, "ndsm_hip_partition" + suffix)
        for ns, sx, thr, cap in (((5, 4), xs, 0.0, 3), ((1, 4), xs, 0.0, 3), ((5, 4), back, 0.0, 3), ((5, 4), xs, -1.0, 3),
                                 ((5, 4), xs, float("nan"), 0), ((5, 4), xs, 0.0, -1), ((0, -3), xs, 0.0, 2 ** 62),
                                 ((2 ** 30, 2 ** 30), xs, 0.0, 3)):
            counts = np.full(2, 7, dtype=np.int64)
            label = np.full(20, 7, dtype=np.int32)
            rec = [np.full(3, 7, dtype=t) for t in (np.int64, np.int32, np.int64, np.float64, np.float64, np.float64)]
            got = fn(p(np.array(ns, dtype=np.intc)), p(sx), p(ys), p(bz), thr, cap, p(counts), p(label), *map(p, rec))
            assert got == 9001, (suffix, ns, thr, cap)
            assert list(counts) == [0, 0] and (label == 7).all() and all((r == 7).all() for r in rec)
        assert fn(None, None, None, None, 0.0, 4, None, None, None, None, None, None, None, None) == 9001
        fn = getattr(L, "ndsm_hip_vecpot_connect" + suffix)
        for K, step, ms, cap in ((2, 0.5, 10, 3), (-1, 0.5, 10, 3), (2, 0.0, 0, -1), (2, float("nan"), 10, 2 ** 62)):
            counts = np.full(2, 7, dtype=np.int64)
            out = [np.full(60, 7.0) for _ in range(8)]
            assert fn(None, p(bz), p(bz), K, step, ms, cap, p(counts), *map(p, out)) == 9001, (suffix, K, step, ms, cap)
            assert list(counts) == [0, 0] and all((a == 7.0).all() for a in out)
        assert fn(None, None, None, 0, 0.5, 1, 0, None, None, None, None, None, None, None, None, None) == 9001
    for v, k in zip((xs, ys, bz), keep):
        assert np.array_equal(v, k)
    # the Python layer raises instead
    with pytest.raises(ndsm_amd.NdsmHipError, match="9001"):
        ndsm_amd.partition_magnetogram(xs, ys, bz.reshape(4, 5))
    with pytest.raises(ndsm_amd.NdsmHipError, match="9001"):
        ndsm_amd.partition_magnetogram(xs, ys, bz.reshape(4, 5), device=True)


class NoLibrary:
    """stands in for the library: any call is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("the library was reached: " + name)


def test_connect_options_checked_before_any_library_call():
    """what the library would answer with 9004, and arrays that do not fit their mesh, are a ValueError before the
    library is called"""
    import ndsm_amd
    L = NoLibrary()
    xs, ys, bz = np.arange(5.0), np.arange(4.0), np.zeros((4, 5))
    base = dict(xs=xs, ys=ys, bz=bz, lib=L)
    for kw in (dict(thr=-1e-3), dict(thr=float("nan")), dict(thr=float("inf")), dict(thr="high"), dict(max_patches=-1),
               dict(max_patches=2.5), dict(max_patches=True), dict(max_patches=2 ** 40), dict(xs=xs[:1]), dict(ys=ys[:1]),
               dict(xs=xs[::-1]), dict(ys=np.zeros(4)), dict(bz=bz.T), dict(bz=np.zeros((3, 4, 5)))):
        with pytest.raises(ValueError):
            ndsm_amd.partition_magnetogram(**dict(base, **kw))
    x = np.linspace(0.0, 1.0, 8)
    b = np.zeros((3, 8, 8, 8))
    for kw in (dict(thr=-1.0), dict(thr=float("nan")), dict(max_pairs=-1), dict(max_pairs=0.5)):
        with pytest.raises(ValueError):
            ndsm_amd.find_connectivity(x, x, x, b, lib=L, **kw)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            ndsm_amd.connectivity_matrix(ndsm_amd.Connectivity(*[None] * 11, 2), K=bad)
