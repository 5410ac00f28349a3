"""GPU tests of the resampling entries (csrc/resample.hip) and of the coarse-to-fine cascade of the optimization method
(vecpot_optimize_cascade) against their numpy model (tests/cascade_model.py), bit for bit: fields as uint64, every
history row, info.  The model restates the 1-D rules and strings optimize_model.run calls together; nothing here is
taken from the device code's results.  Shapes are written nx x ny x nz as in the library."""
import ctypes

import numpy as np
import pytest

import cascade_model as C
import optimize_model as M
from device_arena import Arena, LibTransport, slot
from golden_inputs import aniso_mesh, uniform_mesh

pytestmark = pytest.mark.gpu

_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
IDS = lambda s: "x".join(map(str, s))   # noqa: E731
FILL = 7

# source -> destination, nx x ny x nz.  4x4x4 -> itself: every node a copy; 5x7x4 -> 3x4x4: a 2:1 axis, a 7 -> 4 axis
# that is not nested, an axis kept; 33x22x27: the suite's anisotropic shape onto its (n + 1) // 2 shape and onto one
# with ratios that are no whole numbers; 513 -> 257: more than one block along x; 9x6x1 -> 5x4x1: a plane
BOTH = [([4, 4, 4], [4, 4, 4]), ([5, 7, 4], [3, 4, 4]), ([33, 22, 27], [17, 11, 14]), ([33, 22, 27], [13, 9, 10]),
        ([513, 4, 4], [257, 4, 4]), ([9, 6, 1], [5, 4, 1])]
# upwards, linear only: destinations one past a multiple of the 64 x 4 x 1 block along x and y; 2116 (y, z) rows
UP = [([3, 4, 2], [65, 9, 5]), ([5, 4, 4], [129, 4, 5]), ([4, 4, 4], [5, 46, 46])]
RESAMPLE_CASES = [(s, d, m) for s, d in BOTH for m in C.MODES] + [(s, d, "linear") for s, d in UP]

# finest first; [17x13x13, 9x7x7, 5x4x4]: three levels; [65x9x5, 33x5x4]: a z axis 5 -> 4 that is not nested
LEVEL_SETS = ([[9, 9, 7], [5, 5, 4]], [[12, 10, 9], [6, 5, 5]], [[17, 13, 13], [9, 7, 7], [5, 4, 4]],
              [[65, 9, 5], [33, 5, 4]])
CASCADE_CASES = [("uniform", s) for s in LEVEL_SETS] + [("aniso", LEVEL_SETS[1])]
MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def rough(shape, ncomp, seed=1):
    """no symmetry, no zeros, not smooth: every tap and every weight shows"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, size=(ncomp,) + tuple(shape)) + 1.5
    return a if ncomp > 1 else a[0]


def bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    assert not bad.any(), (what, int(bad.sum()), float(np.nanmax(np.abs(got - want))))


def level_meshes(mname, sets):
    fine = MESHES[mname](sets[0])
    return [fine] + [[np.linspace(q[0], q[-1], n) for q, n in zip(fine, s)] for s in sets[1:]]


def field(mesh):
    return M.perturbed_abc(mesh)[1]


def weight(kind, mesh, shape):
    import ndsm_amd
    if kind == "none":
        return None
    if kind == "cosine":
        return ndsm_amd.boundary_weight(shape, 2)
    u = [(q - q[0]) / (q[-1] - q[0]) for q in mesh]
    Z, Y, X = np.meshgrid(u[2], u[1], u[0], indexing="ij")
    return 1.0 + 0.8 * np.sin(3.0 * X + 0.5 + Y * Z) * np.cos(2.0 * Y) + 0.5 * Z * X      # not a product of 1-D factors


def same(got, want, what):
    """(B, [hist], [info]) of the device against the model's, bit for bit"""
    gB, gh, gi = got
    wB, wh, wi = want
    assert list(gi) == list(wi), (what, gi, wi)
    for l, (a, b) in enumerate(zip(gh, wh)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, l, a, b)
    bits(gB, wB, what)


@pytest.mark.parametrize("src,dst,mode", RESAMPLE_CASES, ids=["%s-%s-%s" % (IDS(s), IDS(d), m) for s, d, m in RESAMPLE_CASES])
def test_resample_equals_the_model(hip, src, dst, mode):
    """one and three components, the host and the device entry"""
    import ndsm_amd
    for ncomp in (1, 3):
        a = rough(src[::-1], ncomp)
        want = C.resample(a, tuple(dst[::-1]), mode)
        for device in (False, True):
            got = ndsm_amd.resample(a, tuple(dst[::-1]), mode=mode, device=device)
            bits(got, want, "%s -> %s %s ncomp %d device %s" % (src, dst, mode, ncomp, device))


def test_resample_faces_come_from_faces_only(hip):
    """NaN everywhere inside the source: every face node of the result is finite and has the bits of the clean run"""
    import ndsm_amd
    a = rough((27, 22, 33), 3)
    holed = a.copy()
    holed[:, 1:-1, 1:-1, 1:-1] = np.nan
    for dst in ((14, 11, 17), (10, 9, 13), (4, 4, 4)):
        f = C.faces(dst)
        for mode in C.MODES:
            clean = ndsm_amd.resample(a, dst, mode=mode)
            got = ndsm_amd.resample(holed, dst, mode=mode, device=True)
            assert np.isfinite(got[:, f]).all(), (dst, mode)
            bits(got[:, f], clean[:, f], "faces %s %s" % (dst, mode))
    small = rough((5, 4, 3), 3)
    small[:, 1:-1, 1:-1, 1:-1] = np.nan
    up = ndsm_amd.resample(small, (9, 9, 65), device=True)
    f = C.faces((9, 9, 65))
    assert np.isfinite(up[:, f]).all() and np.isnan(up[:, ~f]).any()


@pytest.mark.parametrize("src,dst,mode", [([33, 22, 27], [13, 9, 10], "average"), ([5, 7, 4], [3, 4, 4], "linear"),
                                          ([3, 4, 2], [65, 9, 5], "linear")], ids=["average-down", "linear-down", "linear-up"])
def test_resample_device_entry_on_offset_arrays(hip, src, dst, mode):
    """views into one larger allocation, 8 mod 16, NaN bands beside the source: the result is that of arrays of their
    own, the source and every guard byte stay as they were"""
    import ndsm_amd
    L = ndsm_amd.load_library()
    a = rough(src[::-1], 3)
    want = C.resample(a, tuple(dst[::-1]), mode)
    ns3, nd3 = np.array(src, dtype=np.intc), np.array(dst, dtype=np.intc)
    for plain in (False, True):
        R = Arena(LibTransport(L), [slot("src", a.reshape(-1), field=True),
                                    slot("dst", np.full(want.size, 3.25), output=True)], plain=plain)
        got = R.run(lambda ds, dd: L.ndsm_hip_resample_device(ns3.ctypes.data_as(_ip), nd3.ctypes.data_as(_ip), 3,
                                                              hip.RESAMPLE_MODES[mode], ds, dd))
        assert R.rc == 0, hip.last_error(L)
        bits(got[1].reshape(want.shape), want, "plain %s" % plain)


def test_resample_argument_errors(hip):
    import ndsm_amd
    L = ndsm_amd.load_library()
    a = rough((4, 5, 6), 2)
    for name in ("ndsm_hip_resample", "ndsm_hip_resample_device"):
        fn = getattr(L, name)
        dev = name.endswith("_device")
        ps, pd = ctypes.c_void_p(), ctypes.c_void_p()
        assert L.ndsm_hip_device_alloc(a.nbytes, ctypes.byref(ps)) == 0
        assert L.ndsm_hip_device_alloc(8 * a.nbytes, ctypes.byref(pd)) == 0
        try:
            out = np.full(8 * a.size, 3.25)
            assert L.ndsm_hip_memcpy_h2d(ps, a.ctypes.data, a.nbytes) == 0
            assert L.ndsm_hip_memcpy_h2d(pd, out.ctypes.data, out.nbytes) == 0

            def call(ns=(6, 5, 4), nd=(3, 3, 4), ncomp=2, mode=1, src=True, dst=True, shapes=(True, True)):
                s3, d3 = np.array(ns, dtype=np.intc), np.array(nd, dtype=np.intc)
                S = (ps if dev else ctypes.c_void_p(a.ctypes.data)) if src else None
                D = (pd if dev else ctypes.c_void_p(out.ctypes.data)) if dst else None
                return fn(s3.ctypes.data_as(_ip) if shapes[0] else None, d3.ctypes.data_as(_ip) if shapes[1] else None,
                          ncomp, mode, S, D)
            for kw in (dict(ncomp=0), dict(ncomp=-1), dict(mode=2), dict(mode=-1), dict(nd=(7, 3, 4)), dict(nd=(3, 3, 5)),
                       dict(nd=(1, 3, 4)), dict(ns=(1, 5, 4), mode=0), dict(nd=(3, 0, 4)), dict(ns=(6, 5, 1), mode=0),
                       dict(ns=(6, 5, 1), nd=(3, 3, 2), mode=0)):
                assert call(**kw) == 9004, (name, kw)
            for kw in (dict(src=False), dict(dst=False), dict(shapes=(False, True)), dict(shapes=(True, False))):
                assert call(**kw) == 9002, (name, kw)
            back = np.empty_like(out)
            assert L.ndsm_hip_memcpy_d2h(back.ctypes.data, pd, out.nbytes) == 0
            assert (back == 3.25).all() and (out == 3.25).all()          # a failed call leaves dst as it was
            assert call() == 0 and call(ns=(6, 5, 1), nd=(3, 3, 1)) == 0
        finally:
            L.ndsm_hip_device_free(ps)
            L.ndsm_hip_device_free(pd)
    for bad in (dict(mode="cubic"), dict(shape=(4, 5)), dict(shape=(9, 5, 6), mode="average")):
        with pytest.raises(ValueError):
            ndsm_amd.resample(a, **dict(dict(shape=(4, 5, 6)), **bad))


def handles(meshes):
    import ndsm_amd
    return [ndsm_amd.VecPot(*m) for m in meshes]


@pytest.mark.parametrize("mname,sets", CASCADE_CASES, ids=[m + "-" + "-".join(IDS(s) for s in ss) for m, ss in CASCADE_CASES])
def test_cascade_equals_the_model(hip, mname, sets):
    """start given; without a weight, with boundary_weight(nd = 2) and with a non-separable weight; 1, 2 and 7 tries on
    successive levels, check 3; the host and the device entry.  The faces of the result are the input's"""
    meshes = level_meshes(mname, sets)
    b = field(meshes[0])
    nit = [1, 2, 7][:len(sets)]
    Vs = handles(meshes)
    try:
        for kind in ("none", "cosine", "nonsep"):
            w = weight(kind, meshes[0], b.shape[1:])
            wB, wh, wi, _ = C.cascade(meshes, b, w, niter_max=nit, check=3, tol=0.0)
            for device in (False, True):
                what = "%s %s w %s device %s" % (mname, sets, kind, device)
                ierr, B, hist, info = Vs[0].optimize_cascade(Vs[1:], b, w=w, start="given", niter_max=nit, check=3,
                                                             tol=0.0, device=device)
                assert ierr == 0, what
                same((B, hist, info), (wB, wh, wi), what)
                f = C.faces(b.shape[1:])
                bits(B[:, f], b[:, f], what + ", faces")
                assert [i[1] for i in info] == nit and all(np.isfinite(h).all() for h in hist), (what, info)
    finally:
        for V in Vs:
            V.close()


def test_cascade_goes_on_past_a_level_that_stops_at_dt_min(hip):
    """dt0 below dt_min on the coarse level only: one row, no try there, and the fine level runs"""
    meshes = level_meshes("uniform", LEVEL_SETS[0])
    b = field(meshes[0])
    h2 = [min(M.spacing(m)) ** 2 for m in meshes]
    kw = dict(niter_max=[4, 5], check=2, tol=0.0, dt0=[0.1 * h2[0], 1.0], dt_min=[1e-7 * h2[0], 2.0])
    want = C.cascade(meshes, b, None, **kw)
    Vs = handles(meshes)
    try:
        ierr, B, hist, info = Vs[0].optimize_cascade(Vs[1:], b, start="given", **kw)
        assert ierr == 0
        same((B, hist, info), want[:3], "dt_min on the coarse level")
        assert info[1] == (1, 0, 2) and info[0] == (3, 4, 0), info
    finally:
        for V in Vs:
            V.close()


def test_one_level_is_optimize_itself(hip):
    import ndsm_amd
    mesh = uniform_mesh([12, 10, 9])
    b = field(mesh)
    w = weight("cosine", mesh, b.shape[1:])
    V = ndsm_amd.VecPot(*mesh)
    try:
        for start in ("given", "potential"):
            for device in (False, True):
                one = V.optimize(b, w=w, start=start, niter_max=3, check=2, tol=0.0, device=device)
                ierr, B, hist, info = V.optimize_cascade([], b, w=w, start=start, niter_max=3, check=2, tol=0.0,
                                                         device=device)
                assert ierr == one[0] and len(hist) == 1 and len(info) == 1
                same((B, hist, info), (one[1], [one[2]], [one[3]]), "one level, start %s device %s" % (start, device))
    finally:
        V.close()


@pytest.mark.parametrize("mname,sets", [("uniform", [[12, 10, 9], [6, 5, 5]]), ("aniso", [[17, 13, 13], [9, 7, 7], [5, 4, 4]])],
                         ids=["uniform-2", "aniso-3"])
def test_potential_start_is_the_chain_of_public_calls(hip, mname, sets):
    """resample (average) of b, optimize(start = "potential") on the coarsest handle, then per finer level resample
    (linear), the k = 0 plane of that level's average of b pasted, optimize(start = "given")"""
    import ndsm_amd
    meshes = level_meshes(mname, sets)
    shapes = [C.shape_of(m) for m in meshes]
    b = field(meshes[0])
    nit = [2, 3, 4][:len(sets)]
    Vs = handles(meshes)
    try:
        for w in (None, weight("nonsep", meshes[0], b.shape[1:])):
            G = [b] + [ndsm_amd.resample(b, s, mode="average") for s in shapes[1:]]
            W = [w] + [None if w is None else ndsm_amd.resample(w, s, mode="linear") for s in shapes[1:]]
            hist, info = [None] * len(sets), [None] * len(sets)
            last = len(sets) - 1
            ierr_c, cur, hist[last], info[last] = Vs[last].optimize(G[last], w=W[last], start="potential",
                                                                    niter_max=nit[last], check=2, tol=0.0)
            for l in range(last - 1, -1, -1):
                s = ndsm_amd.resample(cur, shapes[l], mode="linear")
                s[:, 0] = G[l][:, 0]
                rc, cur, hist[l], info[l] = Vs[l].optimize(s, w=W[l], start="given", niter_max=nit[l], check=2, tol=0.0)
                assert rc == 0
            for device in (False, True):
                ierr, B, gh, gi = Vs[0].optimize_cascade(Vs[1:], b, w=w, start="potential", niter_max=nit, check=2,
                                                         tol=0.0, device=device)
                assert ierr == ierr_c                                          # the coarsest solve's flag is passed on
                same((B, gh, gi), (cur, hist, info), "potential start, device %s" % device)
                assert np.array_equal(B[:, 0], b[:, 0]) and not np.array_equal(B[:, -1], b[:, -1])
    finally:
        for V in Vs:
            V.close()


def options(V):
    return V._options(10000, 1024, 1e-13, 1e-10, 5, False, False, False)


def test_argument_errors_of_the_c_entries(hip):
    import ndsm_amd
    meshes = level_meshes("uniform", [[9, 9, 7], [5, 5, 4]])
    b = field(meshes[0])
    shifted = [q.copy() for q in meshes[1]]
    shifted[1][-1] = np.nextafter(shifted[1][-1], 2.0)                         # one bit off the box in y
    Vs = handles(meshes)
    Vbad = ndsm_amd.VecPot(*shifted)
    L = Vs[0].L
    nan, inf = float("nan"), float("inf")
    try:
        dB = ctypes.c_void_p()
        assert L.ndsm_hip_device_alloc(b.nbytes, ctypes.byref(dB)) == 0
        try:
            for name, host in (("ndsm_hip_vecpot_optimize_cascade", True), ("ndsm_hip_vecpot_optimize_cascade_device", False)):
                fn = getattr(L, name)

                def call(hs=(Vs[0].h, Vs[1].h), nl=None, B=True, start=1, nit=(2, 3), check=2, tol=0.0, d0=(1e-3, 1e-3),
                         dm=(0.0, 0.0), rows=4, hist=True, info=True, per=(True, True, True), harr=True):
                    nl = len(hs) if nl is None else nl
                    io, ro = options(Vs[0])
                    harray = (ctypes.c_void_p * max(len(hs), 1))(*hs)
                    n_a, d_a, m_a = np.array(nit, dtype=np.intc), np.array(d0, dtype=np.float64), np.array(dm, dtype=np.float64)
                    hh, ii = np.full((2, 4, 6), nan), np.full((2, 3), FILL, dtype=np.intc)
                    B0 = b.copy()
                    assert L.ndsm_hip_memcpy_h2d(dB, B0.ctypes.data, B0.nbytes) == 0
                    rc = fn(harray if harr else None, nl, io.ctypes.data_as(_ip), ro.ctypes.data_as(_dp),
                            (ctypes.c_void_p(B0.ctypes.data) if host else dB) if B else None, None, start,
                            n_a.ctypes.data if per[0] else None, check, tol, d_a.ctypes.data if per[1] else None,
                            m_a.ctypes.data if per[2] else None, hh.ctypes.data if hist else None, rows,
                            ii.ctypes.data if info else None)
                    if not host:
                        assert L.ndsm_hip_memcpy_d2h(B0.ctypes.data, dB, B0.nbytes) == 0
                    return rc, hh, ii, B0
                rc, hh, ii, _ = call()
                assert rc == 0 and [tuple(r) for r in ii] == [(2, 2, 0), (3, 3, 0)] and np.isnan(hh[0, 2:]).all(), (rc, ii)
                for kw in (dict(nl=0), dict(nl=-1), dict(start=2), dict(start=-1), dict(nit=(2, 0)), dict(nit=(0, 3)),
                           dict(check=0), dict(rows=1), dict(tol=-1e-9), dict(tol=nan), dict(tol=inf), dict(d0=(1e-3, 0.0)),
                           dict(d0=(nan, 1e-3)), dict(d0=(1e-3, inf)), dict(dm=(0.0, -1.0)), dict(dm=(nan, 0.0)),
                           dict(dm=(0.0, inf)),
                           dict(hs=(Vs[1].h, Vs[0].h)),                      # a coarser level that is larger
                           dict(hs=(Vs[0].h, Vbad.h))):                      # a box that differs in one bit
                    rc, hh, ii, B0 = call(**kw)
                    rows = kw.get("rows", 4)
                    assert rc == 9004, (name, kw, rc)
                    assert np.array_equal(B0, b), (name, kw)                  # B is never cleared
                    if kw.get("nl", 2) >= 1:                                  # hist is (nlevels, rows, 6) to the call
                        flat = hh.reshape(-1)
                        assert not ii.any() and not flat[:2 * rows * 6].any() and np.isnan(flat[2 * rows * 6:]).all(), (name, kw)
                    else:
                        assert (ii == FILL).all() and np.isnan(hh).all(), (name, kw)
                for kw in (dict(hs=(Vs[0].h, None)), dict(hs=(None, Vs[1].h)), dict(harr=False), dict(B=False),
                           dict(hist=False), dict(info=False), dict(per=(False, True, True)), dict(per=(True, False, True)),
                           dict(per=(True, True, False))):
                    assert call(**kw)[0] == 9002, (name, kw)
        finally:
            L.ndsm_hip_device_free(dB)
        for kw in (dict(niter_max=[1, 2, 3]), dict(dt0=[1e-3]), dict(niter_max=[2, 0])):
            with pytest.raises(ValueError):
                Vs[0].optimize_cascade(Vs[1:], b, start="given", **kw)
        with pytest.raises(ValueError):
            Vs[0].optimize_cascade([Vbad], b, start="given")
        with pytest.raises(ValueError):
            Vs[1].optimize_cascade([Vs[0]], np.zeros((3,) + C.shape_of(meshes[1])), start="given")
    finally:
        for V in Vs + [Vbad]:
            V.close()


def test_other_entries_of_the_handles_are_untouched(hip):
    """solve() and optimize() give the same bits on every level's handle before and after a cascade"""
    meshes = level_meshes("uniform", [[12, 10, 9], [6, 5, 5]])
    b = field(meshes[0])
    Vs = handles(meshes)

    def others():
        out = []
        for V, m in zip(Vs, meshes):
            f = field(m)
            out += [np.asarray(v) for v in V.solve(f)]
            out += [np.asarray(v) for v in V.optimize(f, start="potential", niter_max=3, check=2)[:3]]
        return out
    try:
        before = others()
        for start in ("given", "potential"):
            Vs[0].optimize_cascade(Vs[1:], b, w=weight("cosine", meshes[0], b.shape[1:]), start=start, niter_max=3, check=2)
            after = others()
            assert len(before) == len(after)
            for x, y in zip(before, after):
                assert x.shape == y.shape and x.tobytes() == y.tobytes()
    finally:
        for V in Vs:
            V.close()
