"""GPU tests of the confidence-weighted restriction (csrc/resample.hip, resample_weighted_k) and of the cascade of the
measurement fit (vecpot_optimize_cascade with an observation) against their model (tests/obs_cascade_model.py) and
against the chain of public calls, bit for bit: fields as uint64, every history row, info.  The model restates the rule
in Python loops and strings optimize_obs_model.run calls together; nothing here is taken from the device code's
results.  Shapes are written nx x ny x nz as in the library."""
import ctypes
import math

import numpy as np
import pytest

import cascade_model as C
import obs_cascade_model as OC
import optimize_model as M
from device_arena import Arena, LibTransport, slot
from golden_inputs import aniso_mesh, uniform_mesh

pytestmark = pytest.mark.gpu

_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
IDS = lambda s: "x".join(map(str, s))   # noqa: E731
FILL = 7

# source -> destination, nx x ny x nz.  4x4x4 -> itself: every node a copy; 5x7x4 -> 3x4x4: a 2:1 axis, a 7 -> 4 axis that
# is not nested, an axis kept; 33x22x27 onto its (n + 1) // 2 shape and onto one with ratios that are no whole numbers
# (more than three taps per axis); 513 -> 257: more than one block along x; 5x46x46 -> 3x23x23: one past the block
# along y, 69 (z, component) planes; two planes
SHAPES = [([4, 4, 4], [4, 4, 4]), ([5, 7, 4], [3, 4, 4]), ([33, 22, 27], [17, 11, 14]), ([33, 22, 27], [13, 9, 10]),
          ([513, 4, 4], [257, 4, 4]), ([5, 46, 46], [3, 23, 23]), ([9, 6, 1], [5, 4, 1]), ([65, 9, 1], [33, 5, 1])]
KINDS = ("random", "zeros", "ones")
WEIGHTED_CASES = [(s, d, k) for s, d in SHAPES for k in KINDS]

LEVEL_SETS = ([[9, 9, 7], [5, 5, 4]], [[12, 10, 9], [6, 5, 5]], [[17, 13, 13], [9, 7, 7], [5, 4, 4]],
              [[65, 9, 5], [33, 5, 4]])
CASCADE_CASES = [("uniform", s) for s in LEVEL_SETS] + [("aniso", LEVEL_SETS[1])]
MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
# (free, nu, wm, w): a freed and a held face with and without the term, a confidence and a weight or neither
SETTINGS = [(1, 0.1, "nonconst", "nonsep"), (1, 0.0, None, None), (0, 0.1, "nonconst", None), (0, 0.0, None, "nonsep")]


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
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(ncomp,) + tuple(shape)) + 1.5


def confidence(kind, src, dst, ncomp, seed=2):
    """(ncomp, nz, ny, nx).  "random": in (0, 1]; "zeros": the same with a zero row, a zero column and a zero block wider
    than a hat on every axis - destination nodes whose taps are all zero take the den = 0 branch; "ones\""""
    shape = tuple(src[::-1])
    if kind == "ones":
        return np.ones((ncomp,) + shape)
    w = 1.0 - np.random.default_rng(seed).uniform(0.0, 1.0, size=(ncomp,) + shape)
    if kind == "zeros":
        nz, ny, nx = shape
        w[:, :, ny // 2, :] = 0.0
        w[:, :, :, (2 * nx) // 3] = 0.0
        ext = [min(ns, 2 * math.ceil((ns - 1) / max(nd - 1, 1)) + 3) for ns, nd in zip(src[::-1], dst[::-1])]
        w[:, :ext[0], 1:1 + ext[1], 1:1 + ext[2]] = 0.0
    return w


def bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    assert not bad.any(), (what, int(bad.sum()), float(np.nanmax(np.abs(got - want))))


def level_meshes(mname, sets):
    fine = MESHES[mname](sets[0])
    return [fine] + [[np.linspace(q[0], q[-1], n) for q, n in zip(fine, s)] for s in sets[1:]]


def unit(mesh):
    u = [(q - q[0]) / (q[-1] - q[0]) for q in mesh]
    return np.meshgrid(u[2], u[1], u[0], indexing="ij")


def field(mesh):
    return M.perturbed_abc(mesh)[1]


def observation(mesh, kind):
    """(bobs, wm): the exact lower face plus a smooth misfit; a confidence that differs per pixel and component"""
    Z, Y, X = unit(mesh)
    bobs = M.perturbed_abc(mesh)[0][:, 0] + 0.1 * np.array([np.cos(3.0 * X[0]), np.sin(2.0 * Y[0]), X[0] * Y[0]])
    wm = None if kind is None else np.array([0.3 + 0.2 * X[0], 0.25 + 0.2 * Y[0], 1.0 - 0.3 * X[0] * Y[0]])
    return bobs, wm


def weight(kind, mesh):
    if kind is None:
        return None
    Z, Y, X = unit(mesh)
    return 1.0 + 0.8 * np.sin(3.0 * X + 0.5 + Y * Z) * np.cos(2.0 * Y) + 0.5 * Z * X      # not a product of 1-D factors


def same(got, want, what):
    """(B, [hist], [info]) of the device against the model's, bit for bit"""
    gB, gh, gi = got
    wB, wh, wi = want
    assert list(gi) == list(wi), (what, gi, wi)
    for l, (a, b) in enumerate(zip(gh, wh)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, l, a, b)
    bits(gB, wB, what)


def handles(meshes):
    import ndsm_amd
    return [ndsm_amd.VecPot(*m) for m in meshes]


@pytest.mark.parametrize("src,dst,kind", WEIGHTED_CASES, ids=["%s-%s-%s" % (IDS(s), IDS(d), k) for s, d, k in WEIGHTED_CASES])
def test_weighted_restriction_equals_the_model(hip, src, dst, kind):
    """three components and one (the first of the three: the components do not see each other), the host and the device
    entry"""
    import ndsm_amd
    a, w = rough(src[::-1], 3), confidence(kind, src, dst, 3)
    want, wwant = OC.resample_weighted(a, w, tuple(dst[::-1]))
    if kind == "zeros":
        assert (wwant == 0.0).any() and (wwant > 0.0).any()
    if kind == "ones":
        assert (wwant == 1.0).all()
    for device in (False, True):
        what = "%s -> %s %s device %s" % (src, dst, kind, device)
        got, wgot = ndsm_amd.resample_weighted(a, w, tuple(dst[::-1]), device=device)
        bits(got, want, what)
        bits(wgot, wwant, what + ", confidence")
        got, wgot = ndsm_amd.resample_weighted(a[0], w[0], tuple(dst[::-1]), device=device)
        bits(got, want[0], what + ", one component")
        bits(wgot, wwant[0], what + ", one component, confidence")


def test_weighted_restriction_properties_on_the_device(hip):
    """ns = nd returns both arrays; a power of two on the confidence; NaN inside both sources does not reach a face"""
    import ndsm_amd
    a, w = rough((27, 22, 33), 3), confidence("random", [33, 22, 27], [33, 22, 27], 3)
    d, wd = ndsm_amd.resample_weighted(a, w, (27, 22, 33), device=True)
    bits(d, a, "identity")
    bits(wd, w, "identity, confidence")
    d, wd = ndsm_amd.resample_weighted(a, w, (14, 11, 17))
    ds, wds = ndsm_amd.resample_weighted(a, 0.125 * w, (14, 11, 17), device=True)
    bits(ds, d, "scaled confidence")
    bits(wds, 0.125 * wd, "scaled confidence, confidence")
    ha, hw = a.copy(), w.copy()
    ha[:, 1:-1, 1:-1, 1:-1] = np.nan
    hw[:, 1:-1, 1:-1, 1:-1] = np.nan
    for dst in ((14, 11, 17), (4, 4, 4)):
        f = C.faces(dst)
        clean, got = ndsm_amd.resample_weighted(a, w, dst), ndsm_amd.resample_weighted(ha, hw, dst, device=True)
        for x, y in zip(got, clean):
            assert np.isfinite(x[:, f]).all(), dst
            bits(x[:, f], y[:, f], "faces %s" % (dst,))


@pytest.mark.parametrize("src,dst", [([33, 22, 27], [13, 9, 10]), ([9, 6, 1], [5, 4, 1])], ids=["volume", "plane"])
def test_weighted_device_entry_on_offset_arrays(hip, src, dst):
    """views into one larger allocation, 8 mod 16, NaN bands beside all four arrays: the result is that of arrays of
    their own, the sources and every guard byte stay as they were"""
    import ndsm_amd
    L = ndsm_amd.load_library()
    a, w = rough(src[::-1], 3), confidence("zeros", src, dst, 3)
    want, wwant = OC.resample_weighted(a, w, tuple(dst[::-1]))
    ns3, nd3 = np.array(src, dtype=np.intc), np.array(dst, dtype=np.intc)
    for plain in (False, True):
        R = Arena(LibTransport(L), [slot("src", a.reshape(-1), field=True), slot("wsrc", w.reshape(-1), field=True),
                                    slot("dst", np.full(want.size, 3.25), output=True, field=True),
                                    slot("wdst", np.full(want.size, -1.5), output=True, field=True)], plain=plain)
        got = R.run(lambda ds, dw, dd, dwd: L.ndsm_hip_resample_weighted_device(
            ns3.ctypes.data_as(_ip), nd3.ctypes.data_as(_ip), 3, ds, dw, dd, dwd))
        assert R.rc == 0, hip.last_error(L)
        bits(got[2].reshape(want.shape), want, "plain %s" % plain)
        bits(got[3].reshape(want.shape), wwant, "plain %s, confidence" % plain)


def test_weighted_argument_errors(hip):
    import ndsm_amd
    L = ndsm_amd.load_library()
    a, w = rough((4, 5, 6), 2), confidence("random", [6, 5, 4], [3, 3, 4], 2)
    for name in ("ndsm_hip_resample_weighted", "ndsm_hip_resample_weighted_device"):
        fn = getattr(L, name)
        dev = name.endswith("_device")
        out, wout = np.full(2 * a.size, 3.25), np.full(2 * a.size, -1.5)
        host = [a, w, out, wout]
        ptrs = [ctypes.c_void_p() for _ in host]
        try:
            for p, h in zip(ptrs, host):
                assert L.ndsm_hip_device_alloc(h.nbytes, ctypes.byref(p)) == 0
                assert L.ndsm_hip_memcpy_h2d(p, h.ctypes.data, h.nbytes) == 0

            def call(ns=(6, 5, 4), nd=(3, 3, 4), ncomp=2, arrays=(True,) * 4, shapes=(True, True)):
                s3, d3 = np.array(ns, dtype=np.intc), np.array(nd, dtype=np.intc)
                args = [(p if dev else ctypes.c_void_p(h.ctypes.data)) if on else None for p, h, on in zip(ptrs, host, arrays)]
                return fn(s3.ctypes.data_as(_ip) if shapes[0] else None, d3.ctypes.data_as(_ip) if shapes[1] else None,
                          ncomp, *args)
            for kw in (dict(ncomp=0), dict(ncomp=-1), dict(nd=(7, 3, 4)), dict(nd=(3, 3, 5)), dict(nd=(1, 3, 4)),
                       dict(nd=(3, 0, 4)), dict(ns=(6, 5, 1)), dict(ns=(6, 5, 1), nd=(3, 3, 2)), dict(ns=(1, 5, 4))):
                assert call(**kw) == 9004, (name, kw)
            for kw in [dict(arrays=tuple(i != k for i in range(4))) for k in range(4)] + [dict(shapes=(False, True)),
                                                                                          dict(shapes=(True, False))]:
                assert call(**kw) == 9002, (name, kw)
            for p, h, fill in ((ptrs[2], out, 3.25), (ptrs[3], wout, -1.5)):   # a failed call leaves dst and wdst as they were
                back = np.empty_like(h)
                assert L.ndsm_hip_memcpy_d2h(back.ctypes.data, p, h.nbytes) == 0
                assert (back == fill).all() and (h == fill).all()
            assert call() == 0 and call(ns=(6, 5, 1), nd=(3, 3, 1)) == 0
        finally:
            for p in ptrs:
                L.ndsm_hip_device_free(p)
    for bad in (dict(shape=(4, 5)), dict(shape=(9, 5, 6)), dict(shape=(4, 1, 6))):
        with pytest.raises(ValueError):
            ndsm_amd.resample_weighted(a, w, **bad)


@pytest.mark.parametrize("mname,sets", CASCADE_CASES, ids=[m + "-" + "-".join(IDS(s) for s in ss) for m, ss in CASCADE_CASES])
def test_cascade_equals_the_model(hip, mname, sets):
    """start given; 1, 2 and 7 tries from the finest level down, check 3; the host and the device entry.  The held nodes
    of the result are the input's"""
    meshes = level_meshes(mname, sets)
    b = field(meshes[0])
    nit = [1, 2, 7][:len(sets)]
    Vs = handles(meshes)
    try:
        for free, nu, wkind, wgt in SETTINGS:
            bobs, wm = observation(meshes[0], wkind)
            w = weight(wgt, meshes[0])
            wB, wh, wi = OC.cascade_obs(meshes, b, bobs, wm, nu, free, w, niter_max=nit, check=3, tol=0.0)[:3]
            for device in (False, True):
                what = "%s %s free %d nu %g wm %s w %s device %s" % (mname, sets, free, nu, wkind, wgt, device)
                ierr, B, hist, info = Vs[0].optimize_obs_cascade(Vs[1:], b, bobs=bobs, wm=wm, nu=nu, free=bool(free), w=w,
                                                                 start="given", niter_max=nit, check=3, tol=0.0,
                                                                 device=device)
                assert ierr == 0, what
                same((B, hist, info), (wB, wh, wi), what)
                held = OC.paste_mask(b.shape[1:], 3 if free else 1)
                bits(B[:, held], b[:, held], what + ", held nodes")
                assert [i[1] for i in info] == nit and all(np.isfinite(h).all() for h in hist), (what, info)
    finally:
        for V in Vs:
            V.close()


def test_cascade_with_a_confidence_that_has_holes(hip):
    """a zero block in wm wider than a coarse hat: coarse pixels nobody trusts (wm_l = 0, Bobs_l the plain average)"""
    meshes = level_meshes("uniform", LEVEL_SETS[2])
    b = field(meshes[0])
    bobs, wm = observation(meshes[0], "nonconst")
    wm[:, 2:12, 3:13] = 0.0
    want = OC.cascade_obs(meshes, b, bobs, wm, 0.1, 1, None, niter_max=[1, 2, 7], check=3, tol=0.0)
    assert (want[5][1][2] == 0.0).any() and (want[5][1][1] == 0.0).any()
    Vs = handles(meshes)
    try:
        ierr, B, hist, info = Vs[0].optimize_obs_cascade(Vs[1:], b, bobs=bobs, wm=wm, nu=0.1, start="given",
                                                         niter_max=[1, 2, 7], check=3, tol=0.0)
        assert ierr == 0
        same((B, hist, info), want[:3], "holes in wm")
    finally:
        for V in Vs:
            V.close()


def test_cascade_nu_per_level_and_a_level_that_stops_at_dt_min(hip):
    meshes = level_meshes("uniform", LEVEL_SETS[0])
    b = field(meshes[0])
    bobs, wm = observation(meshes[0], "nonconst")
    h2 = [min(M.spacing(m)) ** 2 for m in meshes]
    Vs = handles(meshes)
    try:
        # nu per level
        kw = dict(niter_max=[4, 5], check=2, tol=0.0)
        want = OC.cascade_obs(meshes, b, bobs, wm, [0.3, 0.02], 1, None, **kw)
        other = OC.cascade_obs(meshes, b, bobs, wm, [0.02, 0.3], 1, None, **kw)
        assert not np.array_equal(want[0], other[0])
        for device in (False, True):
            ierr, B, hist, info = Vs[0].optimize_obs_cascade(Vs[1:], b, bobs=bobs, wm=wm, nu=[0.3, 0.02], start="given",
                                                             device=device, **kw)
            assert ierr == 0
            same((B, hist, info), want[:3], "nu per level, device %s" % device)
            for l, nu in enumerate((0.3, 0.02)):
                assert np.all(hist[l][:, 1] == (hist[l][:, 2] + hist[l][:, 3]) + nu * hist[l][:, 4])
        # dt0 below dt_min on the coarse level only: one row, no try there, and the fine level runs
        kw = dict(niter_max=[4, 5], check=2, tol=0.0, dt0=[0.1 * h2[0], 1.0], dt_min=[1e-7 * h2[0], 2.0])
        want = OC.cascade_obs(meshes, b, bobs, wm, 0.1, 1, None, **kw)
        ierr, B, hist, info = Vs[0].optimize_obs_cascade(Vs[1:], b, bobs=bobs, wm=wm, nu=0.1, start="given", **kw)
        assert ierr == 0
        same((B, hist, info), want[:3], "dt_min on the coarse level")
        assert info[1] == (1, 0, 2) and info[0] == (3, 4, 0), info
    finally:
        for V in Vs:
            V.close()


def test_one_level_is_optimize_obs_itself(hip):
    import ndsm_amd
    mesh = uniform_mesh([12, 10, 9])
    b = field(mesh)
    bobs, wm = observation(mesh, "nonconst")
    w = weight("nonsep", mesh)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for start in ("given", "potential"):
            for device in (False, True):
                kw = dict(bobs=bobs, wm=wm, nu=0.1, free=True, w=w, start=start, niter_max=3, check=2, tol=0.0, device=device)
                one = V.optimize_obs(b, **kw)
                ierr, B, hist, info = V.optimize_obs_cascade([], b, **kw)
                assert ierr == one[0] and len(hist) == 1 and len(info) == 1
                same((B, hist, info), (one[1], [one[2]], [one[3]]), "one level, start %s device %s" % (start, device))
    finally:
        V.close()


def test_a_held_face_without_the_term_is_the_plain_cascade(hip):
    """free 0 with nu 0 is optimize_cascade bit for bit in B, info and the shared history columns, whatever bobs and wm
    hold"""
    meshes = level_meshes("aniso", LEVEL_SETS[2])
    b = field(meshes[0])
    w = weight("nonsep", meshes[0])
    junk = np.random.default_rng(9).uniform(-1e3, 1e3, size=(2, 3) + b.shape[2:])
    junk[1] = np.abs(junk[1])
    Vs = handles(meshes)
    try:
        for start in ("given", "potential"):
            for device in (False, True):
                kw = dict(w=w, start=start, niter_max=[2, 3, 4], check=2, tol=0.0, device=device)
                ierr0, B0, hist0, info0 = Vs[0].optimize_cascade(Vs[1:], b, **kw)
                for wm in (junk[1], None):
                    ierr, B, hist, info = Vs[0].optimize_obs_cascade(Vs[1:], b, bobs=junk[0], wm=wm, nu=0.0, free=False, **kw)
                    what = "start %s device %s" % (start, device)
                    assert ierr == ierr0, what
                    same((B, [h[:, [0, 1, 2, 3, 5, 6]].copy() for h in hist], info), (B0, hist0, info0), what)
    finally:
        for V in Vs:
            V.close()


@pytest.mark.parametrize("mname,sets", [("uniform", [[12, 10, 9], [6, 5, 5]]), ("aniso", [[17, 13, 13], [9, 7, 7], [5, 4, 4]])],
                         ids=["uniform-2", "aniso-3"])
def test_potential_start_is_the_chain_of_public_calls(hip, mname, sets):
    """resample_weighted of (bobs, wm) - resample (average) of bobs without wm - and resample (average) of b for the
    level data, optimize_obs(start = "potential") on the coarsest handle, then per finer level resample (linear), the
    paste done in numpy - the k = 0 plane of that level's average of b, with a freed face its rim only -,
    optimize_obs(start = "given")"""
    import ndsm_amd
    meshes = level_meshes(mname, sets)
    shapes = [C.shape_of(m) for m in meshes]
    b = field(meshes[0])
    nit = [2, 3, 4][:len(sets)]
    last = len(sets) - 1
    Vs = handles(meshes)
    try:
        for free, nu, wkind, wgt in SETTINGS[:3]:
            bobs, wm = observation(meshes[0], wkind)
            w = weight(wgt, meshes[0])
            G = [b] + [ndsm_amd.resample(b, s, mode="average") for s in shapes[1:]]
            W = [w] + [None if w is None else ndsm_amd.resample(w, s, mode="linear") for s in shapes[1:]]
            BO, WM = [bobs], [wm]
            for nz, ny, nx in shapes[1:]:
                if wm is None:
                    BO.append(ndsm_amd.resample(bobs[:, None], (1, ny, nx), mode="average")[:, 0])
                    WM.append(None)
                else:
                    d, wd = ndsm_amd.resample_weighted(bobs[:, None], wm[:, None], (1, ny, nx))
                    BO.append(d[:, 0])
                    WM.append(wd[:, 0])
            for device in (False, True):
                hist, info = [None] * len(sets), [None] * len(sets)
                kw = dict(free=bool(free), check=2, tol=0.0, device=device)
                ierr_c, cur, hist[last], info[last] = Vs[last].optimize_obs(
                    G[last], bobs=BO[last], wm=WM[last], nu=nu, w=W[last], start="potential", niter_max=nit[last], **kw)
                for l in range(last - 1, -1, -1):
                    s = ndsm_amd.resample(cur, shapes[l], mode="linear")
                    m = OC.paste_mask(shapes[l], 2 if free else 0)
                    s[:, m] = G[l][:, m]
                    rc, cur, hist[l], info[l] = Vs[l].optimize_obs(s, bobs=BO[l], wm=WM[l], nu=nu, w=W[l], start="given",
                                                                   niter_max=nit[l], **kw)
                    assert rc == 0
                ierr, B, gh, gi = Vs[0].optimize_obs_cascade(Vs[1:], b, bobs=bobs, wm=wm, nu=nu, w=w, start="potential",
                                                             niter_max=nit, **kw)
                what = "potential start, free %d nu %g device %s" % (free, nu, device)
                assert ierr == ierr_c, what                                    # the coarsest solve's flag is passed on
                same((B, gh, gi), (cur, hist, info), what)
                rim = OC.paste_mask(shapes[0], 2)
                bits(B[:, rim], b[:, rim], what + ", rim")
                assert np.array_equal(B[:, 0], b[:, 0]) == (not free) and not np.array_equal(B[:, -1], b[:, -1]), what
    finally:
        for V in Vs:
            V.close()


def options(V):
    return V._options(10000, 1024, 1e-13, 1e-10, 5, False, False, False)


def test_argument_errors_of_the_c_entries(hip):
    import ndsm_amd
    meshes = level_meshes("uniform", [[9, 9, 7], [5, 5, 4]])
    b = field(meshes[0])
    bobs, wm = observation(meshes[0], "nonconst")
    shifted = [q.copy() for q in meshes[1]]
    shifted[1][-1] = np.nextafter(shifted[1][-1], 2.0)                         # one bit off the box in y
    Vs = handles(meshes)
    Vbad = ndsm_amd.VecPot(*shifted)
    L = Vs[0].L
    nan, inf = float("nan"), float("inf")
    try:
        dev = [ctypes.c_void_p() for _ in range(3)]
        for p, h in zip(dev, (b, bobs, wm)):
            assert L.ndsm_hip_device_alloc(h.nbytes, ctypes.byref(p)) == 0
            assert L.ndsm_hip_memcpy_h2d(p, np.ascontiguousarray(h).ctypes.data, h.nbytes) == 0
        try:
            for name, host in (("ndsm_hip_vecpot_optimize_obs_cascade", True),
                               ("ndsm_hip_vecpot_optimize_obs_cascade_device", False)):
                fn = getattr(L, name)

                def call(hs=(Vs[0].h, Vs[1].h), nl=None, B=True, obs=True, nu=(0.1, 0.1), free=1, start=1, nit=(2, 3), check=2,
                         tol=0.0, d0=(1e-3, 1e-3), dm=(0.0, 0.0), rows=4, hist=True, info=True, per=(True,) * 4, harr=True):
                    nl = len(hs) if nl is None else nl
                    io, ro = options(Vs[0])
                    harray = (ctypes.c_void_p * max(len(hs), 1))(*hs)
                    u_a, n_a = np.array(nu, dtype=np.float64), np.array(nit, dtype=np.intc)
                    d_a, m_a = np.array(d0, dtype=np.float64), np.array(dm, dtype=np.float64)
                    hh, ii = np.full((2, 4, 7), nan), np.full((2, 3), FILL, dtype=np.intc)
                    B0 = b.copy()
                    assert L.ndsm_hip_memcpy_h2d(dev[0], B0.ctypes.data, B0.nbytes) == 0
                    pB, pO, pM = ((ctypes.c_void_p(v.ctypes.data) for v in (B0, bobs, wm)) if host else dev)
                    rc = fn(harray if harr else None, nl, io.ctypes.data_as(_ip), ro.ctypes.data_as(_dp), pB if B else None,
                            None, pO if obs else None, pM, u_a.ctypes.data if per[3] else None, free, start,
                            n_a.ctypes.data if per[0] else None, check, tol, d_a.ctypes.data if per[1] else None,
                            m_a.ctypes.data if per[2] else None, hh.ctypes.data if hist else None, rows,
                            ii.ctypes.data if info else None)
                    if not host:
                        assert L.ndsm_hip_memcpy_d2h(B0.ctypes.data, dev[0], B0.nbytes) == 0
                    return rc, hh, ii, B0
                rc, hh, ii, _ = call()
                assert rc == 0 and [tuple(r) for r in ii] == [(2, 2, 0), (3, 3, 0)] and np.isnan(hh[0, 2:]).all(), (rc, ii)
                for kw in (dict(free=2), dict(free=-1), dict(nu=(-0.1, 0.1)), dict(nu=(0.1, -1e-300)), dict(nu=(nan, 0.1)),
                           dict(nu=(0.1, inf)),
                           dict(nl=0), dict(nl=-1), dict(start=2), dict(start=-1), dict(nit=(2, 0)), dict(nit=(0, 3)),
                           dict(check=0), dict(rows=1), dict(tol=-1e-9), dict(tol=nan), dict(tol=inf), dict(d0=(1e-3, 0.0)),
                           dict(d0=(nan, 1e-3)), dict(d0=(1e-3, inf)), dict(dm=(0.0, -1.0)), dict(dm=(nan, 0.0)),
                           dict(dm=(0.0, inf)),
                           dict(hs=(Vs[1].h, Vs[0].h)),                      # a coarser level that is larger
                           dict(hs=(Vs[0].h, Vbad.h))):                      # a box that differs in one bit
                    rc, hh, ii, B0 = call(**kw)
                    rows = kw.get("rows", 4)
                    assert rc == 9004, (name, kw, rc)
                    assert np.array_equal(B0, b), (name, kw)                  # B is never cleared
                    if kw.get("nl", 2) >= 1:                                  # hist is (nlevels, rows, 7) to the call
                        flat = hh.reshape(-1)
                        assert not ii.any() and not flat[:2 * rows * 7].any() and np.isnan(flat[2 * rows * 7:]).all(), (name, kw)
                    else:
                        assert (ii == FILL).all() and np.isnan(hh).all(), (name, kw)
                for kw in (dict(obs=False), dict(per=(True, True, True, False)),
                           dict(hs=(Vs[0].h, None)), dict(hs=(None, Vs[1].h)), dict(harr=False), dict(B=False),
                           dict(hist=False), dict(info=False), dict(per=(False, True, True, True)),
                           dict(per=(True, False, True, True)), dict(per=(True, True, False, True))):
                    rc, hh, ii, B0 = call(**kw)
                    assert rc == 9002, (name, kw)
                    assert np.array_equal(B0, b), (name, kw)
                    if kw.get("info", True):
                        assert not ii.any(), (name, kw)
                    if kw.get("hist", True):
                        assert not hh.any(), (name, kw)
        finally:
            for p in dev:
                L.ndsm_hip_device_free(p)
        for kw in (dict(nu=[0.1]), dict(nu=[0.1, -0.1]), dict(free=2), dict(niter_max=[1, 2, 3])):
            with pytest.raises(ValueError):
                Vs[0].optimize_obs_cascade(Vs[1:], b, start="given", **kw)
        with pytest.raises(ValueError):
            Vs[0].optimize_obs_cascade([Vbad], b, start="given")
    finally:
        for V in Vs + [Vbad]:
            V.close()


def test_other_entries_are_untouched(hip):
    """solve(), optimize(), optimize_obs(), optimize_cascade() and resample() give the same bits before and after calls
    of the new entries"""
    import ndsm_amd
    meshes = level_meshes("uniform", [[12, 10, 9], [6, 5, 5]])
    b = field(meshes[0])
    bobs, wm = observation(meshes[0], "nonconst")
    w = weight("nonsep", meshes[0])
    Vs = handles(meshes)

    def others():
        out = []
        for V, m in zip(Vs, meshes):
            f = field(m)
            o, c = observation(m, "nonconst")
            out += [np.asarray(v) for v in V.solve(f)]
            out += [np.asarray(v) for v in V.optimize(f, start="potential", niter_max=3, check=2)[:3]]
            out += [np.asarray(v) for v in V.optimize_obs(f, bobs=o, wm=c, nu=0.1, start="potential", niter_max=3, check=2)[:3]]
        r = Vs[0].optimize_cascade(Vs[1:], b, w=w, start="potential", niter_max=3, check=2)
        out += [np.asarray(r[1])] + [np.asarray(h) for h in r[2]]
        out += [ndsm_amd.resample(b, C.shape_of(meshes[1]), mode=mode) for mode in C.MODES]
        out.append(ndsm_amd.resample(r[1], (17, 19, 23), mode="linear"))
        return out
    try:
        before = others()
        for start in ("given", "potential"):
            Vs[0].optimize_obs_cascade(Vs[1:], b, bobs=bobs, wm=wm, nu=0.1, w=w, start=start, niter_max=3, check=2)
            ndsm_amd.resample_weighted(bobs[:, None], wm[:, None], (1, 5, 6))
            after = others()
            assert len(before) == len(after)
            for x, y in zip(before, after):
                assert x.shape == y.shape and x.tobytes() == y.tobytes()
    finally:
        for V in Vs:
            V.close()
