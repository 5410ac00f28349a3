"""GPU tests of the optimization method with a measurement term and a freed lower face (csrc/optimize_obs.hip,
vecpot_optimize_obs) against its numpy model (tests/optimize_obs_model.py), bit for bit: the field as uint64, every
history row, info.  The model restates the kernels' expressions and the reduction's partition; nothing here is taken
from the device code's results."""
import ctypes

import numpy as np
import pytest

import optimize_model as M
import optimize_obs_model as O
from device_arena import Arena, LibTransport, slot
from golden_inputs import aniso_mesh, uniform_mesh

pytestmark = pytest.mark.gpu

_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
IDS = lambda s: "x".join(map(str, s))   # noqa: E731
FILL = 7

# 4x4x4: a free patch of 2 x 2 nodes whose one-sided z row reaches k = 2, next to the top face; 4x4x5, 5x7x4: one axis
# longer; 33x22x27: the suite's anisotropic shape; 513x4x4: three points per reduction thread, a row wider than any
# block; 5x46x46: 2116 rows on 2048 blocks; 65x9x5: one more than a multiple of the force pass's 64 x 4 x 1 block
SHAPES = ([4, 4, 4], [4, 4, 5], [5, 7, 4], [33, 22, 27], [513, 4, 4], [5, 46, 46], [65, 9, 5])
CASES = [("uniform", s) for s in SHAPES] + [("aniso", [33, 22, 27]), ("aniso", [5, 7, 4])]
MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
# (free, nu, wm, w): both values of each, every pair of free and nu, a NULL and a given array on either side of each
CONFIGS = [(1, 0.1, "smooth", "nonsep"), (1, 0.1, "none", "none"), (1, 0.0, "smooth", "none"), (1, 0.0, "none", "nonsep"),
           (0, 0.1, "smooth", "nonsep"), (0, 0.1, "none", "none"), (0, 0.0, "smooth", "none")]


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def unit(mesh):
    u = [(q - q[0]) / (q[-1] - q[0]) for q in mesh]
    return np.meshgrid(u[2], u[1], u[0], indexing="ij")


def field(mesh):
    """the ABC field with an interior bump: not force-free, not solenoidal, nowhere zero"""
    return M.perturbed_abc(mesh)[1]


def observation(mesh, b):
    """the lower face of b moved by a smooth pattern of height 0.1, another one per component"""
    _, Y, X = unit(mesh)
    Y, X = Y[0], X[0]
    return b[:, 0] + 0.1 * np.array([np.cos(3.0 * X + Y), np.sin(2.0 * Y - X + 0.3), 0.5 - X * Y])


def weight(kind, mesh):
    if kind == "none":
        return None
    Z, Y, X = unit(mesh)
    return 1.0 + 0.8 * np.sin(3.0 * X + 0.5 + Y * Z) * np.cos(2.0 * Y) + 0.5 * Z * X      # not a product of 1-D factors


def confidence(kind, mesh):
    """wm: None, a smooth non-constant one per component, or that with zeros - whole rows, a column, single pixels"""
    if kind == "none":
        return None
    _, Y, X = unit(mesh)
    Y, X = Y[0], X[0]
    wm = np.array([0.3 + 0.2 * np.sin(2.0 * X + Y), 0.25 + 0.2 * X * Y, 1.0 - 0.3 * np.cos(X - 2.0 * Y)])
    if kind == "zeros":
        wm[0, 1, :] = 0.0
        wm[1, :, 2] = 0.0
        wm[:, 2, 1] = 0.0
        wm[2, -2, -2] = 0.0
    return wm


def same(got, want, what):
    """(B, hist, info) of the device against the model's, bit for bit"""
    gB, gh, gi = got
    wB, wh, wi = want
    assert gi == wi, (what, gi, wi, gh, wh)
    assert gh.shape == wh.shape and gh.tobytes() == wh.tobytes(), (what, gh, wh)
    assert gB.shape == wB.shape, what
    bad = gB.view(np.uint64) != wB.view(np.uint64)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(gB - wB).max()))


@pytest.mark.parametrize("mname,ns", CASES, ids=[m + "-" + IDS(s) for m, s in CASES])
def test_driver_equals_the_model(hip, mname, ns):
    """after 1, 2 and 7 tries, the face held and freed, nu 0 and 0.1, wm NULL and non-constant, w NULL and
    non-separable: the field, the history and info of the host entry are the model's; 1 and 2 accepted tries leave the
    current field in either buffer.  Two calls give the same bits, and so does another check interval"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b = field(mesh)
    bobs = observation(mesh, b)
    V = ndsm_amd.VecPot(*mesh)
    try:
        parities = set()
        for free, nu, wmk, wk in CONFIGS:
            w, wm = weight(wk, mesh), confidence(wmk, mesh)
            for n in (1, 2, 7):
                what = "%s %s free %d nu %g wm %s w %s, %d tries" % (mname, ns, free, nu, wmk, wk, n)
                kw = dict(bobs=bobs, wm=wm, nu=nu, free=free, w=w, niter_max=n, check=1, tol=0.0)
                wB, wh, wi, _ = O.run(mesh, b, **kw)
                ierr, B, hist, info = V.optimize_obs(b, start="given", **kw)
                assert ierr == 0, what
                same((B, hist, info), (wB, wh, wi), what)
                assert info == (n + 1, n, 0) and np.isfinite(hist).all() and hist.shape == (n + 1, 7), (what, hist)
                assert np.all(hist[:, 1] == (hist[:, 2] + hist[:, 3]) + nu * hist[:, 4]), what
                moved = not np.array_equal(B[:, 0, 1:-1, 1:-1], b[:, 0, 1:-1, 1:-1])
                assert moved == (free == 1 and hist[-1, 6] > 0), what
                parities.add(int(hist[-1, 6]) % 2)
                if n == 7:
                    again = V.optimize_obs(b, start="given", **kw)
                    same(again[1:], (B, hist, info), what + ", second call")
                    kw3 = dict(kw, check=3)
                    _, B3, hist3, info3 = V.optimize_obs(b, start="given", **kw3)
                    same((B3, hist3, info3), O.run(mesh, b, **kw3)[:3], what + ", check 3")
                    assert info3 == (4, 7, 0) and np.array_equal(B3.view(np.uint64), B.view(np.uint64)), what
                    assert hist3[-1].tobytes() == hist[-1].tobytes()
        assert parities == {0, 1}
    finally:
        V.close()


@pytest.mark.parametrize("mname,ns", [("uniform", [4, 4, 4]), ("aniso", [33, 22, 27]), ("uniform", [513, 4, 4])],
                         ids=["uniform-4x4x4", "aniso-33x22x27", "uniform-513x4x4"])
def test_held_face_without_the_term_is_optimize(hip, mname, ns):
    """the anchor: free = 0 with nu = 0 is ndsm_hip_vecpot_optimize on the same input - B bitwise, info, and the
    columns the two histories share - whatever Bobs and wm hold; L_m is still reported"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b = field(mesh)
    bobs = observation(mesh, b)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for wk in ("none", "nonsep"):
            w = weight(wk, mesh)
            for kw in (dict(niter_max=7, check=3, tol=0.0), dict(niter_max=12, check=12, tol=0.0, dt0=16.0 * min(M.spacing(mesh)) ** 2)):
                _, B0, h0, i0 = V.optimize(b, w=w, start="given", **kw)
                for wmk in ("none", "smooth"):
                    _, B, h, i = V.optimize_obs(b, bobs=bobs, wm=confidence(wmk, mesh), nu=0.0, free=False, w=w,
                                                start="given", **kw)
                    what = (mname, ns, wk, wmk, kw)
                    assert i == i0 and np.array_equal(B.view(np.uint64), B0.view(np.uint64)), what
                    assert h[:, [0, 1, 2, 3, 5, 6]].tobytes() == h0.tobytes(), (what, h, h0)
                    assert np.all(h[:, 4] == h[0, 4]) and h[0, 4] > 0.0, what
    finally:
        V.close()


@pytest.mark.parametrize("mname,ns", [("uniform", [5, 7, 4]), ("aniso", [33, 22, 27]), ("uniform", [513, 4, 4])],
                         ids=["uniform-5x7x4", "aniso-33x22x27", "uniform-513x4x4"])
def test_rejections_stop_rules_and_zero_confidence(hip, mname, ns):
    """a first step 16 times too large (rejections, then acceptances) and one of 1e300 (inf and NaN in L_T, L_m
    included: rejections, then dt_min); the three stop rules and a history that runs out of rows; a wm with zeros"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b = field(mesh)
    bobs = observation(mesh, b)
    h2 = min(M.spacing(mesh)) ** 2
    V = ndsm_amd.VecPot(*mesh)
    try:
        for wk, wmk in (("none", "smooth"), ("nonsep", "zeros")):
            w, wm = weight(wk, mesh), confidence(wmk, mesh)
            for kw in (dict(niter_max=12, check=12, tol=0.0, dt0=16.0 * h2),                # rejected, then accepted
                       dict(niter_max=11, check=4, tol=0.0, dt0=3.0 * h2, hist_rows=3),   # rows run out; a short tail
                       dict(niter_max=50, check=5, tol=0.999),                              # tol at the first check
                       dict(niter_max=50, check=5, dt0=100.0, dt_min=60.0),                 # dt_min after one rejection
                       dict(niter_max=50, check=5, dt0=1.0, dt_min=2.0),                    # dt_min before any try
                       dict(niter_max=40, check=40, tol=0.0, dt0=1e300)):                   # overflow, then dt_min
                what = "%s %s w %s wm %s %s" % (mname, ns, wk, wmk, kw)
                want = O.run(mesh, b, bobs=bobs, wm=wm, nu=0.1, free=1, w=w, **kw)
                ierr, B, hist, info = V.optimize_obs(b, bobs=bobs, wm=wm, nu=0.1, free=True, w=w, start="given", **kw)
                assert ierr == 0
                same((B, hist, info), want[:3], what)
            _, B, hist, info = V.optimize_obs(b, bobs=bobs, wm=wm, nu=0.1, w=w, start="given", niter_max=12, check=12,
                                              tol=0.0, dt0=16.0 * h2)
            assert info == (2, 12, 0) and 0 < hist[1, 6] < 12, hist                 # both rejections and acceptances
            _, B, hist, info = V.optimize_obs(b, bobs=bobs, wm=wm, nu=0.1, w=w, start="given", niter_max=40, check=40,
                                              tol=0.0, dt0=1e300)
            assert info[2] == 2 and hist[-1, 6] == 0 and np.array_equal(B.view(np.uint64), b.view(np.uint64)), hist
        _, B, hist, info = V.optimize_obs(b, bobs=bobs, nu=0.1, start="given", niter_max=50, check=5, tol=0.999)
        assert info == (2, 5, 1)
        # bobs = None: the observation is the lower face of b, L_m starts at 0
        want = O.run(mesh, b, nu=0.1, niter_max=3, check=1, tol=0.0)
        _, B, hist, info = V.optimize_obs(b, nu=0.1, start="given", niter_max=3, check=1, tol=0.0)
        same((B, hist, info), want[:3], "bobs None")
        assert hist[0, 4] == 0.0 and hist[-1, 4] > 0.0
    finally:
        V.close()


def options(V):
    return V._options(10000, 1024, 1e-13, 1e-10, 5, False, False, False)


@pytest.mark.parametrize("mname,ns", [("uniform", [4, 4, 4]), ("aniso", [5, 7, 4]), ("aniso", [33, 22, 27])],
                         ids=["uniform-4x4x4", "aniso-5x7x4", "aniso-33x22x27"])
def test_host_entry_device_entry_and_offset_arrays(hip, mname, ns):
    """ndsm_hip_vecpot_optimize_obs = ndsm_hip_vecpot_optimize_obs_device on arrays of their own = the same on views
    into one larger allocation (8 mod 16, NaN bands beside B, w, Bobs and wm): B comes out, the others are read only,
    nothing else changes; 2 and 3 tries, so that the result is copied into the caller's array once and lies there
    once"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b = field(mesh)
    bobs = observation(mesh, b)
    h2 = min(M.spacing(mesh)) ** 2
    V = ndsm_amd.VecPot(*mesh)
    L = V.L
    try:
        for wk, wmk in (("none", "none"), ("nonsep", "smooth")):
            w, wm = weight(wk, mesh), confidence(wmk, mesh)
            for n in (2, 3):
                args = (0.1, 1, 1, n, 2, 0.0, 0.1 * h2, 1e-7 * h2)
                want = O.run(mesh, b, bobs=bobs, wm=wm, nu=0.1, free=1, w=w, niter_max=n, check=2, tol=0.0,
                             dt0=0.1 * h2, dt_min=1e-7 * h2, hist_rows=4)
                io, ro = options(V)
                B = b.reshape(-1).copy()
                ins = [None if a is None else a.reshape(-1).copy() for a in (w, bobs, wm)]
                hist, info = np.full((4, 7), np.nan), np.full(3, FILL, dtype=np.intc)
                rc = L.ndsm_hip_vecpot_optimize_obs(V.h, io.ctypes.data_as(_ip), ro.ctypes.data_as(_dp), B.ctypes.data,
                                                    *[None if a is None else a.ctypes.data for a in ins], *args,
                                                    hist.ctypes.data, 4, info.ctypes.data)
                assert rc == 0, hip.last_error(L)
                for a, k in zip(ins, (w, bobs, wm)):
                    assert a is None or np.array_equal(a, k.reshape(-1))
                rows = int(info[0])
                assert np.isnan(hist[rows:]).all()                   # rows past the ones written are left alone
                same((B.reshape(b.shape), hist[:rows], tuple(int(v) for v in info)), want[:3], "host entry")
                for plain in (False, True):
                    slots = [slot("B", b.reshape(-1), output=True, field=True)]
                    if w is not None:
                        slots.append(slot("w", w.reshape(-1), field=True))
                    slots.append(slot("Bobs", bobs.reshape(-1), field=True))
                    if wm is not None:
                        slots.append(slot("wm", wm.reshape(-1), field=True))
                    io_d, ro_d = options(V)
                    hist_d, info_d = np.full((4, 7), np.nan), np.full(3, FILL, dtype=np.intc)
                    R = Arena(LibTransport(L), slots, plain=plain)

                    def call(dB, *rest):
                        it = iter(rest)
                        dw = None if w is None else next(it)
                        dbobs = next(it)
                        dwm = None if wm is None else next(it)
                        return L.ndsm_hip_vecpot_optimize_obs_device(
                            V.h, io_d.ctypes.data_as(_ip), ro_d.ctypes.data_as(_dp), dB, dw, dbobs, dwm, *args,
                            hist_d.ctypes.data, 4, info_d.ctypes.data)
                    got = R.run(call)
                    what = "%s %s w %s wm %s %d tries plain %s" % (mname, ns, wk, wmk, n, plain)
                    assert R.rc == 0, (what, hip.last_error(L))
                    assert np.array_equal(got[0].view(np.uint64), B.view(np.uint64)), what
                    assert hist_d.tobytes() == hist.tobytes() and info_d.tobytes() == info.tobytes(), what
                    assert np.array_equal(io_d, io), what
    finally:
        V.close()


@pytest.mark.parametrize("mname,ns", [("uniform", [12, 10, 9]), ("aniso", [20, 17, 23])], ids=["uniform-12x10x9", "aniso-20x17x23"])
def test_potential_start_is_the_hand_built_chain(hip, mname, ns):
    """start = "potential" equals: the potential field of b's B.n by the device entry of solve(), the k = 0 plane of b
    - not of Bobs - put over it, then start = "given"; the rim and the five other faces are that start field's"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b = field(mesh)
    bobs = observation(mesh, b)
    wm = confidence("smooth", mesh)
    V = ndsm_amd.VecPot(*mesh)
    try:
        ierr_s, _, bp = V.solve(b, device=True)
        fail = int(V.last_ioptc[V.L.get_iopt_fail3d()])
        b0 = bp.copy()
        b0[:, 0] = b[:, 0]
        for w in (None, weight("nonsep", mesh)):
            for device in (False, True):
                kw = dict(bobs=bobs, wm=wm, nu=0.1, w=w, niter_max=3, check=2, tol=0.0)
                ierr_g, Bg, hist_g, info_g = V.optimize_obs(b0, start="given", **kw)
                ierr_p, Bp, hist_p, info_p = V.optimize_obs(b, start="potential", device=device, **kw)
                same((Bp, hist_p, info_p), (Bg, hist_g, info_g), "potential start, device %s" % device)
                assert ierr_g == 0 and ierr_p == (1 if ierr_s != 0 or fail != 0 else 0)
                held = np.ones(b.shape[1:], dtype=bool)
                held[:-1, 1:-1, 1:-1] = False
                assert np.array_equal(Bp[:, held].view(np.uint64), b0[:, held].view(np.uint64))
                assert not np.array_equal(Bp[:, 0, 1:-1, 1:-1], b[:, 0, 1:-1, 1:-1])
        want = O.run(mesh, b0, bobs=bobs, wm=wm, nu=0.1, niter_max=3, check=2, tol=0.0)
        got = V.optimize_obs(b, bobs=bobs, wm=wm, nu=0.1, start="potential", niter_max=3, check=2, tol=0.0)
        same(got[1:], want[:3], "potential start, model")
    finally:
        V.close()


def test_argument_errors_of_the_c_entries(hip):
    import ndsm_amd
    mesh = uniform_mesh([5, 7, 4])
    b = field(mesh)
    bobs = np.ascontiguousarray(observation(mesh, b))
    V = ndsm_amd.VecPot(*mesh)
    L = V.L
    nan, inf = float("nan"), float("inf")
    try:
        dB, dO = ctypes.c_void_p(), ctypes.c_void_p()
        assert L.ndsm_hip_device_alloc(b.nbytes, ctypes.byref(dB)) == 0
        assert L.ndsm_hip_device_alloc(bobs.nbytes, ctypes.byref(dO)) == 0
        try:
            assert L.ndsm_hip_memcpy_h2d(dB, b.ctypes.data, b.nbytes) == 0
            assert L.ndsm_hip_memcpy_h2d(dO, bobs.ctypes.data, bobs.nbytes) == 0
            for name, pB, pO in (("ndsm_hip_vecpot_optimize_obs", ctypes.c_void_p(b.ctypes.data),
                                  ctypes.c_void_p(bobs.ctypes.data)),
                                 ("ndsm_hip_vecpot_optimize_obs_device", dB, dO)):
                fn = getattr(L, name)
                dev = name.endswith("_device")

                #                                     nu free start niter check tol dt0 dt_min
                def call(h=V.h, B=pB, Bo=pO, args=(0.1, 0, 1, 3, 1, 0.0, 1e-3, 0.0), rows=4, hist=True, info=True):
                    io, ro = options(V)
                    hh, ii = np.full((4, 7), nan), np.full(3, FILL, dtype=np.intc)
                    rc = fn(h, io.ctypes.data_as(_ip), ro.ctypes.data_as(_dp), B, None, Bo, None, *args,
                            hh.ctypes.data if hist else None, rows, ii.ctypes.data if info else None)
                    return rc, hh, ii
                rc, hh, ii = call()
                assert rc == 0 and tuple(ii) == (4, 3, 0) and np.isfinite(hh).all()
                keep = np.empty_like(b)
                if dev:
                    assert L.ndsm_hip_memcpy_d2h(keep.ctypes.data, dB, b.nbytes) == 0
                else:
                    keep[:] = b
                good = (0.1, 0, 1, 3, 1, 0.0, 1e-3, 0.0)
                for pos, bad in ((0, -1e-9), (0, nan), (0, inf), (0, -inf), (1, 2), (1, -1), (2, 2), (2, -1), (3, 0),
                                 (4, 0), (5, -1e-9), (5, nan), (5, inf), (6, 0.0), (6, -1.0), (6, inf), (6, nan),
                                 (7, -1.0), (7, nan), (7, inf)):
                    args = good[:pos] + (bad,) + good[pos + 1:]
                    rc, hh, ii = call(args=args)
                    assert rc == 9004 and not ii.any() and not hh.any(), (name, args, rc)
                rc, hh, ii = call(rows=1)
                assert rc == 9004 and not ii.any() and not hh[0].any() and np.isnan(hh[1:]).all()
                assert call(h=None)[0] == 9002 and call(B=None)[0] == 9002 and call(Bo=None)[0] == 9002
                assert call(hist=False)[0] == 9002 and call(info=False)[0] == 9002
                back = b
                if dev:
                    back = np.empty_like(b)
                    assert L.ndsm_hip_memcpy_d2h(back.ctypes.data, dB, b.nbytes) == 0
                assert np.array_equal(back.view(np.uint64), keep.view(np.uint64))       # a failed call never clears B
        finally:
            L.ndsm_hip_device_free(dB)
            L.ndsm_hip_device_free(dO)
    finally:
        V.close()


def test_other_entries_of_the_handle_are_untouched(hip):
    """solve(), optimize() and helicity() give the same bits before and after an optimize_obs() on one handle"""
    import ndsm_amd
    mesh = uniform_mesh([12, 10, 9])
    b = field(mesh)
    bobs = observation(mesh, b)
    V = ndsm_amd.VecPot(*mesh)

    def others():
        s = V.solve(b)
        o = V.optimize(b, start="given", niter_max=3, check=2)
        h = V.helicity(b)
        return ([np.asarray(v) for v in s] + [np.asarray(v) for v in o[:3]] +
                [np.asarray(v, dtype=np.float64) for v in h[:10]])
    try:
        before = others()
        for start in ("given", "potential"):
            V.optimize_obs(b, bobs=bobs, wm=confidence("smooth", mesh), nu=0.1, w=weight("nonsep", mesh), start=start,
                           niter_max=3, check=2)
            after = others()
            assert len(before) == len(after)
            for x, y in zip(before, after):
                assert x.shape == y.shape and x.tobytes() == y.tobytes()
    finally:
        V.close()
