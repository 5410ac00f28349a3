"""GPU tests of the optimization-method force-free solver (csrc/optimize.hip, vecpot_optimize) against its numpy model
(tests/optimize_model.py), bit for bit: the field as uint64, every history row, info.  The model restates the kernels'
expressions and the reduction's partition; nothing here is taken from the device code's results."""
import ctypes

import numpy as np
import pytest

import optimize_model as M
from device_arena import Arena, LibTransport, slot
from golden_inputs import aniso_mesh, uniform_mesh

pytestmark = pytest.mark.gpu

_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
IDS = lambda s: "x".join(map(str, s))   # noqa: E731
FILL = 7

# 4x4x4: an interior of 2^3 nodes, every Omega they use comes from one-sided rows; 4x4x5, 5x7x4: one axis longer;
# 33x22x27: the suite's anisotropic shape; 513x4x4: three points per reduction thread, a row wider than any block;
# 5x46x46: 2116 rows on 2048 blocks; 65x9x5: one more than a multiple of the force pass's 64 x 4 x 1 block on each axis
SHAPES = ([4, 4, 4], [4, 4, 5], [5, 7, 4], [33, 22, 27], [513, 4, 4], [5, 46, 46], [65, 9, 5])
CASES = [("uniform", s) for s in SHAPES] + [("aniso", [33, 22, 27]), ("aniso", [5, 7, 4])]
MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def field(mesh):
    """the ABC field with an interior bump: not force-free, not solenoidal, nowhere zero"""
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
    """(B, hist, info) of the device against the model's, bit for bit"""
    gB, gh, gi = got
    wB, wh, wi = want
    assert gi == wi, (what, gi, wi, gh, wh)
    assert gh.shape == wh.shape and gh.tobytes() == wh.tobytes(), (what, gh, wh)
    assert gB.shape == wB.shape, what
    bad = gB.view(np.uint64) != wB.view(np.uint64)
    assert not bad.any(), (what, int(bad.sum()), float(np.abs(gB - wB).max()))


@pytest.mark.parametrize("mname,ns", CASES, ids=[m + "-" + IDS(s) for m, s in CASES])
def test_driver_equals_the_model(hip, mname, ns):
    """after 1, 2 and 7 tries, without a weight, with boundary_weight(nd = 2) and with a non-separable weight: the
    field, the history and info of the host entry are the model's; 1 and 2 accepted tries leave the current field in
    either buffer.  Two calls give the same bits"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b = field(mesh)
    V = ndsm_amd.VecPot(*mesh)
    try:
        parities = set()
        for kind in ("none", "cosine", "nonsep"):
            w = weight(kind, mesh, b.shape[1:])
            for n in (1, 2, 7):
                what = "%s %s w %s, %d tries" % (mname, ns, kind, n)
                wB, wh, wi, _ = M.run(mesh, b, w, niter_max=n, check=1, tol=0.0)
                ierr, B, hist, info = V.optimize(b, w=w, start="given", niter_max=n, check=1, tol=0.0)
                assert ierr == 0, what
                same((B, hist, info), (wB, wh, wi), what)
                assert info == (n + 1, n, 0) and np.isfinite(hist).all() and hist[-1, 1] < hist[0, 1], (what, hist)
                parities.add(int(hist[-1, 5]) % 2)
                if n == 7:
                    again = V.optimize(b, w=w, start="given", niter_max=n, check=1, tol=0.0)
                    same(again[1:], (B, hist, info), what + ", second call")
                    # the same field whatever the check interval
                    _, B3, hist3, info3 = V.optimize(b, w=w, start="given", niter_max=n, check=3, tol=0.0)
                    w3 = M.run(mesh, b, w, niter_max=n, check=3, tol=0.0)
                    same((B3, hist3, info3), w3[:3], what + ", check 3")
                    assert info3 == (4, 7, 0) and np.array_equal(B3.view(np.uint64), B.view(np.uint64)), what
                    assert hist3[-1].tobytes() == hist[-1].tobytes()
        assert parities == {0, 1}
    finally:
        V.close()


@pytest.mark.parametrize("mname,ns", [("uniform", [5, 7, 4]), ("aniso", [33, 22, 27]), ("uniform", [513, 4, 4])],
                         ids=["uniform-5x7x4", "aniso-33x22x27", "uniform-513x4x4"])
def test_rejections_and_stop_rules(hip, mname, ns):
    """a first step far too large: the first tries are rejected and write the same trial buffer again, later ones are
    accepted and flip the index; then the three stop rules and a history that runs out of rows"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b = field(mesh)
    h2 = min(M.spacing(mesh)) ** 2
    V = ndsm_amd.VecPot(*mesh)
    try:
        for kind in ("none", "nonsep"):
            w = weight(kind, mesh, b.shape[1:])
            for kw in (dict(niter_max=12, check=12, tol=0.0, dt0=16.0 * h2),                # rejected, then accepted
                       dict(niter_max=11, check=4, tol=0.0, dt0=3.0 * h2, hist_rows=3),   # rows run out; a short tail
                       dict(niter_max=50, check=5, tol=0.999),                              # tol at the first check
                       dict(niter_max=50, check=5, dt0=100.0, dt_min=60.0),                 # dt_min after one rejection
                       dict(niter_max=50, check=5, dt0=1.0, dt_min=2.0),                    # dt_min before any try
                       dict(niter_max=40, check=40, tol=0.0, dt0=1e300)):                   # overflow: inf and NaN in L_T
                what = "%s %s w %s %s" % (mname, ns, kind, kw)
                want = M.run(mesh, b, w, **kw)
                ierr, B, hist, info = V.optimize(b, w=w, start="given", **kw)
                assert ierr == 0
                same((B, hist, info), want[:3], what)
            _, B, hist, info = V.optimize(b, w=w, start="given", niter_max=12, check=12, tol=0.0, dt0=16.0 * h2)
            assert info == (2, 12, 0) and 0 < hist[1, 5] < 12, hist                 # both rejections and acceptances
        _, B, hist, info = V.optimize(b, start="given", niter_max=50, check=5, dt0=100.0, dt_min=60.0)
        assert info == (2, 1, 2) and np.array_equal(B.view(np.uint64), b.view(np.uint64))
        _, B, hist, info = V.optimize(b, start="given", niter_max=50, check=5, tol=0.999)
        assert info == (2, 5, 1)
        # the all-zero field: L = 0, and a first try that is rejected
        z = np.zeros_like(b)
        _, B, hist, info = V.optimize(z, start="given", niter_max=1, check=1, tol=0.0)
        assert hist[0, 1] == 0.0 and list(hist[1, [0, 1, 5]]) == [1.0, 0.0, 0.0] and not B.any()
        # a field that is zero at some nodes
        bz = b.copy()
        bz[:, 1, 2, 1] = 0.0
        bz[:, 0, 0, :] = 0.0
        want = M.run(mesh, bz, None, niter_max=3, check=1, tol=0.0)
        _, B, hist, info = V.optimize(bz, start="given", niter_max=3, check=1, tol=0.0)
        same((B, hist, info), want[:3], "zero nodes")
        assert np.isfinite(hist).all()
    finally:
        V.close()


def options(V):
    return V._options(10000, 1024, 1e-13, 1e-10, 5, False, False, False)


@pytest.mark.parametrize("mname,ns", [("uniform", [4, 4, 4]), ("aniso", [5, 7, 4]), ("aniso", [33, 22, 27])],
                         ids=["uniform-4x4x4", "aniso-5x7x4", "aniso-33x22x27"])
def test_host_entry_device_entry_and_offset_arrays(hip, mname, ns):
    """ndsm_hip_vecpot_optimize = ndsm_hip_vecpot_optimize_device on arrays of their own = the same on views into one
    larger allocation (8 mod 16, NaN bands beside B and w): B comes out, w is read only, nothing else changes; 2 and 3
    tries, so that the result is copied into the caller's array once and lies there once"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b = field(mesh)
    h2 = min(M.spacing(mesh)) ** 2
    V = ndsm_amd.VecPot(*mesh)
    L = V.L
    try:
        for kind in ("none", "nonsep"):
            w = weight(kind, mesh, b.shape[1:])
            for n in (2, 3):
                args = (1, n, 2, 0.0, 0.1 * h2, 1e-7 * h2)
                want = M.run(mesh, b, w, niter_max=n, check=2, tol=0.0, dt0=0.1 * h2, dt_min=1e-7 * h2, hist_rows=4)
                io, ro = options(V)
                B = b.reshape(-1).copy()
                W = None if w is None else w.reshape(-1).copy()
                hist, info = np.full((4, 6), np.nan), np.full(3, FILL, dtype=np.intc)
                rc = L.ndsm_hip_vecpot_optimize(V.h, io.ctypes.data_as(_ip), ro.ctypes.data_as(_dp), B.ctypes.data,
                                                None if W is None else W.ctypes.data, *args, hist.ctypes.data, 4,
                                                info.ctypes.data)
                assert rc == 0, hip.last_error(L)
                assert W is None or np.array_equal(W, w.reshape(-1))
                rows = int(info[0])
                assert np.isnan(hist[rows:]).all()                   # rows past the ones written are left alone
                same((B.reshape(b.shape), hist[:rows], tuple(int(v) for v in info)), want[:3], "host entry")
                for plain in (False, True):
                    slots = [slot("B", b.reshape(-1), output=True, field=True)]
                    if w is not None:
                        slots.append(slot("w", w.reshape(-1), field=True))
                    io_d, ro_d = options(V)
                    hist_d, info_d = np.full((4, 6), np.nan), np.full(3, FILL, dtype=np.intc)
                    R = Arena(LibTransport(L), slots, plain=plain)
                    got = R.run(lambda dB, dw=None: L.ndsm_hip_vecpot_optimize_device(
                        V.h, io_d.ctypes.data_as(_ip), ro_d.ctypes.data_as(_dp), dB, dw, *args, hist_d.ctypes.data, 4,
                        info_d.ctypes.data))
                    what = "%s %s w %s %d tries plain %s" % (mname, ns, kind, n, plain)
                    assert R.rc == 0, (what, hip.last_error(L))
                    assert np.array_equal(got[0].view(np.uint64), B.view(np.uint64)), what
                    assert hist_d.tobytes() == hist.tobytes() and info_d.tobytes() == info.tobytes(), what
                    assert np.array_equal(io_d, io), what
    finally:
        V.close()


@pytest.mark.parametrize("mname,ns", [("uniform", [12, 10, 9]), ("aniso", [20, 17, 23])], ids=["uniform-12x10x9", "aniso-20x17x23"])
def test_potential_start_is_the_hand_built_chain(hip, mname, ns):
    """start = "potential" equals: the potential field of b's B.n by the device entry of solve(), the k = 0 plane of b
    put over it, then start = "given".  The side and top faces are the potential field's"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b = field(mesh)
    V = ndsm_amd.VecPot(*mesh)
    try:
        ierr_s, _, bp = V.solve(b, device=True)
        fail = int(V.last_ioptc[V.L.get_iopt_fail3d()])
        b0 = bp.copy()
        b0[:, 0] = b[:, 0]
        for w in (None, weight("cosine", mesh, b.shape[1:])):
            for device in (False, True):
                ierr_g, Bg, hist_g, info_g = V.optimize(b0, w=w, start="given", niter_max=3, check=2, tol=0.0)
                ierr_p, Bp, hist_p, info_p = V.optimize(b, w=w, start="potential", niter_max=3, check=2, tol=0.0,
                                                        device=device)
                same((Bp, hist_p, info_p), (Bg, hist_g, info_g), "potential start, device %s" % device)
                assert ierr_g == 0 and ierr_p == (1 if ierr_s != 0 or fail != 0 else 0)
                face = np.ones(b.shape[1:], dtype=bool)
                face[1:-1, 1:-1, 1:-1] = False
                assert np.array_equal(Bp[:, face].view(np.uint64), b0[:, face].view(np.uint64))
                assert np.array_equal(Bp[:, 0], b[:, 0]) and not np.array_equal(Bp[:, -1], b[:, -1])
        want = M.run(mesh, b0, None, niter_max=3, check=2, tol=0.0)
        same(V.optimize(b, start="potential", niter_max=3, check=2, tol=0.0)[1:], want[:3], "potential start, model")
    finally:
        V.close()


def test_argument_errors_of_the_c_entries(hip):
    import ndsm_amd
    mesh = uniform_mesh([5, 7, 4])
    b = field(mesh)
    V = ndsm_amd.VecPot(*mesh)
    L = V.L
    nan, inf = float("nan"), float("inf")
    try:
        dB = ctypes.c_void_p()
        assert L.ndsm_hip_device_alloc(b.nbytes, ctypes.byref(dB)) == 0
        try:
            assert L.ndsm_hip_memcpy_h2d(dB, b.ctypes.data, b.nbytes) == 0
            for name, pB in (("ndsm_hip_vecpot_optimize", ctypes.c_void_p(b.ctypes.data)),
                             ("ndsm_hip_vecpot_optimize_device", dB)):
                fn = getattr(L, name)

                def call(h=V.h, B=pB, args=(1, 3, 1, 0.0, 1e-3, 0.0), rows=4, hist=True, info=True):
                    io, ro = options(V)
                    hh, ii = np.full((4, 6), nan), np.full(3, FILL, dtype=np.intc)
                    rc = fn(h, io.ctypes.data_as(_ip), ro.ctypes.data_as(_dp), B, None, *args,
                            hh.ctypes.data if hist else None, rows, ii.ctypes.data if info else None)
                    return rc, hh, ii
                rc, hh, ii = call()
                assert rc == 0 and tuple(ii) == (4, 3, 0) and np.isfinite(hh).all()
                for args in ((2, 3, 1, 0.0, 1e-3, 0.0), (-1, 3, 1, 0.0, 1e-3, 0.0), (1, 0, 1, 0.0, 1e-3, 0.0),
                             (1, 3, 0, 0.0, 1e-3, 0.0), (1, 3, 1, -1e-9, 1e-3, 0.0), (1, 3, 1, nan, 1e-3, 0.0),
                             (1, 3, 1, inf, 1e-3, 0.0), (1, 3, 1, 0.0, 0.0, 0.0), (1, 3, 1, 0.0, -1.0, 0.0),
                             (1, 3, 1, 0.0, inf, 0.0), (1, 3, 1, 0.0, nan, 0.0), (1, 3, 1, 0.0, 1e-3, -1.0),
                             (1, 3, 1, 0.0, 1e-3, nan), (1, 3, 1, 0.0, 1e-3, inf)):
                    rc, hh, ii = call(args=args)
                    assert rc == 9004 and not ii.any() and not hh.any(), (name, args, rc)
                rc, hh, ii = call(rows=1)
                assert rc == 9004 and not ii.any() and not hh[0].any() and np.isnan(hh[1:]).all()
                assert call(h=None)[0] == 9002 and call(B=None)[0] == 9002
                assert call(hist=False)[0] == 9002 and call(info=False)[0] == 9002
            back = np.empty_like(b)
            assert L.ndsm_hip_memcpy_d2h(back.ctypes.data, dB, b.nbytes) == 0
        finally:
            L.ndsm_hip_device_free(dB)
    finally:
        V.close()


def test_other_entries_of_the_handle_are_untouched(hip):
    """solve(), force_free() and helicity() give the same bits before and after an optimize() on one handle"""
    import ndsm_amd
    mesh = uniform_mesh([12, 10, 9])
    b = field(mesh)
    alpha0 = ndsm_amd.boundary_alpha(mesh[0], mesh[1], b, 1e-3)
    V = ndsm_amd.VecPot(*mesh)

    def others():
        s = V.solve(b)
        f = V.force_free(b, alpha0, niter_max=1)
        h = V.helicity(b)
        return [np.asarray(v) for v in s] + [np.asarray(v) for v in f] + [np.asarray(v, dtype=np.float64) for v in h[:10]]
    try:
        before = others()
        for start in ("given", "potential"):
            V.optimize(b, w=weight("cosine", mesh, b.shape[1:]), start=start, niter_max=3, check=2)
            after = others()
            assert len(before) == len(after)
            for x, y in zip(before, after):
                assert x.shape == y.shape and x.tobytes() == y.tobytes()
    finally:
        V.close()
