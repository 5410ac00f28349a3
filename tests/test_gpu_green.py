"""GPU tests of the Green's-function entries (csrc/green.hip; semantics: include/ndsm_hip.h, "Open-box potential
field") against their numpy model (tests/green_model.py), bit for bit: the points entry over the source shapes at
which the tiles and the slices change, the box entry's two target sets against each other and against the points
entry, calls of more targets than one launch takes (all three target generators), the host entries against the device
entries on offset caller arrays, solve_open against the composition it stands for, and every 9002 and 9004 case.
Nothing here is taken from the device code's results.

The sums are IEEE +, *, / and sqrt in the stated order, so the comparison is for equal bits; each points case prints its
largest gap in units of eps * sum |term| (0 when the bits agree) before it asserts."""
import ctypes
import functools

import numpy as np
import pytest

import green_model as gm
from device_arena import Arena, LibTransport, slot

pytestmark = pytest.mark.gpu

_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
IDS = lambda s: "x".join(map(str, s))   # noqa: E731

# nsx x nsy.  2x2: the smallest; 17x15 (255 pixels), 16x16 and 257x2: one short of a tile of 256, a whole tile, two tiles
# and a rest; 65x63 (4095), 64x64 and 65x64: the last sizes of one slice and the first of two; 513x512: 64 slices of
# 4104 pixels, the last one short
SOURCES = [(2, 2), (17, 15), (16, 16), (257, 2), (65, 63), (64, 64), (65, 64), (513, 512)]
NPTS = [1, 63, 64, 65, 257]          # around a wavefront, and more than one block of 256 targets
BOXES = [(2, 2, 2), (3, 3, 3), (5, 4, 3), (17, 12, 9)]


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    assert not bad.any(), (what, int(bad.sum()), float(np.nanmax(np.abs(got - want))))


def source(ns, seed=2):
    """a rough magnetogram on a mesh with unequal spacings and a shifted origin; zs off zero"""
    nsx, nsy = ns
    rng = np.random.default_rng(seed + 7 * nsx + nsy)
    xs, ys = 0.37 + 0.013 * np.arange(nsx), -1.21 + 0.017 * np.arange(nsy)
    return xs, ys, 0.25, rng.uniform(-1.0, 1.0, size=(nsy, nsx)) + 0.3


def mixed_targets(xs, ys, zs, n, seed=4):
    """n targets, five kinds in turn: above the plane, on it at a source node, on it off the nodes, below it, outside
    the source's extent (above the plane and on it in turn)"""
    rng = np.random.default_rng(seed + len(xs))
    lx, ly = xs[-1] - xs[0], ys[-1] - ys[0]
    P = np.empty((n, 3))
    for t in range(n):
        kind = t % 5
        X, Y = xs[0] + lx * rng.uniform(-0.1, 1.1), ys[0] + ly * rng.uniform(-0.1, 1.1)
        Z = zs + rng.uniform(0.001, 0.4)
        if kind == 1:
            X, Y, Z = xs[rng.integers(len(xs))], ys[rng.integers(len(ys))], zs
        elif kind == 2:
            X, Y, Z = xs[0] + lx * rng.uniform(0.01, 0.99), ys[0] + ly * rng.uniform(0.01, 0.99), zs
        elif kind == 3:
            Z = zs - rng.uniform(0.001, 0.4)
        elif kind == 4:
            X = xs[-1] + rng.uniform(0.01, 1.0) if t % 2 else xs[0] - rng.uniform(0.01, 1.0)
            Z = zs if t % 10 == 4 else Z
        P[t] = X, Y, Z
    P[n - 1] = xs[-1], ys[-1], zs                  # the last node: theta = 1 on both axes
    return P


@functools.lru_cache(maxsize=None)
def points_case(ns):
    """the source, 257 mixed targets, the model's field at them and the model's sum |term|: computed once per source"""
    xs, ys, zs, bz = source(ns)
    P = mixed_targets(xs, ys, zs, max(NPTS))
    sums, mag = gm.green_sums(xs, ys, zs, bz, P[:, 0], P[:, 1], P[:, 2], with_abs=True)
    want = gm.green_points(xs, ys, zs, bz, P)
    for a in (P, want, mag):
        a.setflags(write=False)
    return xs, ys, zs, bz, P, want, mag.T


@pytest.mark.parametrize("npts", NPTS)
@pytest.mark.parametrize("ns", SOURCES, ids=IDS)
def test_points_equal_the_model(hip, ns, npts):
    xs, ys, zs, bz, P, want, mag = points_case(ns)
    P, want, mag = P[:npts], want[:npts], mag[:npts]
    if npts == 1:
        assert np.isfinite(want).all()
    else:
        assert np.isnan(want[3]).all() and np.isfinite(want[[0, 1, 2, 4]]).all()
    for device in (False, True):
        got = hip.green_field_points(xs, ys, zs, bz, P, device=device)
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        with np.errstate(all="ignore"):
            gap = np.where(fin & (mag > 0), np.abs(got - want) / (np.finfo(float).eps * mag), 0.0)
        print("source %s npts %d device %s: largest gap %.3g eps sum|term|" % (IDS(ns), npts, device, gap[fin].max()))
        bits(got, want, (ns, npts, device))


def test_points_do_not_depend_on_their_number_or_order(hip):
    xs, ys, zs, bz, P, want, _ = points_case((65, 64))
    perm = np.random.default_rng(0).permutation(len(P))
    bits(hip.green_field_points(xs, ys, zs, bz, P[perm]), want[perm], "permuted")
    bits(hip.green_field_points(xs, ys, zs, bz, P[200:201]), want[200:201], "one of many")


def test_no_points_touch_nothing(hip):
    xs, ys, zs, bz = source((5, 4))
    assert hip.green_field_points(xs, ys, zs, bz, np.zeros((0, 3))).shape == (0, 3)
    assert hip.green_field_points(xs, ys, zs, bz, np.zeros((0, 3)), device=True).shape == (0, 3)


def test_non_finite_bz_propagates(hip):
    xs, ys, zs, bz = source((17, 15))
    bz = bz.copy()
    bz[3, 4], bz[9, 2] = np.nan, np.inf
    P = mixed_targets(xs, ys, zs, 65)
    P[1] = xs[4], ys[3], zs                        # on the NaN pixel: the sums leave it out, Bz takes it
    want = gm.green_points(xs, ys, zs, bz, P)
    assert np.isnan(want[0]).all() and np.isnan(want[1, 2])
    got = hip.green_field_points(xs, ys, zs, bz, P)
    # (which NaN comes out - its sign and payload - is not part of the semantics: NaN where the model has NaN)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want)
    assert fin.any()
    bits(got[fin], want[fin], "non-finite bz")


CHUNK = 262144                       # csrc/green.hip takes the targets of a call through in launches of at most this many


def tiny_source():
    """six pixels: the model of a quarter of a million targets costs nothing"""
    return 0.37 + 0.21 * np.arange(3), -0.4 + 0.33 * np.arange(2), 0.25, np.array([[0.7, -1.1, 0.4], [1.3, 0.2, -0.9]])


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_points_past_one_chunk(hip, device):
    """262144 + 300 points: a second launch whose targets start at 262144, whose count (300) is below the first one's
    and no multiple of the block of 256, and whose slice sums reuse the first launch's scratch.  All targets differ, so
    a target written from the other launch's sums, or to the other launch's place, shows"""
    xs, ys, zs, bz = tiny_source()
    n = CHUNK + 300
    rng = np.random.default_rng(21)
    P = np.array([rng.uniform(0.0, 1.2, n), rng.uniform(-0.8, 0.4, n), zs + rng.uniform(0.001, 0.5, n)]).T
    t = np.arange(n)
    P[t % 5 == 1, 2] = zs                                  # on the plane, inside and outside the source
    P[t % 7 == 3, 2] -= 0.6                                # below it
    want = gm.green_points(xs, ys, zs, bz, P)
    edge = slice(CHUNK - 256, n)                           # both sides of the boundary, and the short last launch
    assert np.isnan(want[edge]).any() and np.isfinite(want[edge]).any() and (P[edge, 2] == zs).any()
    assert not np.array_equal(want[:300], want[CHUNK:])
    got = hip.green_field_points(xs, ys, zs, bz, P, device=device)
    bits(got[edge], want[edge], "around the boundary")
    bits(got, want, "all")


# nx x ny x nz.  65x65x63: 266175 nodes, 4031 in the second launch; 2x365x361: 263530 nodes that are all face nodes
@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("n3,which", (((65, 65, 63), "volume"), ((2, 365, 361), "faces")), ids=("volume", "faces"))
def test_box_past_one_chunk(hip, n3, which, device):
    nx, ny, nz = n3
    assert nx * ny * nz > CHUNK and (nx * ny * nz - CHUNK) % 256 != 0
    x, y, z = 0.31 + np.linspace(0.0, 0.7, nx), -0.55 + np.linspace(0.0, 0.8, ny), 0.25 + np.linspace(0.0, 0.6, nz)
    xs, ys, zs, bz = tiny_source()
    want = gm.green_box(x, y, z, bz, xs, ys, zs, which="volume")
    assert which == "volume" or gm.face_mask(want.shape[1:]).all()
    assert np.isfinite(want).all()
    got = hip.magnetogram_field(x, y, z, bz, xs, ys, zs, which=which, device=device)
    flat = slice(CHUNK - 256, CHUNK + 256)
    bits(got.reshape(3, -1)[:, flat], want.reshape(3, -1)[:, flat], "around the boundary")
    bits(got, want, (n3, which))


def box_mesh(n3, on_plane):
    """unequal spacings, a shifted origin; the source of box_source() is wider than its footprint and not aligned"""
    nx, ny, nz = n3
    x = 0.41 + np.linspace(0.0, 0.9, nx)
    y = -0.77 + np.linspace(0.0, 0.6, ny)
    z = (0.25 if on_plane else 0.31) + np.linspace(0.0, 0.45, nz)
    return x, y, z


def box_source():
    rng = np.random.default_rng(9)
    xs, ys = -0.513 + 0.047 * np.arange(52), -1.694 + 0.061 * np.arange(41)
    return xs, ys, 0.25, rng.uniform(-1.0, 1.0, size=(41, 52)) + 0.3


@pytest.mark.parametrize("on_plane", (True, False), ids=("z0=zs", "z0>zs"))
@pytest.mark.parametrize("n3", BOXES, ids=IDS)
def test_box_faces_volume_and_points_agree(hip, n3, on_plane):
    x, y, z = box_mesh(n3, on_plane)
    xs, ys, zs, bz = box_source()
    assert xs[0] < x[0] and xs[-1] > x[-1] and ys[0] < y[0] and ys[-1] > y[-1]
    want = gm.green_box(x, y, z, bz, xs, ys, zs, which="volume")
    assert np.isfinite(want).all()
    mask = gm.face_mask(want.shape[1:])
    assert mask.all() == (min(n3) == 2) and (~mask).sum() == (n3[0] - 2) * (n3[1] - 2) * (n3[2] - 2)
    Zg, Yg, Xg = np.meshgrid(z, y, x, indexing="ij")
    pts = hip.green_field_points(xs, ys, zs, bz, np.array([Xg[mask], Yg[mask], Zg[mask]]).T)
    for device in (False, True):
        vol = hip.magnetogram_field(x, y, z, bz, xs, ys, zs, which="volume", device=device)
        bits(vol, want, ("volume", n3, device))
        faces = hip.magnetogram_field(x, y, z, bz, xs, ys, zs, which="faces", device=device)
        bits(faces[:, mask], vol[:, mask], ("faces", n3, device))
        assert not faces[:, ~mask].any()                       # zeros inside
        bits(pts.T.copy(), faces[:, mask], ("points", n3, device))
    if on_plane:
        bits(vol[2, 0], gm.plane_bz(xs, ys, bz, Xg[0], Yg[0]), "the plane's Bz")


def green_box_raw(hip, L, src, mesh, which, B, device):
    """the raw entry on B (flat, as the caller holds it): host, or device through an arena of offset arrays with NaN
    bands beside bz and B; returns (rc, B afterwards)"""
    xs, ys, zs, bz = src
    x, y, z = mesh
    ns2, n3 = np.array([len(xs), len(ys)], dtype=np.intc), np.array([len(x), len(y), len(z)], dtype=np.intc)
    head = (ns2.ctypes.data_as(_ip), xs.ctypes.data_as(_dp), ys.ctypes.data_as(_dp), zs)
    tail = (n3.ctypes.data_as(_ip), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), z.ctypes.data_as(_dp), which)
    S = np.ascontiguousarray(bz).reshape(-1)
    if not device:
        out = B.copy()
        return L.ndsm_hip_green_box(*head, S.ctypes.data, *tail, out.ctypes.data), out
    arena = Arena(LibTransport(L), [slot("bz", S, field=True), slot("B", B, output=True, field=True)])
    _, out = arena.run(lambda dS, dB: L.ndsm_hip_green_box_device(*head, dS, *tail, dB))
    return arena.rc, out


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("n3", BOXES[1:], ids=IDS)
def test_box_host_equals_device_on_offset_arrays(hip, n3, which):
    L = hip.load_library()
    mesh, src = box_mesh(n3, True), box_source()
    n = int(np.prod(n3))
    B = np.full(3 * n, np.nan)                              # the sentinel the interior keeps for which = 0
    rc_h, host = green_box_raw(hip, L, src, mesh, which, B, False)
    rc_d, dev = green_box_raw(hip, L, src, mesh, which, B, True)
    assert rc_h == 0 and rc_d == 0
    bits(dev, host, (n3, which))
    mask = np.broadcast_to(gm.face_mask(n3[::-1]), (3,) + tuple(n3[::-1])).reshape(-1)
    if which == 0:
        assert np.isnan(host[~mask]).all() and np.isfinite(host[mask]).all()
    else:
        assert np.isfinite(host).all()
    bits(host[mask].reshape(3, -1), gm.green_box(*mesh, src[3], src[0], src[1], src[2])[:, gm.face_mask(n3[::-1])], "model")


@pytest.mark.parametrize("npts", (1, 65, 257))
def test_points_host_equals_device_on_offset_arrays(hip, npts):
    L = hip.load_library()
    xs, ys, zs, bz, P, want, _ = points_case((65, 64))
    P = np.ascontiguousarray(P[:npts]).reshape(-1)
    ns2 = np.array([len(xs), len(ys)], dtype=np.intc)
    head = (ns2.ctypes.data_as(_ip), xs.ctypes.data_as(_dp), ys.ctypes.data_as(_dp), zs)
    S = np.ascontiguousarray(bz).reshape(-1)
    host = np.full(3 * npts, 7.0)
    assert L.ndsm_hip_green_points(*head, S.ctypes.data, npts, P.ctypes.data, host.ctypes.data) == 0
    arena = Arena(LibTransport(L), [slot("bz", S, field=True), slot("pts", P, field=True),
                                    slot("B", np.full(3 * npts, 7.0), output=True)])
    _, _, dev = arena.run(lambda dS, dP, dB: L.ndsm_hip_green_points_device(*head, dS, npts, dP, dB))
    assert arena.rc == 0
    bits(dev, host, npts)
    bits(host.reshape(-1, 3), want[:npts], "model")


def open_case():
    """17 x 12 x 9 with hy != hx, and the monopole pair's Bz on a plane wider than the box.  The box's x and y are
    slices of the source mesh: a box node on the plane is then bitwise a source node, which the punctured rule leaves
    out - a target that misses a source node by a rounding error would get a term of the order 1 / eps^2 instead."""
    hx, hy = 0.125, 1.6 / 11
    xs, ys = hx * np.arange(-24, 25), hy * (np.arange(-20, 20) + 0.5)
    x, y = xs[16:33].copy(), ys[14:26].copy()
    assert len(x) == 17 and len(y) == 12 and x[0] == -1.0 and x[-1] == 1.0 and abs(y[0] + 0.8) < 1e-12
    Ys, Xs = np.meshgrid(ys, xs, indexing="ij")
    return x, y, hx * np.arange(9), xs, ys, gm.monopole_pair(Xs, Ys, 0.0)[2]


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_solve_open_is_magnetogram_field_then_solve(hip, device):
    x, y, z, xs, ys, bz = open_case()
    V = hip.VecPot(x, y, z)
    try:
        ierr, A, B = V.solve_open(bz, xs=xs, ys=ys, zs=0.0, device=device)
        assert ierr == 0 and V.last_ioptc[8] == 0               # every solve reached vc_tol
        b = hip.magnetogram_field(x, y, z, bz, xs=xs, ys=ys, zs=0.0, device=device)
        ierr2, A2, B2 = V.solve(b, device=device)
        assert ierr2 == 0
        bits(A, A2, "A")
        bits(B, B2, "B")
        # the field it is meant to be, to the accuracy of the 7-point solve at this size
        Zg, Yg, Xg = np.meshgrid(z, y, x, indexing="ij")
        exact = gm.monopole_pair(Xg, Yg, Zg)
        inner = (slice(None), slice(1, -1), slice(1, -1), slice(1, -1))
        assert np.abs(B[inner] - exact[inner]).max() < 0.15 * np.abs(exact[inner]).max()
        # the one-shot form, and the defaults xs = x, ys = y, zs = z[0]
        if not device:
            own = bz[14:26, 16:33]
            ierr3, A3, B3 = hip.potential_open(x, y, z, own)
            ierr4, A4, B4 = V.solve(hip.magnetogram_field(x, y, z, own))
            assert ierr3 == 0 and ierr4 == 0
            bits(A3, A4, "one-shot A")
            bits(B3, B4, "one-shot B")
    finally:
        V.close()


def test_error_codes_leave_the_outputs_untouched(hip):
    L = hip.load_library()
    xs, ys, zs, bz = source((5, 4))
    S = np.ascontiguousarray(bz).reshape(-1)
    x, y, z = box_mesh((3, 3, 3), True)
    P = np.ascontiguousarray(mixed_targets(xs, ys, zs, 4)).reshape(-1)

    def ip(v):
        return None if v is None else np.array(v, dtype=np.intc).ctypes.data_as(_ip)

    def dp(v):
        return None if v is None else v.ctypes.data_as(_dp)

    def vp(v):
        return None if v is None else v.ctypes.data

    def points(device, ns=(5, 4), sx=xs, sy=ys, s=S, npts=4, pts=P, out=True):
        B = np.full(12, 3.25)
        fn = L.ndsm_hip_green_points_device if device else L.ndsm_hip_green_points
        rc = fn(ip(ns), dp(sx), dp(sy), zs, vp(s), npts, vp(pts), vp(B) if out else None)
        assert (B == 3.25).all()
        return rc

    def box(device, ns=(5, 4), sx=xs, sy=ys, s=S, n3=(3, 3, 3), mx=x, my=y, mz=z, which=0, zs_=zs, out=True):
        B = np.full(81, 3.25)
        fn = L.ndsm_hip_green_box_device if device else L.ndsm_hip_green_box
        rc = fn(ip(ns), dp(sx), dp(sy), zs_, vp(s), ip(n3), dp(mx), dp(my), dp(mz), which, vp(B) if out else None)
        assert (B == 3.25).all()
        return rc

    flat, back = np.array([1.0, 1.0, 2.0, 3.0, 4.0]), xs[::-1].copy()
    for device in (False, True):
        # (device: the value and NULL checks come before any array is looked at, so host addresses do no harm)
        for kw in (dict(ns=None), dict(sx=None), dict(sy=None), dict(s=None), dict(pts=None), dict(out=False)):
            assert points(device, **kw) == 9002, (device, kw)
        for kw in (dict(ns=(1, 4)), dict(ns=(5, 1)), dict(sx=flat), dict(sx=back), dict(sy=np.zeros(4)), dict(npts=-1),
                   dict(sx=np.array([0.0, np.nan, 2, 3, 4]))):
            assert points(device, **kw) == 9004, (device, kw)
        assert points(device, npts=0) == 0 and points(device, npts=0, pts=None, out=False) == 0
        for kw in (dict(ns=None), dict(sx=None), dict(sy=None), dict(s=None), dict(n3=None), dict(mx=None), dict(my=None),
                   dict(mz=None), dict(out=False)):
            assert box(device, **kw) == 9002, (device, kw)
        for kw in (dict(ns=(1, 4)), dict(ns=(5, 1)), dict(sx=flat), dict(sy=ys[::-1].copy()), dict(which=2), dict(which=-1),
                   dict(n3=(1, 3, 3)), dict(n3=(3, 1, 3)), dict(n3=(3, 3, 1)), dict(zs_=np.nextafter(z[0], 9.0))):
            assert box(device, **kw) == 9004, (device, kw)
    # the handle entry
    V = hip.VecPot(*box_mesh((5, 4, 4), True))
    try:
        ioptc, ropt = V._options(10000, 1024, 1e-13, 1e-10, 5, False, False, False)
        for device in (False, True):
            fn = L.ndsm_hip_vecpot_open_device if device else L.ndsm_hip_vecpot_open

            def run(h=V.h, ns=(5, 4), sx=xs, sy=ys, s=S, zs_=zs, a=True, b=True):
                A, B = np.full(240, 1.5), np.full(240, 3.25)
                rc = fn(h, ioptc.ctypes.data_as(_ip), ropt.ctypes.data_as(_dp), ip(ns), dp(sx), dp(sy), zs_, vp(s),
                        vp(A) if a else None, vp(B) if b else None)
                assert (A == 1.5).all() and (B == 3.25).all()
                return rc
            for kw in (dict(h=None), dict(ns=None), dict(sx=None), dict(sy=None), dict(s=None), dict(a=False), dict(b=False)):
                assert run(**kw) == 9002, (device, kw)
            for kw in (dict(ns=(1, 4)), dict(ns=(5, 1)), dict(sx=flat), dict(sy=ys[::-1].copy()),
                       dict(zs_=np.nextafter(V.z[0], 9.0))):
                assert run(**kw) == 9004, (device, kw)
    finally:
        V.close()
