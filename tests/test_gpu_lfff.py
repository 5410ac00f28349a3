"""GPU tests of the constant-alpha force-free entries (pairs_k<LfffTerm> in csrc/green.hip; semantics:
include/ndsm_hip.h, "Linear force-free field") against the Green's-function entries and against their numpy
model (tests/lfff_model.py).

alpha = 0: equal bits with ndsm_hip_green_points / ndsm_hip_green_box.  alpha != 0: the device's sin and cos are not
numpy's, so the comparison with the model is a cap and not bit for bit.  With M the model's per-component scale (per
pair (1 + |ar|) times the sum of the absolute products of each addend) each case computes the float64 model's own
error against the same lines in np.longdouble, c0 = max gap / (eps M) - the accumulation's share - and the device must
stay within (2 c0 + 16) eps M: its error is of the model's kind and order, once each, and 16 allows 4 ulp on each of
sin and cos where they enter an addend at most twice.  The structure of the entries (faces, volume, points, chunks,
caller arrays) is tested for equal bits among the device's own results.  Nothing here is taken from the device code.

Measured on an MI355X: the largest device gap is 0.333 eps M (2 x 2, alpha 0.3) over the 24 point cases, whose c0 run
from 0.015 to 31 (64 x 64, alpha 0.3; 27 for 65 x 63 at alpha 3), and 1.27 eps M over the box and chunk cases (c0 2.0
to 15.5): the device does the model's own float64 roundings and differs from it in sin and cos alone, so it sits far
closer to the model than the model does to its long-double self.  DESIGN.md section 35 has the table."""
import ctypes
import functools

import numpy as np
import pytest

import green_model as gm
import lfff_model as lm
from device_arena import Arena, LibTransport, slot
from test_gpu_green import (SOURCES, NPTS, BOXES, IDS, CHUNK, hip, bits, source, mixed_targets, tiny_source,  # noqa: F401
                            box_mesh, box_source)

pytestmark = pytest.mark.gpu

_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)
EPS = np.finfo(float).eps
ALPHAS = [0.3, 3.0, -25.0]


def well_apart(xs, ys, X, Y):
    """no target (X[t], Y[t]) has 0 < R2 < (h / 1024)^2 to any pixel: on the vertical through a pixel bit for bit, or
    well away from it (the hazard of the header)"""
    lim = (min(xs[1] - xs[0], ys[1] - ys[0]) / 1024) ** 2
    for lo in range(0, len(X), 4096):
        dx2 = np.sort((X[lo:lo + 4096, None] - xs[None, :]) ** 2, axis=1)[:, :2]      # the two nearest columns and rows
        dy2 = np.sort((Y[lo:lo + 4096, None] - ys[None, :]) ** 2, axis=1)[:, :2]
        R2 = dx2[:, :, None] + dy2[:, None, :]
        assert not ((R2 > 0) & (R2 < lim)).any()


def targets(ns):
    """test_gpu_green's 257 mixed targets and one straight above a node"""
    xs, ys, zs, bz = source(ns)
    P = np.concatenate([mixed_targets(xs, ys, zs, max(NPTS)), [(xs[len(xs) // 2], ys[len(ys) // 3], zs + 0.07)]])
    P[2], P[-1] = P[-1].copy(), P[2].copy()                 # (among the first 63 as well; target 2 moves to the end)
    well_apart(xs, ys, P[:, 0], P[:, 1])
    assert ((P[2, 0] - xs) == 0).any() and ((P[2, 1] - ys) == 0).any() and P[2, 2] > zs
    return xs, ys, zs, bz, P


def capped(got, want, mag, c0, what):
    """NaN where the model has NaN, and elsewhere within (2 c0 + 16) eps M; returns the largest gap / (eps M)"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    fin = np.isfinite(want)
    with np.errstate(all="ignore"):
        ratio = np.where(fin & (mag > 0), np.abs(got - want) / (EPS * mag), np.where(fin & (got != want), np.inf, 0.0))
    worst = float(ratio.max())
    print("%s: device gap %.3g eps M, c0 %.3g, cap %.3g" % (what, worst, c0, 2 * c0 + 16))
    assert worst <= 2 * c0 + 16, (what, worst, c0)
    return worst


def model_with_c0(xs, ys, zs, bz, alpha, X, Y, Z):
    """(sums (3,nt) in float64, M (3,nt), c0): c0 the float64 model's largest gap to the np.longdouble model in eps M"""
    sums, mag = lm.lfff_sums(xs, ys, zs, bz, alpha, X, Y, Z, with_abs=True)
    ext = lm.lfff_sums(xs, ys, zs, bz, alpha, X, Y, Z, dtype=np.longdouble)
    with np.errstate(all="ignore"):
        gap = np.where(mag > 0, np.abs(sums - ext).astype(np.float64) / (EPS * mag), 0.0)
    return sums, mag, float(np.nanmax(gap))


def apply_plane(sums, xs, ys, zs, bz, X, Y, Z):
    out = sums.copy()
    w = Z - zs
    out[2] = np.where(w == 0.0, gm.plane_bz(xs, ys, bz, X, Y), out[2])
    out[:, w < 0.0] = np.nan
    return out


# the targets the model is run at under the largest source (a quarter of a million pixels, twice, once in long
# doubles): two of each kind, the three around a wavefront, and the last of the first block of 256 with the two of the
# second one.  The device is always run at all 258; test_points_do_not_depend_on_their_number_or_order and the
# alpha = 0 tests tie the others to these
FEW = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 62, 63, 64, 255, 256, 257]


@functools.lru_cache(maxsize=None)
def points_case(ns, alpha):
    """the source, 258 targets, the targets sel the model is run at, the model's field (len(sel),3), M (len(sel),3) and
    c0: computed once per source and alpha"""
    xs, ys, zs, bz, P = targets(ns)
    sel = np.array(FEW if ns[0] * ns[1] > 65 * 64 else range(len(P)))
    Q = P[sel]
    sums, mag, c0 = model_with_c0(xs, ys, zs, bz, alpha, Q[:, 0], Q[:, 1], Q[:, 2])
    want = apply_plane(sums, xs, ys, zs, bz, Q[:, 0], Q[:, 1], Q[:, 2]).T.copy()
    mag = mag.T.copy()
    mag[Q[:, 2] == zs, 2] = 0.0                              # Bz on the plane is the interpolation: equal bits
    for a in (P, want, mag):
        a.setflags(write=False)
    return xs, ys, zs, bz, P, sel, want, mag, c0


# ---- alpha = 0: the Green's-function entries bit for bit ----

@pytest.mark.parametrize("ns", SOURCES, ids=IDS)
def test_alpha_zero_points_equal_green_points(hip, ns):
    xs, ys, zs, bz, P = targets(ns)
    for npts in NPTS + [len(P)]:
        want = hip.green_field_points(xs, ys, zs, bz, P[:npts])
        for device in (False, True):
            got = hip.lfff_field_points(xs, ys, zs, bz, 0.0, P[:npts], device=device)
            assert np.array_equal(np.isnan(got), np.isnan(want))
            fin = ~np.isnan(want)
            bits(got[fin], want[fin], (ns, npts, device))
            got = hip.lfff_field_points(xs, ys, zs, bz, -0.0, P[:npts], device=device)
            bits(got[fin], want[fin], (ns, npts, device, "-0.0"))


@pytest.mark.parametrize("on_plane", (True, False), ids=("z0=zs", "z0>zs"))
@pytest.mark.parametrize("n3", BOXES, ids=IDS)
def test_alpha_zero_box_equals_green_box(hip, n3, on_plane):
    x, y, z = box_mesh(n3, on_plane)
    xs, ys, zs, bz = box_source()
    for which in ("faces", "volume"):
        want = hip.magnetogram_field(x, y, z, bz, xs, ys, zs, which=which)
        assert np.isfinite(want).all()
        for device in (False, True):
            bits(hip.linear_force_free_field(x, y, z, bz, 0.0, xs, ys, zs, which=which, device=device), want,
                 (n3, which, device))


# ---- alpha != 0: the model within the cap ----

@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("ns", SOURCES, ids=IDS)
def test_points_stay_within_the_cap(hip, ns, alpha):
    xs, ys, zs, bz, P, sel, want, mag, c0 = points_case(ns, alpha)
    assert np.isnan(want[3]).all() and np.isfinite(want[[0, 1, 2, 4]]).all()
    assert np.abs(want[np.isfinite(want)]).max() > 0
    for npts in NPTS + [len(P)]:
        k = int((sel < npts).sum())                          # (sel ascends)
        for device in (False, True):
            got = hip.lfff_field_points(xs, ys, zs, bz, alpha, P[:npts], device=device)
            capped(got[sel[:k]], want[:k], mag[:k], c0,
                   "source %s alpha %g npts %d device %s" % (IDS(ns), alpha, npts, device))


@pytest.mark.parametrize("ns", [(65, 64), (513, 512)], ids=IDS)
def test_points_do_not_depend_on_their_number_or_order(hip, ns):
    xs, ys, zs, bz, P = targets(ns)
    ref = hip.lfff_field_points(xs, ys, zs, bz, 3.0, P)
    fin = ~np.isnan(ref)
    perm = np.random.default_rng(0).permutation(len(P))
    bits(hip.lfff_field_points(xs, ys, zs, bz, 3.0, P[perm])[fin[perm]], ref[perm][fin[perm]], "permuted")
    bits(hip.lfff_field_points(xs, ys, zs, bz, 3.0, P[200:201]), ref[200:201], "one of many")
    for npts in NPTS:
        got = hip.lfff_field_points(xs, ys, zs, bz, 3.0, P[:npts], device=True)
        bits(got[fin[:npts]], ref[:npts][fin[:npts]], npts)


def test_no_points_touch_nothing(hip):
    xs, ys, zs, bz = source((5, 4))
    assert hip.lfff_field_points(xs, ys, zs, bz, 3.0, np.zeros((0, 3))).shape == (0, 3)
    assert hip.lfff_field_points(xs, ys, zs, bz, 3.0, np.zeros((0, 3)), device=True).shape == (0, 3)


# ---- structure, bit for bit at alpha = 3 ----

@functools.lru_cache(maxsize=None)
def box_case(n3, on_plane):
    x, y, z = box_mesh(n3, on_plane)
    xs, ys, zs, bz = box_source()
    Zg, Yg, Xg = (g.reshape(-1) for g in np.meshgrid(z, y, x, indexing="ij"))
    well_apart(xs, ys, Xg[:len(x) * len(y)], Yg[:len(x) * len(y)])
    sums, mag, c0 = model_with_c0(xs, ys, zs, bz, 3.0, Xg, Yg, Zg)
    shape = (3, len(z), len(y), len(x))
    want = apply_plane(sums, xs, ys, zs, bz, Xg, Yg, Zg).reshape(shape)
    mag = mag.copy()
    mag[2, Zg == zs] = 0.0
    return want, mag.reshape(shape), c0


@pytest.mark.parametrize("on_plane", (True, False), ids=("z0=zs", "z0>zs"))
@pytest.mark.parametrize("n3", BOXES, ids=IDS)
def test_box_faces_volume_and_points_agree(hip, n3, on_plane):
    x, y, z = box_mesh(n3, on_plane)
    xs, ys, zs, bz = box_source()
    assert xs[0] < x[0] and xs[-1] > x[-1] and ys[0] < y[0] and ys[-1] > y[-1]
    want, mag, c0 = box_case(n3, on_plane)
    assert np.isfinite(want).all()
    mask = gm.face_mask(want.shape[1:])
    Zg, Yg, Xg = np.meshgrid(z, y, x, indexing="ij")
    pts = hip.lfff_field_points(xs, ys, zs, bz, 3.0, np.array([Xg[mask], Yg[mask], Zg[mask]]).T)
    first = None
    for device in (False, True):
        vol = hip.linear_force_free_field(x, y, z, bz, 3.0, xs, ys, zs, which="volume", device=device)
        if first is None:
            first = vol
            capped(vol, want, mag, c0, "box %s on_plane %s" % (IDS(n3), on_plane))
            assert np.abs(vol - hip.magnetogram_field(x, y, z, bz, xs, ys, zs, which="volume")).max() > 1e-3   # not alpha = 0
        bits(vol, first, ("volume", n3, device))
        faces = hip.linear_force_free_field(x, y, z, bz, 3.0, xs, ys, zs, which="faces", device=device)
        bits(faces[:, mask], vol[:, mask], ("faces", n3, device))
        assert not faces[:, ~mask].any()                       # zeros inside
        bits(pts.T.copy(), faces[:, mask], ("points", n3, device))
    if on_plane:
        bits(first[2, 0], gm.plane_bz(xs, ys, bz, Xg[0], Yg[0]), "the plane's Bz")


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_points_past_one_chunk(hip, device):
    """262144 + 300 points under a six-pixel source: a second launch whose targets start at 262144 and whose slice sums
    reuse the first launch's scratch; all targets differ"""
    xs, ys, zs, bz = tiny_source()
    n = CHUNK + 300
    rng = np.random.default_rng(21)
    P = np.array([rng.uniform(0.0, 1.2, n), rng.uniform(-0.8, 0.4, n), zs + rng.uniform(0.001, 0.5, n)]).T
    t = np.arange(n)
    P[t % 5 == 1, 2] = zs
    P[t % 7 == 3, 2] -= 0.6
    well_apart(xs, ys, P[:, 0], P[:, 1])
    sums, mag, c0 = model_with_c0(xs, ys, zs, bz, 3.0, P[:, 0], P[:, 1], P[:, 2])
    want = apply_plane(sums, xs, ys, zs, bz, P[:, 0], P[:, 1], P[:, 2]).T.copy()
    mag = mag.T.copy()
    mag[P[:, 2] == zs, 2] = 0.0
    got = hip.lfff_field_points(xs, ys, zs, bz, 3.0, P, device=device)
    capped(got, want, mag, c0, "points past one chunk, device %s" % device)
    again = hip.lfff_field_points(xs, ys, zs, bz, 3.0, P, device=device)
    fin = ~np.isnan(got)
    bits(again[fin], got[fin], "a second call")
    assert not np.array_equal(got[:300], got[CHUNK:])


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("n3,which", (((65, 65, 63), "volume"), ((2, 365, 361), "faces")), ids=("volume", "faces"))
def test_box_past_one_chunk(hip, n3, which, device):
    nx, ny, nz = n3
    assert nx * ny * nz > CHUNK and (nx * ny * nz - CHUNK) % 256 != 0
    x, y, z = 0.31 + np.linspace(0.0, 0.7, nx), -0.55 + np.linspace(0.0, 0.8, ny), 0.25 + np.linspace(0.0, 0.6, nz)
    xs, ys, zs, bz = tiny_source()
    Zg, Yg, Xg = (g.reshape(-1) for g in np.meshgrid(z, y, x, indexing="ij"))
    well_apart(xs, ys, Xg[:nx * ny], Yg[:nx * ny])
    sums, mag, c0 = model_with_c0(xs, ys, zs, bz, 3.0, Xg, Yg, Zg)
    shape = (3, nz, ny, nx)
    want = apply_plane(sums, xs, ys, zs, bz, Xg, Yg, Zg).reshape(shape)
    mag = mag.copy()
    mag[2, Zg == zs] = 0.0
    assert which == "volume" or gm.face_mask(shape[1:]).all()
    got = hip.linear_force_free_field(x, y, z, bz, 3.0, xs, ys, zs, which=which, device=device)
    capped(got, want, mag.reshape(shape), c0, "box past one chunk %s device %s" % (which, device))
    bits(hip.linear_force_free_field(x, y, z, bz, 3.0, xs, ys, zs, which=which, device=device), got, "a second call")


# ---- caller arrays ----

def lfff_box_raw(L, src, mesh, alpha, which, B, device):
    """the raw entry on B (flat, as the caller holds it): host, or device through an arena of offset arrays with NaN
    bands beside bz and B (the arena checks its guards); returns (rc, B afterwards)"""
    xs, ys, zs, bz = src
    x, y, z = mesh
    ns2, n3 = np.array([len(xs), len(ys)], dtype=np.intc), np.array([len(x), len(y), len(z)], dtype=np.intc)
    head = (ns2.ctypes.data_as(_ip), xs.ctypes.data_as(_dp), ys.ctypes.data_as(_dp), zs)
    tail = (n3.ctypes.data_as(_ip), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), z.ctypes.data_as(_dp), which)
    S = np.ascontiguousarray(bz).reshape(-1)
    if not device:
        out = B.copy()
        return L.ndsm_hip_lfff_box(*head, S.ctypes.data, alpha, *tail, out.ctypes.data), out
    arena = Arena(LibTransport(L), [slot("bz", S, field=True), slot("B", B, output=True, field=True)])
    _, out = arena.run(lambda dS, dB: L.ndsm_hip_lfff_box_device(*head, dS, alpha, *tail, dB))
    return arena.rc, out


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("n3", BOXES[1:], ids=IDS)
def test_box_host_equals_device_on_offset_arrays(hip, n3, which):
    L = hip.load_library()
    mesh, src = box_mesh(n3, True), box_source()
    n = int(np.prod(n3))
    B = np.full(3 * n, np.nan)                              # the sentinel the interior keeps for which = 0
    rc_h, host = lfff_box_raw(L, src, mesh, 3.0, which, B, False)
    rc_d, dev = lfff_box_raw(L, src, mesh, 3.0, which, B, True)
    assert rc_h == 0 and rc_d == 0
    bits(dev, host, (n3, which))
    mask = np.broadcast_to(gm.face_mask(n3[::-1]), (3,) + tuple(n3[::-1])).reshape(-1)
    if which == 0:
        assert np.isnan(host[~mask]).all() and np.isfinite(host[mask]).all()
    else:
        assert np.isfinite(host).all()
    vol = hip.linear_force_free_field(*mesh, src[3], 3.0, src[0], src[1], src[2], which="volume").reshape(-1)
    bits(host[mask], vol[mask], "the wrapper's volume")


@pytest.mark.parametrize("npts", (1, 65, 257))
def test_points_host_equals_device_on_offset_arrays(hip, npts):
    L = hip.load_library()
    xs, ys, zs, bz, P = targets((65, 64))
    ref = hip.lfff_field_points(xs, ys, zs, bz, 3.0, P[:npts])
    P = np.ascontiguousarray(P[:npts]).reshape(-1)
    ns2 = np.array([len(xs), len(ys)], dtype=np.intc)
    head = (ns2.ctypes.data_as(_ip), xs.ctypes.data_as(_dp), ys.ctypes.data_as(_dp), zs)
    S = np.ascontiguousarray(bz).reshape(-1)
    host = np.full(3 * npts, 7.0)
    assert L.ndsm_hip_lfff_points(*head, S.ctypes.data, 3.0, npts, P.ctypes.data, host.ctypes.data) == 0
    arena = Arena(LibTransport(L), [slot("bz", S, field=True), slot("pts", P, field=True),
                                    slot("B", np.full(3 * npts, 7.0), output=True)])
    _, _, dev = arena.run(lambda dS, dP, dB: L.ndsm_hip_lfff_points_device(*head, dS, 3.0, npts, dP, dB))
    assert arena.rc == 0
    fin = ~np.isnan(host)
    assert np.array_equal(np.isnan(dev), np.isnan(host))
    bits(dev[fin], host[fin], npts)
    bits(host[fin], ref.reshape(-1)[fin], "the wrapper")


# ---- errors ----

def test_error_codes_leave_the_outputs_untouched(hip):
    L = hip.load_library()
    xs, ys, zs, bz = source((5, 4))
    S = np.ascontiguousarray(bz).reshape(-1)
    x, y, z = box_mesh((3, 3, 3), True)
    P = np.ascontiguousarray(mixed_targets(xs, ys, zs, 4)).reshape(-1)
    nan, inf = float("nan"), float("inf")

    def ip(v):
        return None if v is None else np.array(v, dtype=np.intc).ctypes.data_as(_ip)

    def dp(v):
        return None if v is None else v.ctypes.data_as(_dp)

    def vp(v):
        return None if v is None else v.ctypes.data

    def points(device, ns=(5, 4), sx=xs, sy=ys, s=S, al=3.0, npts=4, pts=P, out=True):
        B = np.full(12, 3.25)
        fn = L.ndsm_hip_lfff_points_device if device else L.ndsm_hip_lfff_points
        rc = fn(ip(ns), dp(sx), dp(sy), zs, vp(s), al, npts, vp(pts), vp(B) if out else None)
        assert (B == 3.25).all()
        return rc

    def box(device, ns=(5, 4), sx=xs, sy=ys, s=S, al=3.0, n3=(3, 3, 3), mx=x, my=y, mz=z, which=0, zs_=zs, out=True):
        B = np.full(81, 3.25)
        fn = L.ndsm_hip_lfff_box_device if device else L.ndsm_hip_lfff_box
        rc = fn(ip(ns), dp(sx), dp(sy), zs_, vp(s), al, ip(n3), dp(mx), dp(my), dp(mz), which, vp(B) if out else None)
        assert (B == 3.25).all()
        return rc

    flat, back = np.array([1.0, 1.0, 2.0, 3.0, 4.0]), xs[::-1].copy()
    for device in (False, True):
        # (device: the value and NULL checks come before any array is looked at, so host addresses do no harm)
        for kw in (dict(ns=None), dict(sx=None), dict(sy=None), dict(s=None), dict(pts=None), dict(out=False),
                   dict(ns=None, al=nan)):                   # (9002 comes before 9004)
            assert points(device, **kw) == 9002, (device, kw)
        for kw in (dict(ns=(1, 4)), dict(ns=(5, 1)), dict(sx=flat), dict(sx=back), dict(sy=np.zeros(4)), dict(npts=-1),
                   dict(sx=np.array([0.0, np.nan, 2, 3, 4])), dict(al=nan), dict(al=inf), dict(al=-inf),
                   dict(al=nan, npts=0)):
            assert points(device, **kw) == 9004, (device, kw)
        assert points(device, npts=0) == 0 and points(device, npts=0, pts=None, out=False) == 0
        for kw in (dict(ns=None), dict(sx=None), dict(sy=None), dict(s=None), dict(n3=None), dict(mx=None), dict(my=None),
                   dict(mz=None), dict(out=False), dict(out=False, al=inf)):
            assert box(device, **kw) == 9002, (device, kw)
        for kw in (dict(ns=(1, 4)), dict(ns=(5, 1)), dict(sx=flat), dict(sy=ys[::-1].copy()), dict(which=2), dict(which=-1),
                   dict(n3=(1, 3, 3)), dict(n3=(3, 1, 3)), dict(n3=(3, 3, 1)), dict(zs_=np.nextafter(z[0], 9.0)),
                   dict(al=nan), dict(al=inf), dict(al=-inf)):
            assert box(device, **kw) == 9004, (device, kw)


# ---- composition ----

def test_the_field_is_accepted_by_helicity(hip):
    """linear_force_free_field(which="volume") is the b of VecPot.helicity; no value is pinned"""
    hx = 0.125
    xs = hx * np.arange(-24, 25)
    x, z = xs[16:33].copy(), hx * np.arange(9)
    Ys, Xs = np.meshgrid(xs, xs, indexing="ij")
    bz = lm.gauss_pair(Xs, Ys)
    b = hip.linear_force_free_field(x, x, z, bz, 1.0, xs=xs, ys=xs, zs=0.0, which="volume")
    assert b.shape == (3, 9, 17, 17) and np.isfinite(b).all()
    bits(b[2, 0], bz[16:33, 16:33], "the magnetogram on the plane")
    V = hip.VecPot(x, x, z)
    try:
        H = V.helicity(b)
        assert H.ierr in (0, 1)
        assert np.isfinite(H.recon_rms) and np.isfinite(H.divB_max) and np.isfinite(H.H_R)
    finally:
        V.close()
