"""The Green's-function field of the half space above a magnetogram in numpy (semantics: include/ndsm_hip.h,
ndsm_hip_green_points), in the order the library sums in: vectorised over the targets and over the slices, sequential
over the pixels of a slice, the slice sums then folded in ascending order.  numpy's elementwise +, *, / and sqrt are
IEEE operations that nothing contracts, so the bits are the ones the header states."""
import numpy as np

TWO_PI = 6.283185307179586
SLICE_MIN, SLICE_CAP = 4096, 64


def slices(npix):
    """(NS, len): NS = min(64, ceil(npix / 4096)) slices of len = ceil(npix / NS) pixels, the last one shorter"""
    ns = min(SLICE_CAP, -(-npix // SLICE_MIN))
    return ns, -(-npix // ns)


def slice_ranges(npix):
    ns, ln = slices(npix)
    return [(s * ln, min(npix, (s + 1) * ln)) for s in range(ns)]


def green_sums(xs, ys, zs, bz, X, Y, Z, with_abs=False):
    """(3, nt): the sums of the three terms over all pixels for the targets X, Y, Z (nt), whatever w = Z - zs is.
    bz (nsy, nsx).  with_abs: also (3, nt) sum |term|, added in any order (the scale of the rounding error)."""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    X, Y, Z = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (X, Y, Z))
    nsx, nsy = len(xs), len(ys)
    assert np.shape(bz) == (nsy, nsx)
    npix = nsx * nsy
    c = ((xs[1] - xs[0]) * (ys[1] - ys[0])) / TWO_PI
    ns, ln = slices(npix)
    # pixel p = s * ln + n of slice s, padded to ns * ln with pixels that add nothing
    p = np.arange(ns * ln)
    real = p < npix
    pc = np.where(real, p, 0)
    q = np.where(real, np.asarray(bz, dtype=np.float64).reshape(-1)[pc] * c, 0.0).reshape(ns, ln)
    sx, sy = xs[pc % nsx].reshape(ns, ln), ys[pc // nsx].reshape(ns, ln)
    real = real.reshape(ns, ln)
    w = Z - zs
    ww = w * w
    acc = np.zeros((3, ns, len(X)))
    mag = np.zeros((3, len(X)))
    with np.errstate(all="ignore"):
        for n in range(ln):
            dx = X[None, :] - sx[:, n, None]
            dy = Y[None, :] - sy[:, n, None]
            r2 = (dx * dx + dy * dy) + ww[None, :]
            t = q[:, n, None] / (r2 * np.sqrt(r2))
            on = (r2 > 0.0) & real[:, n, None]          # the punctured rule: no term at all
            for k, d in enumerate((dx, dy, np.broadcast_to(w[None, :], dx.shape))):
                acc[k] = np.where(on, acc[k] + d * t, acc[k])
                if with_abs:
                    mag[k] += np.where(on, np.abs(d * t), 0.0).sum(axis=0)
        out = acc[:, 0, :].copy()
        for s in range(1, ns):
            out = out + acc[:, s, :]
    return (out, mag) if with_abs else out


def lerp(v0, v1, th):
    with np.errstate(all="ignore"):
        mid = (1.0 - th) * v0 + th * v1
    return np.where(th == 0.0, v0, np.where(th == 1.0, v1, mid))


def plane_bz(xs, ys, bz, X, Y):
    """the bilinear interpolation of bz (nsy, nsx) at (X, Y); 0 outside the mesh; a node's value bit for bit on a node"""
    xs, ys, bz = (np.asarray(v, dtype=np.float64) for v in (xs, ys, bz))
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    inside = (X >= xs[0]) & (X <= xs[-1]) & (Y >= ys[0]) & (Y <= ys[-1])
    Xc, Yc = np.where(inside, X, xs[0]), np.where(inside, Y, ys[0])
    i0 = np.clip(np.searchsorted(xs, Xc, side="right") - 1, 0, len(xs) - 2)   # the largest node with xs[i0] <= X
    j0 = np.clip(np.searchsorted(ys, Yc, side="right") - 1, 0, len(ys) - 2)
    tx = (Xc - xs[i0]) / (xs[i0 + 1] - xs[i0])
    ty = (Yc - ys[j0]) / (ys[j0 + 1] - ys[j0])
    a = lerp(bz[j0, i0], bz[j0, i0 + 1], tx)
    b = lerp(bz[j0 + 1, i0], bz[j0 + 1, i0 + 1], tx)
    return np.where(inside, lerp(a, b, ty), 0.0)


def green_targets(xs, ys, zs, bz, X, Y, Z):
    """(3, nt): the field at the targets with the rules of the plane applied"""
    X, Y, Z = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (X, Y, Z))
    out = green_sums(xs, ys, zs, bz, X, Y, Z)
    w = Z - zs
    out[2] = np.where(w == 0.0, plane_bz(xs, ys, bz, X, Y), out[2])
    out[:, w < 0.0] = np.nan
    return out


def green_points(xs, ys, zs, bz, pts):
    """B (npts, 3) at pts (npts, 3)"""
    P = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    return green_targets(xs, ys, zs, bz, P[:, 0], P[:, 1], P[:, 2]).T.copy()


def face_mask(shape):
    """(nz, ny, nx) bool: the nodes with an index at either end of an axis"""
    m = np.zeros(shape, dtype=bool)
    m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = (True,) * 6
    return m


def green_box(x, y, z, bz, xs=None, ys=None, zs=None, which="faces", fill=0.0):
    """b (3, nz, ny, nx) on the box mesh; which "faces": the face nodes, `fill` inside; "volume": every node"""
    x, y, z = (np.asarray(v, dtype=np.float64) for v in (x, y, z))
    xs, ys = x if xs is None else xs, y if ys is None else ys
    zs = z[0] if zs is None else zs
    shape = (len(z), len(y), len(x))
    Zg, Yg, Xg = np.meshgrid(z, y, x, indexing="ij")
    sel = face_mask(shape) if which == "faces" else np.ones(shape, dtype=bool)
    b = np.full((3,) + shape, fill, dtype=np.float64)
    b[:, sel] = green_targets(xs, ys, zs, bz, Xg[sel], Yg[sel], Zg[sel])
    return b


def monopole_pair(X, Y, Z, depth=0.3):
    """(3, ...) the field of two monopoles, +1 at (0.3, 0.1, -depth) and -1 at (-0.3, -0.1, -depth): harmonic in
    z > -depth, B = sum s (r - r_s) / |r - r_s|^3"""
    X, Y, Z = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (X, Y, Z)))
    b = np.zeros((3,) + X.shape)
    for s, (px, py) in ((1.0, (0.3, 0.1)), (-1.0, (-0.3, -0.1))):
        dx, dy, dz = X - px, Y - py, Z + depth
        r3 = (dx * dx + dy * dy + dz * dz) ** 1.5
        b += s * np.array([dx, dy, dz]) / r3
    return b
