"""The constant-alpha force-free field of the half space above a magnetogram in numpy (semantics: include/ndsm_hip.h,
ndsm_hip_lfff_points), in the order the library sums in: vectorised over the targets and over the slices, sequential
over the pixels of a slice, the slice sums then folded in ascending order (green_model's frame with the richer pair
term).  numpy's elementwise +, *, / and sqrt are IEEE operations that nothing contracts; its sin and cos are the host
library's, not the device's, so at alpha != 0 the device agrees to a rounding bound and not to the bit.  `dtype`
np.longdouble runs the same lines in extended precision: the yardstick of the float64 model's own rounding error."""
import numpy as np

import green_model as gm


def closed_form(alpha, x, y, z):
    """(3, ...) Chiu & Hilton's kernel G for the C = 0 family at the offsets x, y (not both 0) and the height z > 0,
    written out from Gamma = [z cos(alpha r) / r - cos(alpha z)] / (2 pi R):
    Gx = (x / R) dGamma/dz + alpha Gamma y / R, Gy = (y / R) dGamma/dz - alpha Gamma x / R,
    Gz = z [cos(alpha r) / r^3 + alpha sin(alpha r) / r^2] / (2 pi)"""
    x, y, z = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (x, y, z)))
    R = np.sqrt(x * x + y * y)
    r = np.sqrt(x * x + y * y + z * z)
    cr, sr = np.cos(alpha * r), np.sin(alpha * r)
    gam = (z * cr / r - np.cos(alpha * z)) / (2 * np.pi * R)
    dgam = (cr / r - z * z * cr / r ** 3 - alpha * z * z * sr / r ** 2 + alpha * np.sin(alpha * z)) / (2 * np.pi * R)
    gx = (x / R) * dgam + alpha * gam * y / R
    gy = (y / R) * dgam - alpha * gam * x / R
    gz = z * (cr / r ** 3 + alpha * sr / r ** 2) / (2 * np.pi)
    return np.array([gx, gy, gz])


def lfff_sums(xs, ys, zs, bz, alpha, X, Y, Z, with_abs=False, dtype=np.float64):
    """(3, nt): the sums of the header's terms over all pixels for the targets X, Y, Z (nt), whatever w = Z - zs is.
    bz (nsy, nsx).  with_abs: also M (3, nt), the scale of the rounding error per component - per pair (1 + |ar|) times
    the sum of the absolute products of each addend, with every sine and cosine counted as 1 (their errors are
    absolute: 4 ulp of a value up to 1, and eps |ar| from the rounding of the argument): for Sx
    |dx t| + |u| (|dx| (1 + ww / r2) + |dy| (|w| / r + 1)), likewise Sy, and for Sz |w t| (1 + |ar|)."""
    T = dtype
    xs, ys = np.asarray(xs, dtype=np.float64).astype(T), np.asarray(ys, dtype=np.float64).astype(T)
    X, Y, Z = (np.asarray(v, dtype=np.float64).reshape(-1).astype(T) for v in (X, Y, Z))
    alpha, zs = T(alpha), T(zs)
    nsx, nsy = len(xs), len(ys)
    assert np.shape(bz) == (nsy, nsx)
    npix = nsx * nsy
    c = ((xs[1] - xs[0]) * (ys[1] - ys[0])) / T(gm.TWO_PI)
    ns, ln = gm.slices(npix)
    p = np.arange(ns * ln)
    real = p < npix
    pc = np.where(real, p, 0)
    q = np.where(real, np.asarray(bz, dtype=np.float64).astype(T).reshape(-1)[pc] * c, T(0)).reshape(ns, ln)
    sx, sy = xs[pc % nsx].reshape(ns, ln), ys[pc // nsx].reshape(ns, ln)
    real = real.reshape(ns, ln)
    w = (Z - zs)[None, :]
    ww = w * w
    sz, cz = np.sin(alpha * w), np.cos(alpha * w)
    acc = np.zeros((3, ns, len(X)), dtype=T)
    mag = np.zeros((3, len(X)), dtype=T)
    with np.errstate(all="ignore"):
        for n in range(ln):
            qn = q[:, n, None]
            dx = X[None, :] - sx[:, n, None]
            dy = Y[None, :] - sy[:, n, None]
            R2 = dx * dx + dy * dy
            r2 = R2 + ww
            on = (r2 > 0) & real[:, n, None]               # the punctured rule: no term at all
            on2 = on & (R2 > 0)
            r = np.sqrt(r2)
            t = qn / (r2 * r)
            ar = alpha * r
            cr, sr = np.cos(ar), np.sin(ar)
            acc[0] = np.where(on, acc[0] + (dx * t) * cr, acc[0])
            acc[1] = np.where(on, acc[1] + (dy * t) * cr, acc[1])
            acc[2] = np.where(on, acc[2] + (w * t) * (cr + ar * sr), acc[2])
            u = alpha * (qn / R2)
            e = sz - (ww / r2) * sr
            f = (w / r) * cr - cz
            acc[0] = np.where(on2, acc[0] + u * (dx * e + dy * f), acc[0])
            acc[1] = np.where(on2, acc[1] + u * (dy * e - dx * f), acc[1])
            if with_abs:
                k = 1 + np.abs(ar)
                au, ae, af = np.abs(u), 1 + ww / r2, np.abs(w) / r + 1
                adx, ady, at = np.abs(dx), np.abs(dy), np.abs(t)
                mag[0] += (np.where(on, k * adx * at, 0) + np.where(on2, k * au * (adx * ae + ady * af), 0)).sum(axis=0)
                mag[1] += (np.where(on, k * ady * at, 0) + np.where(on2, k * au * (ady * ae + adx * af), 0)).sum(axis=0)
                mag[2] += np.where(on, k * np.abs(w) * at * k, 0).sum(axis=0)
        out = acc[:, 0, :].copy()
        for s in range(1, ns):
            out = out + acc[:, s, :]
    return (out, mag) if with_abs else out


def lfff_targets(xs, ys, zs, bz, alpha, X, Y, Z):
    """(3, nt): the field at the targets with the rules of the plane applied (green_model's)"""
    X, Y, Z = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (X, Y, Z))
    out = lfff_sums(xs, ys, zs, bz, alpha, X, Y, Z)
    w = Z - zs
    out[2] = np.where(w == 0.0, gm.plane_bz(xs, ys, bz, X, Y), out[2])
    out[:, w < 0.0] = np.nan
    return out


def lfff_points(xs, ys, zs, bz, alpha, pts):
    """B (npts, 3) at pts (npts, 3)"""
    P = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    return lfff_targets(xs, ys, zs, bz, alpha, P[:, 0], P[:, 1], P[:, 2]).T.copy()


def lfff_box(x, y, z, bz, alpha, xs=None, ys=None, zs=None, which="volume", fill=0.0):
    """b (3, nz, ny, nx) on the box mesh; which "faces": the face nodes, `fill` inside; "volume": every node"""
    x, y, z = (np.asarray(v, dtype=np.float64) for v in (x, y, z))
    xs, ys = x if xs is None else xs, y if ys is None else ys
    zs = z[0] if zs is None else zs
    shape = (len(z), len(y), len(x))
    Zg, Yg, Xg = np.meshgrid(z, y, x, indexing="ij")
    sel = gm.face_mask(shape) if which == "faces" else np.ones(shape, dtype=bool)
    b = np.full((3,) + shape, fill, dtype=np.float64)
    b[:, sel] = lfff_targets(xs, ys, zs, bz, alpha, Xg[sel], Yg[sel], Zg[sel])
    return b


def gauss_pair(X, Y, width=0.3):
    """two Gaussians of opposite sign at (0.3, 0.1) and (-0.3, -0.1): a flux-balanced bipole"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    return (np.exp(-((X - 0.3) ** 2 + (Y - 0.1) ** 2) / width) - np.exp(-((X + 0.3) ** 2 + (Y + 0.1) ** 2) / width))
