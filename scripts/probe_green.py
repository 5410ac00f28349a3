"""The Green's-function field of a magnetogram on the faces of a box, timed with device events in one run:
usage probe_green.py [--repeats R] [--box N] [--source M]   (default --repeats 5 --box 128 --source 768)

An N^3 box on [-1, 1]^2 x [0, 2] whose x and y are a slice of the M x M source mesh of the same spacing (the B_z of a
pair of submerged monopoles as the magnetogram), arrays resident in device memory.  A timed window - between two events
on the library stream - holds K calls of one kind, K chosen after one warm-up call so that a window is at least 0.2 s
long; the kinds alternate window by window, R windows each:
  faces    ndsm_hip_green_box_device, which = 0: the face nodes
  points   ndsm_hip_green_points_device on 65536 of the same nodes
Reported: median, min and max per call, and the pair terms (targets x pixels) per second of the median.  The entries
allocate and free their scratch and copy five mesh vectors per call; that is inside the window."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import ndsm_amd  # noqa: E402
from ndsm_amd import _lib  # noqa: E402

WINDOW_S = 0.2
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)


def face_mask(shape):
    """(nz, ny, nx) bool: the nodes with an index at either end of an axis"""
    m = np.zeros(shape, dtype=bool)
    m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = (True,) * 6
    return m


def monopole_bz(X, Y, depth=0.3):
    """B_z on the plane z = 0 of two monopoles, +1 at (0.3, 0.1, -depth) and -1 at (-0.3, -0.1, -depth)"""
    bz = np.zeros(X.shape)
    for s, (px, py) in ((1.0, (0.3, 0.1)), (-1.0, (-0.3, -0.1))):
        dx, dy = X - px, Y - py
        bz += s * depth / (dx * dx + dy * dy + depth * depth) ** 1.5
    return bz


def timed(L, fn):
    _lib._check(L.ndsm_hip_timer_start(), "timer_start", L)
    fn()
    ms = ctypes.c_double(0)
    _lib._check(L.ndsm_hip_timer_stop(ctypes.byref(ms)), "timer_stop", L)
    return ms.value * 1e-3


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(float(np.median(ts)) * 1e3, 3), "min_ms": round(ts[0] * 1e3, 3), "max_ms": round(ts[-1] * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--box", type=int, default=128)
    ap.add_argument("--source", type=int, default=768)
    a = ap.parse_args()
    n, m = a.box, a.source
    assert m >= n
    L = ndsm_amd.load_library()
    _lib._check(L.ndsm_hip_init(-1), "init", L)
    h = 2.0 / (n - 1)
    lo = (m - n) // 2
    xs = h * (np.arange(m) - lo) - 1.0
    x, z = xs[lo:lo + n].copy(), h * np.arange(n)
    Ys, Xs = np.meshgrid(xs, xs, indexing="ij")
    bz = np.ascontiguousarray(monopole_bz(Xs, Ys)).reshape(-1)
    mask = face_mask((n, n, n))
    Zg, Yg, Xg = np.meshgrid(z, x, x, indexing="ij")
    P = np.array([Xg[mask], Yg[mask], Zg[mask]]).T[:65536].copy().reshape(-1)
    npts = len(P) // 3
    host = {"bz": bz, "B": np.zeros(3 * n ** 3), "P": P, "BP": np.zeros(3 * npts)}
    dev = {}
    for k, v in host.items():
        dev[k] = ctypes.c_void_p()
        _lib._check(L.ndsm_hip_device_alloc(v.nbytes, ctypes.byref(dev[k])), "device_alloc", L)
        _lib._check(L.ndsm_hip_memcpy_h2d(dev[k], v.ctypes.data, v.nbytes), "h2d", L)
    ns2, n3 = np.array([m, m], dtype=np.intc), np.array([n, n, n], dtype=np.intc)
    head = (ns2.ctypes.data_as(_ip), xs.ctypes.data_as(_dp), xs.ctypes.data_as(_dp), 0.0, dev["bz"])

    def faces():
        _lib._check(L.ndsm_hip_green_box_device(*head, n3.ctypes.data_as(_ip), x.ctypes.data_as(_dp), x.ctypes.data_as(_dp),
                                                z.ctypes.data_as(_dp), 0, dev["B"]), "green_box_device", L)

    def points():
        _lib._check(L.ndsm_hip_green_points_device(*head, npts, dev["P"], dev["BP"]), "green_points_device", L)

    kinds = {"faces": (faces, int(mask.sum())), "points": (points, npts)}
    reps, times = {}, {k: [] for k in kinds}
    for k, (fn, _) in kinds.items():
        fn()                                                     # warm-up: code objects, first allocation
        reps[k] = max(1, int(np.ceil(WINDOW_S / max(timed(L, fn), 1e-6))))
    for _ in range(a.repeats):
        for k, (fn, _) in kinds.items():
            times[k].append(timed(L, lambda: [fn() for _ in range(reps[k])]) / reps[k])
    out = {"box": n, "source": m, "repeats": a.repeats}
    for k, (_, nt) in kinds.items():
        out[k] = dict(stats(times[k]), targets=nt, calls_per_window=reps[k],
                      pair_terms_per_s=float("%.4g" % (nt * m * m / float(np.median(times[k])))))
    for p in dev.values():
        L.ndsm_hip_device_free(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
