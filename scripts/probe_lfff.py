"""The constant-alpha force-free field of a magnetogram against the potential field on the same inputs, timed with
device events in one run:
usage probe_lfff.py [--repeats R] [--box N] [--source M] [--alpha A]   (default --repeats 5 --box 128 --source 768 --alpha 2)

probe_green.py's set-up and protocol: an N^3 box on [-1, 1]^2 x [0, 2] whose x and y are a slice of the M x M source
mesh of the same spacing (the B_z of a pair of submerged monopoles as the magnetogram), arrays resident in device
memory.  A timed window - between two events on the library stream - holds K calls of one kind, K chosen after one
warm-up call so that a window is at least 0.2 s long; the kinds alternate window by window, R windows each:
  faces    ndsm_hip_{lfff,green}_box_device, which = 0: the face nodes
  volume   the same with which = 1: all N^3 nodes
  points   ndsm_hip_{lfff,green}_points_device on 65536 of the face nodes
Reported per kind and entry: median, min and max per call, the pair terms (targets x pixels) per second of the median,
and the ratio of the two medians.  The entries allocate and free their scratch and copy five mesh vectors per call;
that is inside the window."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import ndsm_amd  # noqa: E402
from ndsm_amd import _lib  # noqa: E402
from probe_green import WINDOW_S, face_mask, monopole_bz, timed, stats  # noqa: E402

_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--box", type=int, default=128)
    ap.add_argument("--source", type=int, default=768)
    ap.add_argument("--alpha", type=float, default=2.0)
    a = ap.parse_args()
    n, m, alpha = a.box, a.source, a.alpha
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
    mesh = (n3.ctypes.data_as(_ip), x.ctypes.data_as(_dp), x.ctypes.data_as(_dp), z.ctypes.data_as(_dp))

    def box(lfff, which):
        if lfff:
            return lambda: _lib._check(L.ndsm_hip_lfff_box_device(*head, alpha, *mesh, which, dev["B"]), "lfff_box_device", L)
        return lambda: _lib._check(L.ndsm_hip_green_box_device(*head, *mesh, which, dev["B"]), "green_box_device", L)

    def points(lfff):
        if lfff:
            return lambda: _lib._check(L.ndsm_hip_lfff_points_device(*head, alpha, npts, dev["P"], dev["BP"]),
                                       "lfff_points_device", L)
        return lambda: _lib._check(L.ndsm_hip_green_points_device(*head, npts, dev["P"], dev["BP"]), "green_points_device", L)

    kinds = {}
    for name, lfff in (("lfff", True), ("potential", False)):
        kinds["faces " + name] = (box(lfff, 0), int(mask.sum()))
        kinds["volume " + name] = (box(lfff, 1), n ** 3)
        kinds["points " + name] = (points(lfff), npts)
    reps, times = {}, {k: [] for k in kinds}
    for k, (fn, _) in kinds.items():
        fn()                                                     # warm-up: code objects, first allocation
        reps[k] = max(1, int(np.ceil(WINDOW_S / max(timed(L, fn), 1e-6))))
    for _ in range(a.repeats):
        for k, (fn, _) in kinds.items():
            times[k].append(timed(L, lambda: [fn() for _ in range(reps[k])]) / reps[k])
    out = {"box": n, "source": m, "alpha": alpha, "repeats": a.repeats}
    for k, (_, nt) in kinds.items():
        out[k] = dict(stats(times[k]), targets=nt, calls_per_window=reps[k],
                      pair_terms_per_s=float("%.4g" % (nt * m * m / float(np.median(times[k])))))
    for g in ("faces", "volume", "points"):
        out[g + " lfff / potential"] = float("%.3g" % (out[g + " lfff"]["median_ms"] / out[g + " potential"]["median_ms"]))
    for p in dev.values():
        L.ndsm_hip_device_free(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
