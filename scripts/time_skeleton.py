"""The skeleton entry on device-resident arrays, timed with device events, against the paths entry on the same seeds:
usage time_skeleton.py [--repeats R] [--nring K] [--max-nulls M] [n ...]
(default 128 256, --nring 16, --max-nulls 1024, --repeats 5)

The protocol of time_trace.py.  Per size n^3, on one VecPot handle: the ABC field (tests/test_gpu_field.py) plus the
white noise of time_nulls.py (about 1 % of the cells candidates), its nulls from ndsm_hip_vecpot_nulls_device - the
raw records, left in device memory and passed straight on, the first M of them -, K fan seeds per null at the default
angles, radius 0.5, step 0.5, the default max_steps, every = 1.  B, the records, the ring and every output stay in
device memory.  Timed
in the same run, each warmed up once and then R times between two events on the library stream, the calls repeated
inside one timed window until it is at least 0.2 s long:
  skel0_count, skel0_fill   the skeleton entry with capture = 0: the counting call (max_points = 0) and the filling call
                            (max_points = total, points and bpt)
  skel_count, skel_fill     the same with capture = 0.5 (the capture loop over all nulls after every step)
  paths_count, paths_fill   ndsm_hip_vecpot_paths_device without G on the skeleton's own seeds (formed on the host by
                            tests/skeleton_model.seeds_numpy, the device's bits): one call per direction, the lanes that
                            run forward and those that run backward, the two times added
Reported per variant: the median time of one call [min, max]; the ratios skel0 / paths (expected about 1: the same
lines) and skel / skel0 (the share of the capture loop, expected to grow with the number of nulls); lines, points and
how the lines ended."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import ndsm_amd  # noqa: E402
from ndsm_amd import _lib  # noqa: E402
from skeleton_model import default_ring, seeds_numpy  # noqa: E402
from test_gpu_field import abc_field  # noqa: E402
from time_nulls import noisy  # noqa: E402

WINDOW_S = 0.2
CAP = 1 << 16
RADIUS, STEP = 0.5, 0.5


def main(sizes, nring=16, repeats=5, max_nulls=1024):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    rows = []
    for n in sizes:
        mesh, b = abc_field([n, n, n])
        b = np.ascontiguousarray(b)
        V = ndsm_amd.VecPot(*mesh)
        max_steps = V.default_max_steps(STEP)
        live = []

        def alloc(nbytes):
            p = ctypes.c_void_p()
            assert L.ndsm_hip_device_alloc(max(nbytes, 8), ctypes.byref(p)) == 0, _lib.last_error(L)
            live.append(p)
            return p

        def up(a):
            a = np.ascontiguousarray(a)
            p = alloc(a.nbytes)
            if a.nbytes:
                assert L.ndsm_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
            return p

        def down(p, a):
            assert L.ndsm_hip_memcpy_d2h(a.ctypes.data, p, a.nbytes) == 0
            return a

        dB = alloc(b.nbytes)
        counts = np.zeros(2, dtype=np.int64)

        def candidates_of(f):
            assert L.ndsm_hip_memcpy_h2d(dB, f.ctypes.data, f.nbytes) == 0
            assert L.ndsm_hip_vecpot_nulls_device(V.h, dB, 0, counts.ctypes.data, *[None] * 7) == 0, _lib.last_error(L)
            return int(counts[0])

        bn, amp = noisy(b, np.random.default_rng(11), candidates_of)
        bn = np.ascontiguousarray(bn)
        assert L.ndsm_hip_memcpy_h2d(dB, bn.ctypes.data, bn.nbytes) == 0
        rec = [alloc(CAP * w) for w in (8, 24, 72, 8, 8, 4, 4)]
        assert L.ndsm_hip_vecpot_nulls_device(V.h, dB, CAP, counts.ctypes.data, *rec) == 0, _lib.last_error(L)
        nn = int(min(counts[1], CAP, max_nulls))
        ring = default_ring(nring)
        dring = up(ring)
        Lm = 2 + nring
        nl = nn * Lm
        pernull = [alloc(4 * nn)] + [alloc(24 * nn) for _ in range(3)]
        lines = [alloc(24 * nl), alloc(8 * nl), alloc(4 * nl), alloc(4 * nl), alloc(4 * nl), alloc(8 * (nl + 1))]
        total = np.zeros(1, dtype=np.int64)

        def skel(capture, cap, pts):
            rc = L.ndsm_hip_vecpot_skeleton_device(V.h, dB, nn, rec[1], rec[2], nring, dring, RADIUS, capture, STEP,
                                                   max_steps, 1, cap, *pernull, *lines, total.ctypes.data, *pts)
            assert rc == 0, _lib.last_error(L)

        # the same seeds for the paths entry, one call per direction
        pos, jac = down(rec[1], np.zeros((nn, 3))), down(rec[2], np.zeros((nn, 3, 3)))
        _pernull, seeds, sgn = seeds_numpy(mesh, pos, jac, ring, RADIUS)
        groups = []
        for sg in (1, -1):
            S = np.ascontiguousarray(seeds[sgn == sg])
            k = len(S)
            groups.append((sg, k, up(S), [alloc(24 * k), alloc(8 * k), alloc(8 * k), alloc(4 * k), alloc(4 * k),
                                          alloc(8 * (k + 1))]))
        ptotal = np.zeros(1, dtype=np.int64)

        def paths(fill):
            for sg, k, dS, out in groups:
                if k == 0:
                    continue
                cap, pts = (0, [None] * 4) if not fill else (fill[sg][0], [fill[sg][1], fill[sg][2], None, None])
                rc = L.ndsm_hip_vecpot_paths_device(V.h, dB, None, k, dS, STEP, max_steps, sg, 1, cap, *out,
                                                    ptotal.ctypes.data, *pts)
                assert rc == 0, _lib.last_error(L)

        def timed(fn, count):
            assert L.ndsm_hip_timer_start() == 0
            for _ in range(count):
                fn()
            ms = ctypes.c_double(0)
            assert L.ndsm_hip_timer_stop(ctypes.byref(ms)) == 0
            return ms.value * 1e-3 / count

        def measure(fn):
            fn()                                              # warm-up
            first = timed(fn, 1)
            count = max(1, int(np.ceil(WINDOW_S / first)))
            ts = sorted(timed(fn, count) for _ in range(repeats))
            return float(np.median(ts)), ts[0], ts[-1]

        row = {"n": n, "noise_amplitude": round(amp, 4), "nulls_found": int(counts[1]), "nulls": nn, "nring": nring,
               "lines": nl, "max_steps": max_steps}
        variants = []
        for tag, capture in (("skel0", 0.0), ("skel", 0.5)):
            skel(capture, 0, [None, None])
            npts = int(total[0])
            pts = [alloc(24 * npts), alloc(24 * npts)]
            row[tag + "_points"] = npts
            variants += [(tag + "_count", lambda c=capture: skel(c, 0, [None, None])),
                         (tag + "_fill", lambda c=capture, k=npts, p=pts: skel(c, k, p))]
        fill = {}
        for sg, k, dS, out in groups:
            if k == 0:
                continue
            rc = L.ndsm_hip_vecpot_paths_device(V.h, dB, None, k, dS, STEP, max_steps, sg, 1, 0, *out,
                                                ptotal.ctypes.data, *[None] * 4)
            assert rc == 0, _lib.last_error(L)
            fill[sg] = (int(ptotal[0]), alloc(24 * int(ptotal[0])), alloc(24 * int(ptotal[0])))
        row["paths_points"] = sum(v[0] for v in fill.values())
        variants += [("paths_count", lambda: paths(None)), ("paths_fill", lambda: paths(fill))]
        for tag, fn in variants:
            med, lo, hi = measure(fn)
            row.update({tag + "_ms": round(med * 1e3, 3), tag + "_min_ms": round(lo * 1e3, 3),
                        tag + "_max_ms": round(hi * 1e3, 3)})
        skel(0.5, 0, [None, None])
        status = down(lines[2], np.zeros(nl, dtype=np.int32))
        kind = down(pernull[0], np.zeros(nn, dtype=np.int32))
        row["status_counts"] = {int(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))}
        row["kind_counts"] = {int(k): int(v) for k, v in zip(*np.unique(kind, return_counts=True))}
        both = lambda t: row[t + "_count_ms"] + row[t + "_fill_ms"]   # noqa: E731
        row["skel0_over_paths"] = round(both("skel0") / both("paths"), 3)
        row["skel_over_skel0"] = round(both("skel") / both("skel0"), 3)
        for p in live:
            L.ndsm_hip_device_free(p)
        V.close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--repeats": "5", "--nring": "16", "--max-nulls": "1024"}
    for o in list(opts):
        if o in args:
            i = args.index(o)
            opts[o] = args[i + 1]
            del args[i:i + 2]
    main([int(a) for a in args] or [128, 256], nring=int(opts["--nring"]), repeats=int(opts["--repeats"]),
         max_nulls=int(opts["--max-nulls"]))
