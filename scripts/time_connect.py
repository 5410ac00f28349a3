"""The flux partition and the patch connectivity on device-resident arrays, timed with device events:
usage time_connect.py [--repeats R] [--side M] [n ...]   (default 512 1024, --repeats 5, --side 128)

The protocol of time_flow.py: the arrays stay in device memory; each variant is warmed up once and
then timed R times between two events on the library stream; the calls are repeated inside one timed window until it is
at least 0.2 s long.  Reported per variant: median [min - max] of one call.
  partition, partition_count   ndsm_hip_partition_device on n x n white noise U(-1, 1), thr = 0, with room for every patch
                               and with max_patches = 0 (pointers, jumping, numbering and labels, no sort)
  connect                      ndsm_hip_vecpot_connect_device on an M x M x M box, M^2 feet, labels from the partition of
                               its lower face, room for every pair
  connect_keyed                the same call with max_steps = 1: every line is one step long, so what is left is the sort,
                               the runs and the sums on keys of the same width (and the launches)
  trace                        the yardstick, in the same run: ndsm_hip_vecpot_trace_device forward from the same M^2 seeds
                               (a foot with B_z < 0 leaves through the face in its first step: about half the work)
  trace_signed                 the fair yardstick: two calls of it, forward from the feet with B_z > 0 and backward from
                               the feet with B_z < 0 - the lines the connect call walks, in two launches
None of the figures is a bare kernel time."""
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


def main(sizes, repeats=5, side=128):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)

    def timed(fn, calls):
        assert L.ndsm_hip_timer_start() == 0
        for _ in range(calls):
            fn()
        ms = ctypes.c_double(0)
        assert L.ndsm_hip_timer_stop(ctypes.byref(ms)) == 0
        return ms.value * 1e-3 / calls

    def measure(fn):
        fn()                                              # warm-up
        first = timed(fn, 1)
        calls = max(1, int(np.ceil(WINDOW_S / first)))
        ts = sorted(timed(fn, calls) for _ in range(repeats))
        return float(np.median(ts)), ts[0], ts[-1], calls

    def put(row, name, stats):
        med, tmin, tmax, calls = stats
        row.update({name + "_ms": round(med * 1e3, 4), name + "_min_ms": round(tmin * 1e3, 4),
                    name + "_max_ms": round(tmax * 1e3, 4), name + "_calls_per_window": calls})
        return med

    def upload(host):
        dev = {}
        for k, a in host.items():
            dev[k] = ctypes.c_void_p()
            assert L.ndsm_hip_device_alloc(a.nbytes, ctypes.byref(dev[k])) == 0, _lib.last_error(L)
            assert L.ndsm_hip_memcpy_h2d(dev[k], a.ctypes.data, a.nbytes) == 0
        return dev

    def records(m):
        return {"root": np.zeros(m, dtype=np.int64), "sign": np.zeros(m, dtype=np.int32), "npix": np.zeros(m, dtype=np.int64),
                "flux": np.zeros(m), "sx": np.zeros(m), "sy": np.zeros(m)}

    rng = np.random.default_rng(7)
    counts = np.zeros(2, dtype=np.int64)
    for n in sizes:
        xs = ys = 0.1 * np.arange(n)
        ns = np.array([n, n], dtype=np.intc)
        head = (ns.ctypes.data_as(_lib._ip), _lib._d(xs), _lib._d(ys))
        dev = upload(dict({"bz": rng.uniform(-1.0, 1.0, (n, n)), "label": np.zeros((n, n), dtype=np.int32)},
                          **records(n * n)))

        def partition(cap):
            def call():
                rc = L.ndsm_hip_partition_device(*head, dev["bz"], 0.0, cap, counts.ctypes.data, dev["label"],
                                                 *[dev[k] for k in ("root", "sign", "npix", "flux", "sx", "sy")])
                assert rc == 0, _lib.last_error(L)
            return call

        row = {"n": n, "pixels": n * n}
        med = put(row, "partition", measure(partition(n * n)))
        row["patches"] = int(counts[1])
        row["partition_Mpix_per_s"] = round(n * n / med / 1e6, 1)
        put(row, "partition_count", measure(partition(0)))
        for p in dev.values():
            L.ndsm_hip_device_free(p)
        print(json.dumps(row), flush=True)

    m = side
    x = np.linspace(-1.0, 1.0, m)
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
    k = np.pi
    b = np.stack([np.sin(k * Z) + np.cos(k * Y), np.sin(k * X) + np.cos(k * Z), np.sin(k * Y) + np.cos(k * X)])
    V = ndsm_amd.VecPot(x, x, x)
    ns = np.array([m, m], dtype=np.intc)
    head = (ns.ctypes.data_as(_lib._ip), _lib._d(x), _lib._d(x))
    npix = m * m
    seeds = np.stack([np.tile(x, m), np.repeat(x, m), np.full(npix, x[0])], axis=1)
    host = {"B": np.ascontiguousarray(b), "label": np.zeros(npix, dtype=np.int32), "dest": np.zeros(npix, dtype=np.int32),
            "ends": np.zeros((npix, 3)), "length": np.zeros(npix), "status": np.zeros(npix, dtype=np.int32),
            "pa": np.zeros(npix, dtype=np.int32), "pc": np.zeros(npix, dtype=np.int32),
            "nlines": np.zeros(npix, dtype=np.int64), "pflux": np.zeros(npix), "seeds": np.ascontiguousarray(seeds),
            "integral": np.zeros(npix), "nsteps": np.zeros(npix, dtype=np.int32)}
    bz_face = b[2, 0].reshape(-1)
    up, down = np.ascontiguousarray(seeds[bz_face > 0.0]), np.ascontiguousarray(seeds[bz_face < 0.0])
    host.update({"up": up, "down": down})
    dev = upload(host)
    bz0 = ctypes.c_void_p(dev["B"].value + 16 * m ** 3)
    assert L.ndsm_hip_partition_device(*head, bz0, 0.0, 0, counts.ctypes.data, dev["label"], *[None] * 6) == 0
    K = int(counts[1])
    max_steps = V.default_max_steps(0.5)

    def connect(steps):
        def call():
            rc = L.ndsm_hip_vecpot_connect_device(V.h, dev["B"], dev["label"], K, 0.5, steps, npix, counts.ctypes.data,
                                                  *[dev[k] for k in ("dest", "ends", "length", "status", "pa", "pc",
                                                                     "nlines", "pflux")])
            assert rc == 0, _lib.last_error(L)
        return call

    def trace():
        rc = L.ndsm_hip_vecpot_trace_device(V.h, dev["B"], None, npix, dev["seeds"], 0.5, max_steps, 1, dev["ends"],
                                            dev["length"], dev["integral"], dev["status"], dev["nsteps"])
        assert rc == 0, _lib.last_error(L)

    def trace_signed():
        for name, count, direction in (("up", len(up), 1), ("down", len(down), -1)):
            rc = L.ndsm_hip_vecpot_trace_device(V.h, dev["B"], None, count, dev[name], 0.5, max_steps, direction,
                                                dev["ends"], dev["length"], dev["integral"], dev["status"], dev["nsteps"])
            assert rc == 0, _lib.last_error(L)

    row = {"side": m, "feet": npix, "K": K}
    c = put(row, "connect", measure(connect(max_steps)))
    row["lines"], row["pairs"] = int(counts[0]), int(counts[1])
    s = put(row, "connect_keyed", measure(connect(1)))
    t = put(row, "trace", measure(trace))
    ts = put(row, "trace_signed", measure(trace_signed))
    row["connect_over_trace"] = round(c / t, 3)
    row["connect_over_trace_signed"] = round(c / ts, 3)
    row["keyed_over_connect"] = round(s / c, 3)
    for p in dev.values():
        L.ndsm_hip_device_free(p)
    V.close()
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    repeats, side = 5, 128
    for flag in ("--repeats", "--side"):
        if flag in args:
            i = args.index(flag)
            if flag == "--repeats":
                repeats = int(args[i + 1])
            else:
                side = int(args[i + 1])
            del args[i:i + 2]
    main([int(a) for a in args] or [512, 1024], repeats=repeats, side=side)
