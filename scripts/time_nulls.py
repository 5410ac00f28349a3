"""Null-point detection on device-resident arrays, timed with device events, against the curl kernel on the same three
arrays: usage time_nulls.py [--repeats R] [n ...]   (default 128 256 512, --repeats 5)

Per size n^3, on one VecPot handle, the protocol of time_trace.py: B and the record arrays stay in device memory; each
variant is warmed up once and then timed R times between two events on the library stream; the calls are repeated
inside one timed window until it is at least 0.2 s long.  Reported per variant: median [min - max] of one call.
Variants, all ndsm_hip_vecpot_nulls_device with max_nulls = 4096:
  screen      a uniform field: no cell is a candidate, so the call is the screen alone (the two kernels, the scan of
              the workgroup counts and the count coming to the host); its rate against the 24 n^3 bytes of B
  abc         the ABC field (tests/test_gpu_field.py): few candidates, a handful of nulls - the whole call
  abc_noise   the ABC field plus white noise of an amplitude tuned (with the library's own count) so that about 1 % of
              the cells are candidates
  zero        an all-zero field: every cell is a candidate and fails at its first iteration (the list-building cost)
The yardstick, timed in the same run: curl_k on the same three arrays (it reads the same 24 n^3 bytes and writes 24 n^3
more), reached through ndsm_hip_vecpot_squash_device with G = B, integrand 1 and ONE seed outside the box - the curl
of the twist map plus a one-lane kernel that ends at once.  Neither figure is a bare kernel time: "screen" holds three
launches and the blocking 8-byte read of the count, the yardstick holds the curl, the one-lane kernel and the entry's
synchronisation."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import ndsm_amd  # noqa: E402
from ndsm_amd import _lib  # noqa: E402
from test_gpu_field import abc_field  # noqa: E402

WINDOW_S = 0.2
CAP = 4096


def noisy(b, rng, candidates_of, target=0.01):
    """b plus white noise of the amplitude at which about `target` of the cells are candidates: bisected with the
    library's own count (candidates_of(field); max_nulls = 0, the screen alone), until within a factor 1.3.  The
    candidates of such a field crowd where all three components are weak, so no sample of the box predicts them."""
    noise = rng.standard_normal(b.shape)
    cells = float(np.prod([k - 1 for k in b.shape[1:]]))
    lo, hi = 0.0, 4.0
    for _ in range(12):
        amp = 0.5 * (lo + hi)
        f = b + amp * noise
        frac = candidates_of(f) / cells
        if target / 1.3 <= frac <= target * 1.3:
            break
        if frac < target:
            lo = amp
        else:
            hi = amp
    return f, amp


def main(sizes, repeats=5):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    rows = []
    for n in sizes:
        mesh, b = abc_field([n, n, n])
        b = np.ascontiguousarray(b)
        V = ndsm_amd.VecPot(*mesh)
        rec = [np.zeros(CAP, dtype=np.int64), np.zeros((CAP, 3)), np.zeros((CAP, 9)), np.zeros(CAP), np.zeros(CAP),
               np.zeros(CAP, dtype=np.int32), np.zeros(CAP, dtype=np.int32)]
        host = {"B": b, "seed": np.array([[mesh[0][0] - 1.0, mesh[1][0], mesh[2][0]]]), "q": np.zeros(1),
                "ends": np.zeros((2, 3)), "length": np.zeros(2), "integral": np.zeros(2),
                "status": np.zeros(2, dtype=np.int32), "nsteps": np.zeros(2, dtype=np.int32)}
        host.update({"rec%d" % i: a for i, a in enumerate(rec)})
        dev = {}
        for k, a in host.items():
            dev[k] = ctypes.c_void_p()
            assert L.ndsm_hip_device_alloc(a.nbytes, ctypes.byref(dev[k])) == 0, _lib.last_error(L)
        assert L.ndsm_hip_memcpy_h2d(dev["seed"], host["seed"].ctypes.data, host["seed"].nbytes) == 0
        counts = np.zeros(2, dtype=np.int64)

        def nulls():
            rc = L.ndsm_hip_vecpot_nulls_device(V.h, dev["B"], CAP, counts.ctypes.data,
                                                *[dev["rec%d" % i] for i in range(7)])
            assert rc == 0, _lib.last_error(L)

        def curl():
            rc = L.ndsm_hip_vecpot_squash_device(V.h, dev["B"], dev["B"], 1, 1, dev["seed"], 0.5, 1, dev["q"],
                                                 dev["ends"], dev["length"], dev["integral"], dev["status"],
                                                 dev["nsteps"])
            assert rc == 0, _lib.last_error(L)

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

        def candidates_of(f):
            assert L.ndsm_hip_memcpy_h2d(dev["B"], f.ctypes.data, f.nbytes) == 0
            rc = L.ndsm_hip_vecpot_nulls_device(V.h, dev["B"], 0, counts.ctypes.data, *[None] * 7)
            assert rc == 0, _lib.last_error(L)
            return int(counts[0])

        bn, amp = noisy(b, np.random.default_rng(11), candidates_of)
        fields = {"screen": np.full(b.shape, 0.7), "abc": b, "abc_noise": bn, "zero": np.zeros(b.shape)}
        row = {"n": n, "field_MB": round(b.nbytes / 1e6, 1), "noise_amplitude": round(amp, 4)}
        for name, f in fields.items():
            f = np.ascontiguousarray(f)
            assert L.ndsm_hip_memcpy_h2d(dev["B"], f.ctypes.data, f.nbytes) == 0
            med, tmin, tmax, calls = measure(nulls)
            row.update({name + "_ms": round(med * 1e3, 4), name + "_min_ms": round(tmin * 1e3, 4),
                        name + "_max_ms": round(tmax * 1e3, 4), name + "_calls_per_window": calls,
                        name + "_candidates": int(counts[0]), name + "_nulls": int(counts[1])})
            if name == "screen":
                row["screen_TB_per_s"] = round(b.nbytes / med / 1e12, 3)
            if name == "abc":
                med, tmin, tmax, calls = measure(curl)
                row.update({"curl_ms": round(med * 1e3, 4), "curl_min_ms": round(tmin * 1e3, 4),
                            "curl_max_ms": round(tmax * 1e3, 4), "curl_calls_per_window": calls})
        row["candidate_fraction_abc_noise"] = round(row["abc_noise_candidates"] / float((n - 1) ** 3), 5)
        row["screen_over_curl"] = round(row["screen_ms"] / row["curl_ms"], 3)
        for p in dev.values():
            L.ndsm_hip_device_free(p)
        V.close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


if __name__ == "__main__":
    args = sys.argv[1:]
    repeats = 5
    if "--repeats" in args:
        i = args.index("--repeats")
        repeats = int(args[i + 1])
        del args[i:i + 2]
    main([int(a) for a in args] or [128, 256, 512], repeats=repeats)
