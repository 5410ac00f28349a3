"""Dips and bald patches on device-resident arrays, timed with device events, against the curl kernel and the nulls
screen on the same three arrays: usage time_dips.py [--repeats R] [n ...]   (default 128 256 512, --repeats 5)

Per size n^3, on one VecPot handle, the protocol of time_nulls.py: B and the record arrays stay in device memory; each
variant is warmed up once and then timed R times between two events on the library stream; the calls are repeated
inside one timed window until it is at least 0.2 s long.  Reported per variant: median [min - max] of one call.
Variants, all ndsm_hip_vecpot_dips_device with max_dips = 2^20, each as the full call and with plane_only = 1:
  uniform     a uniform field: no crossing, so the call is the vote pass alone (one kernel, the three scans of the
              workgroup counts and the totals coming to the host); its rate against the 8 n^3 bytes of B_z
  rope        the flux rope about an axis along y of tests/dips_model.py: one crossing per (j, k), about half of them dips
  abc_noise   the ABC field (tests/test_gpu_field.py) plus 1 % white noise
The yardsticks, timed in the same run on the same arrays: curl_k (24 n^3 bytes read, 24 n^3 written), reached through
ndsm_hip_vecpot_squash_device as in time_nulls.py, and the nulls screen on the uniform field
(ndsm_hip_vecpot_nulls_device, no candidate).  None of the figures is a bare kernel time: each holds its entry's
launches and its blocking read of the counts."""
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
from dips_model import inside, rope  # noqa: E402
from test_gpu_field import abc_field  # noqa: E402

WINDOW_S = 0.2
CAP = 2 ** 20
NULLS_CAP = 4096


def main(sizes, repeats=5):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    rows = []
    for n in sizes:
        mesh, b = abc_field([n, n, n])
        b = np.ascontiguousarray(b)
        V = ndsm_amd.VecPot(*mesh)
        rec = [np.zeros(CAP, dtype=np.int64), np.zeros((CAP, 3)), np.zeros((CAP, 3)), np.zeros((CAP, 3)), np.zeros(CAP),
               np.zeros(CAP, dtype=np.int32)]
        nrec = [np.zeros(NULLS_CAP, dtype=np.int64), np.zeros((NULLS_CAP, 3)), np.zeros((NULLS_CAP, 9)),
                np.zeros(NULLS_CAP), np.zeros(NULLS_CAP), np.zeros(NULLS_CAP, dtype=np.int32),
                np.zeros(NULLS_CAP, dtype=np.int32)]
        host = {"B": b, "seed": np.array([[mesh[0][0] - 1.0, mesh[1][0], mesh[2][0]]]), "q": np.zeros(1),
                "ends": np.zeros((2, 3)), "length": np.zeros(2), "integral": np.zeros(2),
                "status": np.zeros(2, dtype=np.int32), "nsteps": np.zeros(2, dtype=np.int32)}
        host.update({"rec%d" % i: a for i, a in enumerate(rec)})
        host.update({"nrec%d" % i: a for i, a in enumerate(nrec)})
        dev = {}
        for k, a in host.items():
            dev[k] = ctypes.c_void_p()
            assert L.ndsm_hip_device_alloc(a.nbytes, ctypes.byref(dev[k])) == 0, _lib.last_error(L)
        assert L.ndsm_hip_memcpy_h2d(dev["seed"], host["seed"].ctypes.data, host["seed"].nbytes) == 0
        counts = np.zeros(3, dtype=np.int64)
        ncounts = np.zeros(2, dtype=np.int64)

        def dips(plane_only):
            def call():
                rc = L.ndsm_hip_vecpot_dips_device(V.h, dev["B"], plane_only, CAP, counts.ctypes.data,
                                                   *[dev["rec%d" % i] for i in range(6)])
                assert rc == 0, _lib.last_error(L)
            return call

        def nulls():
            rc = L.ndsm_hip_vecpot_nulls_device(V.h, dev["B"], NULLS_CAP, ncounts.ctypes.data,
                                                *[dev["nrec%d" % i] for i in range(7)])
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

        def put(row, name, stats):
            med, tmin, tmax, calls = stats
            row.update({name + "_ms": round(med * 1e3, 4), name + "_min_ms": round(tmin * 1e3, 4),
                        name + "_max_ms": round(tmax * 1e3, 4), name + "_calls_per_window": calls})
            return med

        ext = mesh[2][-1] - mesh[2][0]
        noise = 0.01 * np.random.default_rng(11).standard_normal(b.shape)
        fields = {"uniform": np.full(b.shape, 0.7),
                  "rope": rope(mesh, 1.3, 0.225 * ext, 0.7, inside(mesh, 0, n // 2), inside(mesh, 2, n // 2, 0.41)),
                  "abc_noise": b + noise}
        del noise
        row = {"n": n, "field_MB": round(b.nbytes / 1e6, 1)}
        for name, f in fields.items():
            f = np.ascontiguousarray(f)
            assert L.ndsm_hip_memcpy_h2d(dev["B"], f.ctypes.data, f.nbytes) == 0
            for plane_only, tag in ((0, name), (1, name + "_plane")):
                med = put(row, tag, measure(dips(plane_only)))
                row.update({tag + "_crossings": int(counts[0]), tag + "_dips": int(counts[1]),
                            tag + "_bald": int(counts[2])})
                if tag == "uniform":
                    row["uniform_TB_per_s_of_bz"] = round(b.nbytes / 3 / med / 1e12, 3)
            if name == "uniform":
                put(row, "curl", measure(curl))
                put(row, "nulls_screen", measure(nulls))
                assert ncounts[0] == 0
        for tag in ("uniform", "rope", "abc_noise", "nulls_screen"):
            row[tag + "_over_curl"] = round(row[tag + "_ms"] / row["curl_ms"], 3)
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
