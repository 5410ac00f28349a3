"""The flow fit, the plane's vector potential and the fluxes on device-resident arrays, timed with device events:
usage time_flow.py [--repeats R] [--ap-side M] [n ...]   (default 512 1024, --repeats 5, --ap-side 256)

The protocol of time_dips.py: the arrays stay in device memory; each variant is warmed up once and
then timed R times between two events on the library stream; the calls are repeated inside one timed window until it is
at least 0.2 s long.  Reported per variant: median [min - max] of one call.
  fit_r5, fit_r10   ndsm_hip_flow_fit_device on n x n white noise with r = 5 and r = 10: the two prep launches, the fit
                    launch and the stream synchronisation
  flux              ndsm_hip_flow_flux_device on the same arrays (its blocking read of the sums included)
  ap_plane          ndsm_hip_green_ap_plane_device on an M x M magnetogram: M^2 targets times M^2 pixels
  green_points      the yardstick of ap_plane, in the same run: ndsm_hip_green_points_device with the same M^2 pixels and
                    M^2 targets, one mesh row above the plane (a pair there costs a sqrt and a division more)
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


def main(sizes, repeats=5, ap_side=256):
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

    rng = np.random.default_rng(7)
    for n in sizes:
        xs = ys = 0.1 * np.arange(n)
        ns = np.array([n, n], dtype=np.intc)
        head = (ns.ctypes.data_as(_lib._ip), _lib._d(xs), _lib._d(ys))
        host = {"B0": rng.uniform(-1.0, 1.0, (3, n, n)), "B1": rng.uniform(-1.0, 1.0, (3, n, n)), "V": np.zeros((3, n, n)),
                "coef": np.zeros((9, n, n)), "status": np.zeros((n, n), dtype=np.int32),
                "Ap": rng.uniform(-1.0, 1.0, (2, n, n)), "dens": np.zeros((4, n, n))}
        dev = upload(host)
        out = np.zeros(8)

        def fit(r):
            def call():
                rc = L.ndsm_hip_flow_fit_device(*head, dev["B0"], dev["B1"], 0.5, r, 1e-10, dev["V"], dev["coef"],
                                                dev["status"])
                assert rc == 0, _lib.last_error(L)
            return call

        def flux():
            rc = L.ndsm_hip_flow_flux_device(*head, dev["B0"], dev["V"], dev["Ap"], dev["dens"], _lib._d(out))
            assert rc == 0, _lib.last_error(L)

        row = {"n": n, "pixels": n * n}
        for r in (5, 10):
            med = put(row, "fit_r%d" % r, measure(fit(r)))
            row["fit_r%d_Mpix_per_s" % r] = round(n * n / med / 1e6, 1)
            row["fit_r%d_Gpairs_per_s" % r] = round(n * n * (2 * r + 1) ** 2 / med / 1e9, 2)
        st = np.zeros((n, n), dtype=np.int32)
        assert L.ndsm_hip_memcpy_d2h(st.ctypes.data, dev["status"], st.nbytes) == 0
        row["solved"] = int((st == 0).sum())
        put(row, "flux", measure(flux))
        for p in dev.values():
            L.ndsm_hip_device_free(p)
        print(json.dumps(row), flush=True)

    m = ap_side
    xs = ys = 0.1 * np.arange(m)
    ns = np.array([m, m], dtype=np.intc)
    head = (ns.ctypes.data_as(_lib._ip), _lib._d(xs), _lib._d(ys))
    X, Y = np.meshgrid(xs, ys)
    pts = np.stack([X.ravel(), Y.ravel(), np.full(m * m, 0.1)], axis=1)
    dev = upload({"bz": rng.uniform(-1.0, 1.0, (m, m)), "Ap": np.zeros((2, m, m)), "pts": np.ascontiguousarray(pts),
                  "B": np.zeros((m * m, 3))})

    def ap_plane():
        rc = L.ndsm_hip_green_ap_plane_device(*head, dev["bz"], dev["Ap"])
        assert rc == 0, _lib.last_error(L)

    def green_points():
        rc = L.ndsm_hip_green_points_device(*head, 0.0, dev["bz"], m * m, dev["pts"], dev["B"])
        assert rc == 0, _lib.last_error(L)

    row = {"ap_side": m, "pairs": m ** 4}
    a = put(row, "ap_plane", measure(ap_plane))
    g = put(row, "green_points", measure(green_points))
    row["ap_Gpairs_per_s"] = round(m ** 4 / a / 1e9, 2)
    row["green_Gpairs_per_s"] = round(m ** 4 / g / 1e9, 2)
    row["ap_over_green"] = round(a / g, 3)
    for p in dev.values():
        L.ndsm_hip_device_free(p)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    repeats, ap_side = 5, 256
    for flag in ("--repeats", "--ap-side"):
        if flag in args:
            i = args.index(flag)
            if flag == "--repeats":
                repeats = int(args[i + 1])
            else:
                ap_side = int(args[i + 1])
            del args[i:i + 2]
    main([int(a) for a in args] or [512, 1024], repeats=repeats, ap_side=ap_side)
