"""The separator entry on device-resident arrays, timed with device events, against the paths entry on the seeds of its
first round: usage time_separators.py [--repeats R] [--nring K] [--max-nulls M] [n]
(default 128, --nring 8, --max-nulls 32, --repeats 5)

The protocol of time_trace.py.  Two cases per size n^3, each on one VecPot handle, B and every array of the call in
device memory:
  crossing   the two-null crossing field of tests/separator_model.py, its nulls and their types from the Python layer,
             the default brackets of a K-seed ring for both ordered pairs (2 K brackets), radius 1, capture 0.5
  noise      the ABC field plus the white noise of time_skeleton.py, the first M nulls of ndsm_hip_vecpot_nulls_device,
             typed by ndsm_hip_vecpot_skeleton_device, the default brackets of all opposite-sign pairs, radius 0.5,
             capture 0.5
step 0.5, the default max_steps, every 1, tol 1e-12.  Timed in the same run, each warmed up once and then R times
between two events on the library stream, the calls repeated inside one timed window until it is at least 0.2 s long:
  sep_count, sep_fill   the separator entry with rounds = 10: the counting call (max_points = 0: the check of the
                        pairs, the refinement, the counting pass of the lines) and the filling call (max_points =
                        total, points and bpt: all of the counting call again, then the filling pass)
  sep1_count            the counting call with rounds = 1: one round of the refinement
  paths_count           ndsm_hip_vecpot_paths_device without G, max_points = 0, on the 64 seeds of the first round of
                        every bracket that is traced (formed on the host by tests/separator_model.lane_seeds, the
                        device's bits), one call per direction, the times added: the same lines as sep1's round without
                        the capture by m'
Reported per variant: the median time of one call [min, max]; the ratio sep1 / paths (one round against the plain lines
of its seeds); brackets, states, rounds."""
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
from golden_inputs import uniform_mesh  # noqa: E402
from separator_model import basis_numpy, crossing_field, lane_seeds  # noqa: E402
from skeleton_model import default_ring  # noqa: E402
from test_gpu_field import abc_field  # noqa: E402
from time_nulls import noisy  # noqa: E402

WINDOW_S = 0.2
STEP, TOL = 0.5, 1e-12


def main(n=128, nring=8, repeats=5, max_nulls=32):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    rows = []
    for case in ("crossing", "noise"):
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

        if case == "crossing":
            mesh = uniform_mesh([n, n, n])
            b = np.ascontiguousarray(crossing_field(mesh)[0])
            radius = 1.0
        else:
            mesh, b = abc_field([n, n, n])
            radius = 0.5
        V = ndsm_amd.VecPot(*mesh)
        max_steps = V.default_max_steps(STEP)
        if case == "noise":
            dB0 = alloc(b.nbytes)
            counts = np.zeros(2, dtype=np.int64)

            def candidates_of(f):
                assert L.ndsm_hip_memcpy_h2d(dB0, f.ctypes.data, f.nbytes) == 0
                assert L.ndsm_hip_vecpot_nulls_device(V.h, dB0, 0, counts.ctypes.data, *[None] * 7) == 0
                return int(counts[0])
            b, _amp = noisy(np.ascontiguousarray(b), np.random.default_rng(11), candidates_of)
            b = np.ascontiguousarray(b)
        nul = V.nulls(b, device=True)
        keep = slice(0, max_nulls)
        sk = V.skeleton(b, nulls=(nul.position[keep], nul.jacobian[keep]), radius=radius, nring=0, capture=0.5, step=STEP,
                        max_steps=1, max_points=0, values=False, device=True)
        pos, kind, normal = sk.position, sk.kind, sk.normal
        pair, arc = _lib._separator_brackets(kind, default_ring(nring))
        nn, nbr = len(pos), len(pair)
        dB = up(b.reshape(-1))
        din = [up(pos), up(kind), up(normal), up(pair), up(arc)]
        outs = [alloc(w * nbr) for w in (4, 4, 32, 8, 4, 16, 24, 8, 4, 4)] + [alloc(8 * (nbr + 1))]
        total = np.zeros(1, dtype=np.int64)

        def sep(rounds, cap, pts):
            rc = L.ndsm_hip_vecpot_separators_device(V.h, dB, nn, din[0], din[1], din[2], nbr, din[3], din[4], radius, 0.5,
                                                     STEP, max_steps, rounds, TOL, 1, cap, *outs, total.ctypes.data, *pts)
            assert rc == 0, _lib.last_error(L)

        # the seeds of the first round for the paths entry, one call per direction
        valid = (kind[pair[:, 0]] > 0) != (kind[pair[:, 1]] > 0)
        e1, e2 = basis_numpy(normal[pair[:, 0]])
        rho = radius * min(q[1] - q[0] for q in mesh)
        _c, _s, _ok, seeds = lane_seeds(pos[pair[:, 0]], e1, e2, arc[:, :2], arc[:, 2:], rho)
        sgn = np.where(kind[pair[:, 0]] > 0, 1, -1)
        groups = []
        for sg in (1, -1):
            S = np.ascontiguousarray(seeds[valid & (sgn == sg)].reshape(-1, 3))
            k = len(S)
            groups.append((sg, k, up(S), [alloc(24 * k), alloc(8 * k), alloc(8 * k), alloc(4 * k), alloc(4 * k),
                                          alloc(8 * (k + 1))]))
        ptotal = np.zeros(1, dtype=np.int64)

        def paths():
            for sg, k, dS, out in groups:
                if k:
                    rc = L.ndsm_hip_vecpot_paths_device(V.h, dB, None, k, dS, STEP, max_steps, sg, 1, 0, *out,
                                                        ptotal.ctypes.data, *[None] * 4)
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

        sep(10, 0, [None, None])
        npts = int(total[0])
        pts = [alloc(24 * npts), alloc(24 * npts)]
        row = {"case": case, "n": n, "nulls": nn, "nring": nring, "brackets": nbr, "max_steps": max_steps,
               "points": npts, "path_lines": sum(g[1] for g in groups)}
        for tag, fn in (("sep_count", lambda: sep(10, 0, [None, None])), ("sep_fill", lambda: sep(10, npts, pts)),
                        ("sep1_count", lambda: sep(1, 0, [None, None])), ("paths_count", paths)):
            med, lo, hi = measure(fn)
            row.update({tag + "_ms": round(med * 1e3, 3), tag + "_min_ms": round(lo * 1e3, 3),
                        tag + "_max_ms": round(hi * 1e3, 3)})
        sep(10, 0, [None, None])
        state, rounds = np.zeros(nbr, dtype=np.int32), np.zeros(nbr, dtype=np.int32)
        assert L.ndsm_hip_memcpy_d2h(state.ctypes.data, outs[0], state.nbytes) == 0
        assert L.ndsm_hip_memcpy_d2h(rounds.ctypes.data, outs[1], rounds.nbytes) == 0
        row["state_counts"] = np.bincount(state, minlength=6).tolist()
        row["rounds_counts"] = np.bincount(rounds, minlength=11).tolist()
        row["sep1_over_paths"] = round(row["sep1_count_ms"] / row["paths_count_ms"], 3) if row["paths_count_ms"] else None
        for p in live:
            L.ndsm_hip_device_free(p)
        V.close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--repeats": "5", "--nring": "8", "--max-nulls": "32"}
    for o in list(opts):
        if o in args:
            i = args.index(o)
            opts[o] = args[i + 1]
            del args[i:i + 2]
    main(int(args[0]) if args else 128, nring=int(opts["--nring"]), repeats=int(opts["--repeats"]),
         max_nulls=int(opts["--max-nulls"]))
