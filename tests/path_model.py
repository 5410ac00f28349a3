"""The numpy restatement of the path semantics in include/ndsm_hip.h (ndsm_hip_vecpot_paths), which the device matches
bit for bit: path_numpy is line_model.trace_numpy's loop on line_model.Lines - the same stage, step, exit and snap, so
the same states - which records the state of a line before every `every`-th step that moves it, and the final state
with one more interpolation at it.  paths_numpy puts the directions of a call together in lane order."""
import collections

import numpy as np

from line_model import NULL, OUTSIDE, UNFINISHED, Lines

Paths = collections.namedtuple("Paths", ["ends", "length", "integral", "status", "nsteps", "offsets", "points", "bpt",
                                         "gpt", "ipt"])


def npts_of(nsteps, every):
    """the points of a line of n steps: 1 if n = 0, else (n - 1) / every + 2"""
    n = np.asarray(nsteps, dtype=np.int64)
    return np.where(n == 0, 1, (n - 1) // every + 2)


def path_numpy(mesh, b, g, seeds, step, max_steps, sgn, every):
    """a Paths tuple of the lines of one direction (sgn +1 or -1): trace_numpy's five outputs, offsets (ns + 1), and the
    concatenated points (total,3), bpt, gpt (total,3), ipt (total); gpt and ipt are zeros without g"""
    m = Lines(mesh, b, g, step)
    ds = m.ds

    def stage(P):
        c = m.cell(P)
        bx, by, bz = m.values(m.bf, c)
        mag = np.sqrt((bx * bx + by * by) + bz * bz)
        ok = mag > 0.0
        ms = np.where(ok, mag, 1.0)
        ex, ey, ez = bx / ms, by / ms, bz / ms
        k = np.stack([sgn * ex, sgn * ey, sgn * ez], axis=1)
        bv = np.stack([bx, by, bz], axis=1)
        if m.gf is None:
            q = np.zeros(len(P))
            gv = np.zeros((len(P), 3))
        else:
            gx, gy, gz = m.values(m.gf, c)
            q = (gx * ex + gy * ey) + gz * ez
            gv = np.stack([gx, gy, gz], axis=1)
        return ok, k, q, bv, gv

    def rk4(r, k1, q1, s):
        hs, s6 = (0.5 * s)[:, None], s / 6.0
        ok2, k2, q2, _b, _g = stage(r + hs * k1)
        ok3, k3, q3, _b, _g = stage(np.where(ok2[:, None], r + hs * k2, r))
        ok = ok2 & ok3
        ok4, k4, q4, _b, _g = stage(np.where(ok[:, None], r + s[:, None] * k3, r))
        ok = ok & ok4
        rn = r + s6[:, None] * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)
        dI = s6 * (((q1 + 2.0 * q2) + 2.0 * q3) + q4)
        return ok, rn, dI

    ns = len(seeds)
    r = np.array(seeds, dtype=np.float64).reshape(ns, 3)
    length, integral = np.zeros(ns), np.zeros(ns)
    status = np.full(ns, UNFINISHED, dtype=np.int32)
    nsteps = np.zeros(ns, dtype=np.int32)
    inside = m.inside(r)
    status[~inside] = OUTSIDE
    act = np.nonzero(inside)[0]
    rec = [[] for _ in range(ns)]                # per line: (r, b, g, I) of each stored point
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for it in range(max_steps):
            if len(act) == 0:
                break
            ra = r[act]
            ok1, k1, q1, bv, gv = stage(ra)
            okr, rn, dI = rk4(ra, np.where(ok1[:, None], k1, 0.0), q1, np.full(len(act), ds))
            ok = ok1 & okr
            rn = np.where(ok[:, None], rn, ra)
            t, face = m.first_face(ra, rn)
            leave = ok & (face != 0)
            s = np.where(leave, t * ds, ds)
            ok2, rn2, dI2 = rk4(ra, np.where(ok1[:, None], k1, 0.0), q1, s)
            null = ~ok | (leave & ~ok2)
            leave = leave & ok2
            snapped = m.snap(rn2, face)
            go = ok & ~leave & ~null
            ia = act
            if it % every == 0:
                # step `it` moves these lines: their state after `it` steps is a point
                for a in np.nonzero(go | leave)[0]:
                    rec[ia[a]].append((ra[a].copy(), bv[a].copy(), gv[a].copy(), integral[ia[a]]))
            r[ia[go]] = rn[go]
            length[ia[go]] = length[ia[go]] + ds
            integral[ia[go]] = integral[ia[go]] + dI[go]
            nsteps[ia[go]] = it + 1
            r[ia[leave]] = snapped[leave]
            length[ia[leave]] = length[ia[leave]] + s[leave]
            integral[ia[leave]] = integral[ia[leave]] + dI2[leave]
            nsteps[ia[leave]] = it + 1
            status[ia[leave]] = face[leave]
            status[ia[null]] = NULL
            act = ia[go]
        # the final state of every line: B and G interpolated at it, except at a point that is not in the box
        bl, gl = np.zeros((ns, 3)), np.zeros((ns, 3))
        ins = np.nonzero(inside)[0]
        if len(ins):
            _ok, _k, _q, bv, gv = stage(r[ins])
            bl[ins], gl[ins] = bv, gv
    for l in range(ns):
        rec[l].append((r[l].copy(), bl[l], gl[l], integral[l]))
    counts = np.array([len(x) for x in rec], dtype=np.int64)
    assert np.array_equal(counts, npts_of(nsteps, every)), (counts, nsteps, every)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    flat = [x for line in rec for x in line]
    points = np.array([x[0] for x in flat]).reshape(-1, 3)
    bpt = np.array([x[1] for x in flat]).reshape(-1, 3)
    gpt = np.array([x[2] for x in flat]).reshape(-1, 3)
    ipt = np.array([x[3] for x in flat], dtype=np.float64)
    return Paths(r, length, integral, status, nsteps, offsets, points, bpt, gpt, ipt)


def paths_numpy(mesh, b, g, seeds, step, max_steps, direction, every):
    """the Paths of one call: direction +1, -1, or 0 (the forward block, then the backward block)"""
    parts = [path_numpy(mesh, b, g, seeds, step, max_steps, sgn, every)
             for sgn in ((1.0, -1.0) if direction == 0 else (float(direction),))]
    return join(parts)


def join(parts):
    """the Paths of lane blocks put behind each other"""
    offs, at = [np.zeros(1, dtype=np.int64)], 0
    for p in parts:
        offs.append(p.offsets[1:] + at)
        at += int(p.offsets[-1])
    cat = [np.concatenate([p[k] for p in parts]) for k in (0, 1, 2, 3, 4)]
    return Paths(*cat, np.concatenate(offs), *[np.concatenate([p[k] for p in parts]) for k in (6, 7, 8, 9)])


def take(p, idx):
    """the Paths of the lines idx of p (one block), in that order: every line depends on its own seed only"""
    rows = [np.arange(p.offsets[i], p.offsets[i + 1]) for i in idx]
    counts = np.array([len(x) for x in rows], dtype=np.int64)
    rows = np.concatenate(rows) if len(rows) else np.zeros(0, dtype=np.int64)
    return Paths(*[p[k][idx] for k in range(5)], np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                 *[p[k][rows] for k in (6, 7, 8, 9)])
