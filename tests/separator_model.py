"""What the separator tests share (test_separators_model.py on the CPU, test_gpu_separators.py on the GPU):
separators_numpy, the numpy restatement of the semantics of ndsm_hip_vecpot_separators in include/ndsm_hip.h on
line_model.Lines and skeleton_model's functions, in the header's operand order (the device matches it bit for bit) -
basis_numpy, the fan basis from the normal; trace_numpy, skeleton_model.lines_numpy's loop with one target null per
lane and the closest-approach test; the rounds -, the crossing field of DESIGN.md, the default brackets of a ring, and
the closed-form checks as functions of a runner

    run(mesh, b, pos, kind, normal, pair, arc, radius, capture, step, max_steps, rounds, tol, every) -> Sep

so that the same checks run on the restatement and on the device entries."""
import collections

import numpy as np

from line_model import NULL, OUTSIDE, UNFINISHED, Lines, box, grids
from null_model import nulls_numpy
from path_model import npts_of
from skeleton_model import CAPTURED, NONE, type_numpy

SEP_NONE, FOUND, FAR, NO_CROSSING, GAP, UNRESOLVED = range(6)
LANES = 64

Sep = collections.namedtuple("Sep", ["state", "nrounds", "coef", "width", "side", "dmin", "ends", "length", "status",
                                     "nsteps", "offsets", "points", "bpt"])
NAMES = Sep._fields
NPER = 10                   # the per-bracket arrays come first, then offsets and the two point arrays


# ---------------------------------------------------------------------------------------------------------------
# the numpy restatement of include/ndsm_hip.h
# ---------------------------------------------------------------------------------------------------------------
def basis_numpy(w):
    """the fan basis (e1, e2), each (n,3), of the normals w (n,3): item 6 of the skeleton's stage 1"""
    w = [w[:, 0], w[:, 1], w[:, 2]]
    with np.errstate(invalid="ignore", divide="ignore"):
        j = np.zeros(len(w[0]), dtype=np.int64)
        small, wj = np.abs(w[0]), w[0]
        for d in (1, 2):
            take = np.abs(w[d]) < small
            j = np.where(take, d, j)
            wj = np.where(take, w[d], wj)
            small = np.where(take, np.abs(w[d]), small)
        u = [np.where(j == d, 1.0, 0.0) - wj * w[d] for d in range(3)]
        un = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
        e1 = [u[d] / un for d in range(3)]
        e2 = [w[1] * e1[2] - w[2] * e1[1], w[2] * e1[0] - w[0] * e1[2], w[0] * e1[1] - w[1] * e1[0]]
    return np.stack(e1, axis=1), np.stack(e2, axis=1)


def trace_numpy(m, seeds, sgn, tpos, tw, cap2, max_steps, every=1, record=False):
    """skeleton_model.lines_numpy's loop on the Lines m with the capture test against the lane's own target tpos (nl,3)
    alone and the closest-approach test (normal of the target: tw): (ends, length, status, nsteps, best, g, rec) - best
    the smallest d2 of the line (inf: no point), g at its first point; rec (record): the (point, b) rows of each lane"""
    ds = m.ds

    def stage(P, sg):
        c = m.cell(P)
        bx, by, bz = m.values(m.bf, c)
        mag = np.sqrt((bx * bx + by * by) + bz * bz)
        ok = mag > 0.0
        ms = np.where(ok, mag, 1.0)
        ex, ey, ez = bx / ms, by / ms, bz / ms
        return ok, np.stack([sg * ex, sg * ey, sg * ez], axis=1), np.stack([bx, by, bz], axis=1)

    def rk4(r, sg, k1, s):
        hs, s6 = (0.5 * s)[:, None], s / 6.0
        ok2, k2, _b = stage(r + hs * k1, sg)
        ok3, k3, _b = stage(np.where(ok2[:, None], r + hs * k2, r), sg)
        ok = ok2 & ok3
        ok4, k4, _b = stage(np.where(ok[:, None], r + s[:, None] * k3, r), sg)
        ok = ok & ok4
        return ok, r + s6[:, None] * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)

    nl = len(seeds)
    r = np.array(seeds, dtype=np.float64).reshape(nl, 3)
    length = np.zeros(nl)
    status = np.full(nl, UNFINISHED, dtype=np.int32)
    nsteps = np.zeros(nl, dtype=np.int32)
    best = np.full(nl, np.inf)
    g = np.zeros(nl)
    none = sgn == 0.0
    inside = m.inside(r)
    status[~inside] = OUTSIDE
    status[none] = NONE
    runs = inside & ~none
    act = np.nonzero(runs)[0]
    rec = [[] for _ in range(nl)] if record else None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for it in range(max_steps):
            if len(act) == 0:
                break
            ra, sg = r[act], sgn[act]
            ok1, k1, bv = stage(ra, sg)
            k1 = np.where(ok1[:, None], k1, 0.0)
            okr, rn = rk4(ra, sg, k1, np.full(len(act), ds))
            ok = ok1 & okr
            rn = np.where(ok[:, None], rn, ra)
            t, face = m.first_face(ra, rn)
            leave = ok & (face != 0)
            s = np.where(leave, t * ds, ds)
            if leave.any():
                ok2, rn2 = rk4(ra, sg, k1, s)
            else:
                ok2, rn2 = ok, rn
            null = ~ok | (leave & ~ok2)
            leave = leave & ok2
            snapped = m.snap(rn2, face)
            go = ok & ~leave & ~null
            ia = act
            if record and it % every == 0:
                for a in np.nonzero(go | leave)[0]:
                    rec[ia[a]].append((ra[a].copy(), bv[a].copy()))
            r[ia[go]] = rn[go]
            length[ia[go]] = length[ia[go]] + ds
            nsteps[ia[go]] = it + 1
            r[ia[leave]] = snapped[leave]
            length[ia[leave]] = length[ia[leave]] + s[leave]
            nsteps[ia[leave]] = it + 1
            status[ia[leave]] = face[leave]
            status[ia[null]] = NULL
            act = ia[go]
            if len(act):
                d = r[act] - tpos[act]
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                closer = d2 < best[act]
                gg = (tw[act, 0] * d[:, 0] + tw[act, 1] * d[:, 1]) + tw[act, 2] * d[:, 2]
                g[act[closer]] = gg[closer]
                best[act[closer]] = d2[closer]
                got = d2 <= cap2
                status[act[got]] = CAPTURED
                act = act[~got]
        if record:
            bl = np.zeros((nl, 3))
            ins = np.nonzero(runs)[0]
            if len(ins):
                bl[ins] = stage(r[ins], sgn[ins])[2]
            for l in range(nl):
                rec[l].append((r[l].copy(), bl[l]))
    return r, length, status, nsteps, best, g, rec


def width_of(a, b):
    return np.sqrt((a[:, 0] - b[:, 0]) * (a[:, 0] - b[:, 0]) + (a[:, 1] - b[:, 1]) * (a[:, 1] - b[:, 1]))


def lane_seeds(p0, e1, e2, a, b, rho):
    """the lanes of one round of n brackets (p0, e1, e2 (n,3); a, b (n,2)): c, s, ok (n,64) and the seeds (n,64,3)"""
    t = np.arange(LANES) / 63.0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = (1.0 - t)[None, :] * a[:, 0, None] + t[None, :] * b[:, 0, None]
        s = (1.0 - t)[None, :] * a[:, 1, None] + t[None, :] * b[:, 1, None]
        nrm = np.sqrt(c * c + s * s)
        ok = nrm > 0.0
        c, s = c / nrm, s / nrm
        c[:, 0], s[:, 0], ok[:, 0] = a[:, 0], a[:, 1], True
        c[:, -1], s[:, -1], ok[:, -1] = b[:, 0], b[:, 1], True
        seeds = p0[:, None, :] + rho * (c[:, :, None] * e1[:, None, :] + s[:, :, None] * e2[:, None, :])
    return c, s, ok, seeds


def separators_numpy(mesh, b, pos, kind, normal, pair, arc, radius, capture, step, max_steps, rounds, tol, every,
                     history=None):
    """the Sep of one call of ndsm_hip_vecpot_separators; history (a list): per round (live brackets, classes (n,64),
    captured (n,64), nsteps (n,64)) is appended"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    kind = np.asarray(kind, dtype=np.int64).reshape(-1)
    normal = np.asarray(normal, dtype=np.float64).reshape(-1, 3)
    pair = np.asarray(pair, dtype=np.int64).reshape(-1, 2)
    arc = np.asarray(arc, dtype=np.float64).reshape(-1, 4)
    nbr = len(pair)
    m = Lines(mesh, b, None, step)
    hmin = min(m.h[0], m.h[1], m.h[2])
    rho = radius * hmin
    cr = capture * hmin
    cap2 = cr * cr
    m0, m1 = pair[:, 0], pair[:, 1]
    valid = (m0 != m1) & (((kind[m0] > 0) & (kind[m1] < 0)) | ((kind[m0] < 0) & (kind[m1] > 0)))
    sg = np.where(kind[m0] > 0, 1.0, -1.0)
    e1, e2 = basis_numpy(normal[m0])
    a, bb = arc[:, :2].copy(), arc[:, 2:].copy()
    state = np.zeros(nbr, dtype=np.int32)
    nrounds = np.zeros(nbr, dtype=np.int32)
    side = np.zeros(nbr, dtype=np.int32)
    dmin = np.zeros((nbr, 2))
    live = valid.copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for rnd in range(rounds):
            idx = np.nonzero(live)[0]
            if len(idx) == 0:
                break
            n = len(idx)
            c, s, ok, seeds = lane_seeds(pos[m0[idx]], e1[idx], e2[idx], a[idx], bb[idx], rho)
            sgn = np.where(ok, sg[idx][:, None], 0.0)
            tp = np.repeat(pos[m1[idx]], LANES, axis=0)
            tw = np.repeat(normal[m1[idx]], LANES, axis=0)
            _r, _len, st, nst, best, g, _rec = trace_numpy(m, seeds.reshape(-1, 3), sgn.reshape(-1), tp, tw, cap2,
                                                           max_steps)
            best, g, st = best.reshape(n, LANES), g.reshape(n, LANES), st.reshape(n, LANES)
            has_pt = best < np.inf
            cls = np.where(has_pt & (g >= 0.0), 1, np.where(has_pt & (g < 0.0), -1, 0))
            if history is not None:
                history.append((idx, cls, st == CAPTURED, nst.reshape(n, LANES)))
            c0 = cls[:, 0]
            differ = cls != c0[:, None]
            differ[:, 0] = False
            has = differ.any(axis=1)
            hi = np.where(has, np.argmax(differ, axis=1), LANES - 1)
            lo = np.where(has, hi - 1, 0)
            ar = np.arange(n)
            nrounds[idx] = rnd + 1
            side[idx] = c0
            dmin[idx, 0] = np.sqrt(best[ar, lo])
            dmin[idx, 1] = np.sqrt(best[ar, hi])
            gap = (c0 == 0) | (has & (cls[ar, hi] == 0))
            nocross = ~gap & ~has
            narrow = ~gap & has
            state[idx[gap]] = GAP
            state[idx[nocross]] = NO_CROSSING
            k = idx[narrow]
            a[k] = np.stack([c[ar, lo], s[ar, lo]], axis=1)[narrow]
            bb[k] = np.stack([c[ar, hi], s[ar, hi]], axis=1)[narrow]
            conv = width_of(a[k], bb[k]) <= tol
            both = ((st[ar, lo] == CAPTURED) & (st[ar, hi] == CAPTURED))[narrow]
            state[k] = np.where(conv, np.where(both, FOUND, FAR), UNRESOLVED)
            live[idx] = False
            live[k[~conv]] = True
        coef = np.concatenate([a, bb], axis=1)
        width = np.where(valid, width_of(a, bb), 0.0)
        # the line of the a side
        line = np.isin(state, (FOUND, FAR, UNRESOLVED))
        seeds = pos[m0] + rho * (a[:, 0, None] * e1 + a[:, 1, None] * e2)
        seeds = np.where(line[:, None], seeds, pos[m0])
        sgn = np.where(line, sg, 0.0)
    if nbr == 0:
        z = np.zeros
        return Sep(state, nrounds, coef, width, side, dmin, z((0, 3)), z(0), z(0, dtype=np.int32), z(0, dtype=np.int32),
                   z(1, dtype=np.int64), z((0, 3)), z((0, 3)))
    r, length, status, nsteps, _best, _g, rec = trace_numpy(m, seeds, sgn, pos[m1], normal[m1], cap2, max_steps, every,
                                                            record=True)
    counts = np.array([len(x) for x in rec], dtype=np.int64)
    assert np.array_equal(counts, npts_of(nsteps, every)), (counts, nsteps, every)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    flat = [x for ln in rec for x in ln]
    points = np.array([x[0] for x in flat]).reshape(-1, 3)
    bpt = np.array([x[1] for x in flat]).reshape(-1, 3)
    return Sep(state, nrounds, coef, width, side, dmin, r, length, status, nsteps, offsets, points, bpt)


def same_sep(got, want, what, upto=None):
    """bit for bit (NaN == NaN by its bits); upto: the point arrays of `got` hold the first upto slots only"""
    for k, name in enumerate(NAMES):
        w = want[k] if upto is None or k <= NPER else want[k][:upto]
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (what, name, got[k].dtype, got[k].shape, w.shape)
        assert got[k].tobytes() == w.tobytes(), (what, name, got[k], w)


def ring_of(nring, rot=0.0):
    """(c_j, s_j) of the angles rot + 2 pi (j + 1/2) / nring"""
    ang = rot + 2.0 * np.pi * (np.arange(nring) + 0.5) / max(nring, 1)
    return np.stack([np.cos(ang), np.sin(ang)], axis=1).reshape(nring, 2)


def ring_brackets(ring, pairs, narcs=None):
    """the default brackets: for every pair (m, m') the nring cyclically adjacent arcs (ring_j, ring_j+1) - the first
    narcs of them -: pair (nbr,2) int32 and arc (nbr,4), pair by pair, j ascending"""
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    arcs = np.concatenate([ring, np.roll(ring, -1, axis=0)], axis=1)[:narcs]
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    pair = np.repeat(pairs, len(arcs), axis=0)
    return np.ascontiguousarray(pair), np.ascontiguousarray(np.tile(arcs, (len(pairs), 1)))


def opposite_pairs(kind):
    """every ordered pair of typed nulls with opposite signs of kind, ascending"""
    kind = np.asarray(kind)
    return [(m, o) for m in range(len(kind)) for o in range(len(kind))
            if (kind[m] > 0 and kind[o] < 0) or (kind[m] < 0 and kind[o] > 0)]


# ---------------------------------------------------------------------------------------------------------------
# the crossing field
# ---------------------------------------------------------------------------------------------------------------
CROSS_FRACTIONS = np.array([0.47, 0.52, 0.45])


def crossing_field(mesh, a=0.2):
    """B = (a^2 - x'^2, c y', (2 x' - c) z') about the point at the fractions CROSS_FRACTIONS of the box, a in units
    of the x extent, c = 3 a: divergence-free, nulls at x' = -+a with kind (+1, -1) whose fans are the planes z' = 0 and
    y' = 0; they cross transversally in the separator, the segment of the x' axis between the nulls.  Only x'^2 is not
    reproduced by the interpolant; the planes y' = 0 and z' = 0 stay invariant.  Returns b, the centre and a in physical
    units."""
    lo, _h, hi, _n = box(mesh)
    rc = lo + (hi - lo) * CROSS_FRACTIONS
    aa = a * (hi[0] - lo[0])
    c = 3.0 * aa
    X, Y, Z = grids(mesh)
    x, y, z = X - rc[0], Y - rc[1], Z - rc[2]
    return np.stack([aa * aa - x * x, c * y, (2.0 * x - c) * z]), rc, aa


_CROSS = {}


def crossing_case(mesh):
    """the crossing field on the mesh and its two nulls in x order, typed as the skeleton types them (nulls_numpy's
    records, merged by the Python layer's rule): b, rc, pos (2,3), kind (2) int32, normal (2,3)"""
    from ndsm_amd import _lib
    key = tuple(np.asarray(q).tobytes() for q in mesh)
    if key not in _CROSS:
        b, rc, _aa = crossing_field(mesh)
        hmin = min(q[1] - q[0] for q in mesh)
        rec = nulls_numpy(mesh, b, 64)
        nul = _lib._nulls_tuple(list(rec[1:]), int(rec[0][0]), int(rec[0][1]), 1e-6 * hmin)
        assert len(nul.cell) == 2, len(nul.cell)
        order = np.argsort(nul.position[:, 0])
        pos, jac = nul.position[order].copy(), nul.jacobian[order].copy()
        _ok, _s, kind, _eig, _v, w, _e1, _e2 = type_numpy(jac)
        assert kind.tolist() == [1, -1], kind
        _CROSS[key] = (b, rc, pos, kind.astype(np.int32), w, jac)
    return _CROSS[key]


# ---------------------------------------------------------------------------------------------------------------
# the closed-form checks (each takes the runner)
# ---------------------------------------------------------------------------------------------------------------
CROSS_OPT = dict(radius=1.0, capture=0.5, step=0.5, max_steps=400, rounds=10, tol=1e-12, every=1)
OFF_AXIS = 4.7e-7      # in min(h): 100 x 4.7e-9, the restatement's own worst off-axis deviation of a FOUND line


def check_structure(sp, pos, pair, every):
    """what holds for every call: shapes, offsets from nsteps, the last point the end, the one-point lines"""
    nbr = len(pair)
    assert sp.state.shape == sp.nrounds.shape == sp.side.shape == (nbr,)
    assert sp.state.dtype == sp.nrounds.dtype == sp.side.dtype == np.int32
    assert sp.coef.shape == (nbr, 4) and sp.width.shape == (nbr,) and sp.dmin.shape == (nbr, 2)
    assert sp.ends.shape == (nbr, 3) and sp.length.shape == sp.status.shape == sp.nsteps.shape == (nbr,)
    assert sp.offsets.dtype == np.int64 and sp.offsets.shape == (nbr + 1,)
    assert np.array_equal(sp.offsets, np.concatenate([[0], np.cumsum(npts_of(sp.nsteps, every))]))
    total = int(sp.offsets[-1])
    assert sp.points.shape == sp.bpt.shape == (total, 3)
    if nbr == 0:
        return
    last = sp.offsets[1:] - 1
    assert sp.points[last].tobytes() == sp.ends.tobytes(), "the last point is not the end"
    noline = np.isin(sp.state, (SEP_NONE, NO_CROSSING, GAP))
    assert np.array_equal(sp.status == NONE, noline)
    assert np.all(sp.nsteps[noline] == 0) and not np.any(sp.length[noline]) and not np.any(sp.bpt[last[noline]])
    own = np.asarray(pos).reshape(-1, 3)[np.asarray(pair).reshape(-1, 2)[:, 0]]
    assert sp.ends[noline].tobytes() == own[noline].tobytes()
    assert np.all(sp.nrounds[sp.state == SEP_NONE] == 0) and np.all(sp.nrounds[sp.state != SEP_NONE] >= 1)
    assert np.all(np.isin(sp.side[np.isin(sp.state, (FOUND, FAR, UNRESOLVED, NO_CROSSING))], (-1, 1)))


def check_property(sp, run_skeleton, mesh, b, pos, jac, pair, radius, capture, step, max_steps, every, limit=None):
    """the header's property: the line of a FOUND, FAR or UNRESOLVED bracket is fan line 0 of the skeleton entry called
    with the nulls (m, m') and the ring (c_a, s_a) of coef, bit for bit.  run_skeleton: skeleton_model's runner; limit:
    only the first `limit` brackets of each of the three states.  Returns the number of lines compared."""
    rows = np.concatenate([np.nonzero(sp.state == st)[0][:limit] for st in (FOUND, FAR, UNRESOLVED)])
    n = 0
    for l in rows:
        mm = np.asarray(pair).reshape(-1, 2)[l]
        sk = run_skeleton(mesh, b, pos[mm], jac[mm], sp.coef[l, :2].reshape(1, 2), radius, capture, step, max_steps, every)
        a, e = int(sk.offsets[2]), int(sk.offsets[3])
        A, E = int(sp.offsets[l]), int(sp.offsets[l + 1])
        assert sk.points[a:e].tobytes() == sp.points[A:E].tobytes(), l
        assert sk.bpt[a:e].tobytes() == sp.bpt[A:E].tobytes(), l
        assert sk.ends[2].tobytes() == sp.ends[l].tobytes() and sk.length[2] == sp.length[l], l
        assert sk.status[2] == sp.status[l] and sk.nsteps[2] == sp.nsteps[l], l
        assert (sk.status[2] == CAPTURED) == (sk.hit[2] == 1), l
        n += 1
    return n


def check_crossing(run, mesh, rot=0.0, nring=8, **kw):
    """The crossing field with the default brackets of an nring ring (rotated by rot) for both ordered pairs: each of the
    2 nring-arc rings shows exactly two changes of side; the one facing the other null is FOUND - narrower than tol
    within 8 rounds, its line within OFF_AXIS min(h) of the x' axis, CAPTURED by m', its length within one step of
    |pos' - pos| - (radius + capture) min(h) (the line starts at its seed, rho from m on the axis, and ends at the first
    point within the capture radius of m') -, the one facing away is FAR: its line runs away from m' along the axis, so
    it stays farther from m' than m is; every other arc is NO_CROSSING.  Returns
    the Sep, pair and arc."""
    opt = dict(CROSS_OPT, **kw)
    b, rc, pos, kind, normal, _jac = crossing_case(mesh)
    hmin = min(q[1] - q[0] for q in mesh)
    pair, arc = ring_brackets(ring_of(nring, rot), [(0, 1), (1, 0)])
    sp = run(mesh, b, pos, kind, normal, pair, arc, **opt)
    check_structure(sp, pos, pair, opt["every"])
    sep = np.linalg.norm(pos[1] - pos[0])
    worst = 0.0
    for q, (m, o) in enumerate(((0, 1), (1, 0))):
        sl = slice(q * nring, (q + 1) * nring)
        st = sp.state[sl]
        assert sorted(st.tolist()) == sorted([FOUND, FAR] + [NO_CROSSING] * (nring - 2)), st
        f = q * nring + int(np.nonzero(st == FOUND)[0][0])
        g = q * nring + int(np.nonzero(st == FAR)[0][0])
        assert sp.width[f] <= opt["tol"] and sp.nrounds[f] <= 8 and sp.width[g] <= opt["tol"], (sp.width[sl], sp.nrounds[sl])
        assert np.all(sp.nrounds[sl][st == NO_CROSSING] == 1)
        assert sp.status[f] == CAPTURED
        P = sp.points[sp.offsets[f]:sp.offsets[f + 1]]
        off = np.abs(P[:, 1:] - rc[1:]).max() / hmin
        worst = max(worst, off)
        want = sep - (opt["radius"] + opt["capture"]) * hmin
        print("crossing: null", m, "FOUND bracket", f - q * nring, "rounds", sp.nrounds[f], "width", sp.width[f], "steps",
              sp.nsteps[f], "off axis / min(h)", off, "length", sp.length[f], "expected", want, "dmin / min(h)",
              sp.dmin[f] / hmin, "| FAR bracket", g - q * nring, "rounds", sp.nrounds[g], "dmin / min(h)",
              sp.dmin[g] / hmin)
        assert off <= OFF_AXIS, off
        assert abs(sp.length[f] - want) <= opt["step"] * hmin, (sp.length[f], want)
        assert np.all(sp.dmin[f] <= opt["capture"] * hmin) and np.all(sp.dmin[g] > sep), (sp.dmin[f], sp.dmin[g])
        # the FOUND line runs from m to m' along the axis
        assert np.all(np.diff(np.abs(P[:, 0] - pos[m][0])) > 0.0)
        assert np.linalg.norm(sp.ends[f] - pos[o]) <= opt["capture"] * hmin
    check_crossing.worst = worst
    return sp, pair, arc
