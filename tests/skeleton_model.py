"""What the skeleton tests share (test_skeleton_model.py on the CPU, test_gpu_skeleton.py on the GPU): skeleton_numpy,
the numpy restatement of the semantics of ndsm_hip_vecpot_skeleton in include/ndsm_hip.h on line_model.Lines, in the
header's operand order (the device matches it bit for bit) - type_numpy, the type of each null from its Jacobian;
seeds_numpy, the seeds and directions of its lanes; lines_numpy, path_model.path_numpy's loop with a direction per lane
and the capture test -, the separator field of DESIGN.md, and the closed-form checks as functions of a runner

    run(mesh, b, pos, jac, ring, radius, capture, step, max_steps, every) -> Skel

so that the same checks run on the restatement and on the device entries."""
import collections

import numpy as np

from line_model import NULL, OUTSIDE, UNFINISHED, Lines, box, grids
from null_model import LINEAR, _det3, linear_field, nulls_numpy, place
from path_model import npts_of, path_numpy

CAPTURED, NONE = 10, 11
NEWTON_ITERS, CONVERGED = 40, 2.0 ** -40

Skel = collections.namedtuple("Skel", ["kind", "eig", "spine", "normal", "ends", "length", "status", "nsteps", "hit",
                                       "offsets", "points", "bpt"])
NAMES = Skel._fields


# ---------------------------------------------------------------------------------------------------------------
# the numpy restatement of include/ndsm_hip.h
# ---------------------------------------------------------------------------------------------------------------
def _pick(vecs):
    """of three vectors (each a list of three arrays) the one with the largest sum of squares (the lowest index on a
    tie), normalised, its component of largest modulus (the lowest index on a tie) positive; ok: that sum is > 0"""
    ss = [(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] for v in vecs]
    best = ss[0].copy()
    out = [c.copy() for c in vecs[0]]
    for k in (1, 2):
        take = ss[k] > best
        best = np.where(take, ss[k], best)
        out = [np.where(take, vecs[k][d], out[d]) for d in range(3)]
    ok = best > 0.0
    nrm = np.sqrt(np.where(ok, best, 1.0))
    out = [c / nrm for c in out]
    big, lead = np.abs(out[0]), out[0]
    take = np.abs(out[1]) > big
    big, lead = np.where(take, np.abs(out[1]), big), np.where(take, out[1], lead)
    lead = np.where(np.abs(out[2]) > big, out[2], lead)
    flip = lead < 0.0
    return ok, [np.where(flip, -c, c) for c in out]


def type_numpy(jac):
    """stage 1: (ok, s, kind, eig, spine, normal, e1, e2) of the Jacobians jac (n,3,3); the vectors are (n,3), zero
    where not ok"""
    M = np.asarray(jac, dtype=np.float64).reshape(-1, 3, 3)
    n = len(M)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        J = [[M[:, a, d] for d in range(3)] for a in range(3)]
        det = _det3(J)[0]
        s = np.where(det > 0.0, 1.0, np.where(det < 0.0, -1.0, 0.0))
        ok = s != 0.0
        N = [[s * J[a][d] for d in range(3)] for a in range(3)]
        ca = (N[0][0] + N[1][1]) + N[2][2]
        cb = (((N[0][0] * N[1][1] - N[0][1] * N[1][0]) + (N[0][0] * N[2][2] - N[0][2] * N[2][0])) +
              (N[1][1] * N[2][2] - N[1][2] * N[2][1]))
        cc = _det3(N)[0]
        ss = N[0][0] * N[0][0]
        for a, d in ((0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)):
            ss = ss + N[a][d] * N[a][d]
        mu = np.sqrt(ss)
        conv = np.zeros(n, dtype=bool)
        iters = np.zeros(n, dtype=np.int32)
        for it in range(NEWTON_ITERS):
            go = ok & ~conv
            if not go.any():
                break
            pv = ((mu - ca) * mu + cb) * mu - cc
            dp = (3.0 * mu - 2.0 * ca) * mu + cb
            delta = pv / dp
            mun = mu - delta
            mu = np.where(go, mun, mu)
            iters[go] = it + 1
            conv |= go & (np.abs(delta) <= CONVERGED * np.abs(mun))
        ok = ok & conv & (mu > 0.0)
        t = ca - mu
        ok = ok & (t < 0.0)
        K = [[N[a][d] - mu if a == d else N[a][d] for d in range(3)] for a in range(3)]
        A = [[K[1][1] * K[2][2] - K[1][2] * K[2][1], K[0][2] * K[2][1] - K[0][1] * K[2][2],
              K[0][1] * K[1][2] - K[0][2] * K[1][1]],
             [K[1][2] * K[2][0] - K[1][0] * K[2][2], K[0][0] * K[2][2] - K[0][2] * K[2][0],
              K[0][2] * K[1][0] - K[0][0] * K[1][2]],
             [K[1][0] * K[2][1] - K[1][1] * K[2][0], K[0][1] * K[2][0] - K[0][0] * K[2][1],
              K[0][0] * K[1][1] - K[0][1] * K[1][0]]]
        okv, v = _pick([[A[0][j], A[1][j], A[2][j]] for j in range(3)])      # the columns
        okw, w = _pick([[A[i][0], A[i][1], A[i][2]] for i in range(3)])      # the rows
        ok = ok & okv & okw
        # the fan basis: the squash entry's start rule with w in place of e
        j = np.zeros(n, dtype=np.int64)
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
        p2 = cc / mu
        disc = t * t - 4.0 * p2
        kind = np.where(ok, np.where(s > 0.0, -1, 1) * np.where(disc < 0.0, 2, 1), 0).astype(np.int32)
        eig = np.where(ok[:, None], np.stack([s * mu, s * t, p2], axis=1), 0.0)

        def vec(x):
            return np.where(ok[:, None], np.stack(x, axis=1), 0.0)
    type_numpy.last_iters = iters
    return ok, s, kind, eig, vec(v), vec(w), vec(e1), vec(e2)


def seeds_numpy(mesh, pos, jac, ring, radius):
    """the per-null outputs and (seeds (nl,3), sgn (nl)) of the lanes l = m L + q; sgn 0: a null without a type"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    ok, s, kind, eig, v, w, e1, e2 = type_numpy(jac)
    _lo, h, _hi, _n = box(mesh)
    rho = radius * min(h[0], h[1], h[2])
    n, L = len(pos), 2 + len(ring)
    seeds = np.zeros((n, L, 3))
    sgn = np.zeros((n, L))
    with np.errstate(invalid="ignore", over="ignore"):
        seeds[:, 0] = pos + rho * v
        seeds[:, 1] = pos - rho * v
        for q in range(len(ring)):
            seeds[:, 2 + q] = pos + rho * (ring[q, 0] * e1 + ring[q, 1] * e2)
    sgn[:, :2] = s[:, None]
    sgn[:, 2:] = -s[:, None]
    seeds[~ok] = pos[~ok, None, :]
    sgn[~ok] = 0.0
    return (kind, eig, v, w), seeds.reshape(-1, 3), sgn.reshape(-1)


def lines_numpy(mesh, b, seeds, sgn, own, pos, capture, step, max_steps, every):
    """stage 2 (path_model.path_numpy's loop with a direction per lane and the capture test): ends, length, status,
    nsteps, hit, offsets, points, bpt of the lanes; own: the null of each lane"""
    m = Lines(mesh, b, None, step)
    ds = m.ds
    cr = capture * min(m.h[0], m.h[1], m.h[2])
    cap2 = cr * cr
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)

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
    hit = np.full(nl, -1, dtype=np.int32)
    none = sgn == 0.0
    inside = m.inside(r)
    status[~inside] = OUTSIDE
    status[none] = NONE
    runs = inside & ~none
    act = np.nonzero(runs)[0]
    rec = [[] for _ in range(nl)]
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
            ok2, rn2 = rk4(ra, sg, k1, s)
            null = ~ok | (leave & ~ok2)
            leave = leave & ok2
            snapped = m.snap(rn2, face)
            go = ok & ~leave & ~null
            ia = act
            if it % every == 0:
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
            if cap2 > 0.0 and len(act) and len(pos):
                # the first other null within the capture radius, in ascending order
                d = r[act][:, None, :] - pos[None, :, :]
                d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
                near = (d2 <= cap2) & (np.arange(len(pos))[None, :] != own[act][:, None])
                got = near.any(axis=1)
                hit[act[got]] = np.argmax(near[got], axis=1)
                status[act[got]] = CAPTURED
                act = act[~got]
        bl = np.zeros((nl, 3))
        ins = np.nonzero(runs)[0]
        if len(ins):
            bl[ins] = stage(r[ins], sgn[ins])[2]
    for l in range(nl):
        rec[l].append((r[l].copy(), bl[l]))
    counts = np.array([len(x) for x in rec], dtype=np.int64)
    assert np.array_equal(counts, npts_of(nsteps, every)), (counts, nsteps, every)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    flat = [x for line in rec for x in line]
    points = np.array([x[0] for x in flat]).reshape(-1, 3)
    bpt = np.array([x[1] for x in flat]).reshape(-1, 3)
    return r, length, status, nsteps, hit, offsets, points, bpt


def skeleton_numpy(mesh, b, pos, jac, ring, radius, capture, step, max_steps, every):
    """the Skel of one call of ndsm_hip_vecpot_skeleton"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    pernull, seeds, sgn = seeds_numpy(mesh, pos, jac, ring, radius)
    own = np.repeat(np.arange(len(pos)), 2 + len(ring))
    return Skel(*pernull, *lines_numpy(mesh, b, seeds, sgn, own, pos, capture, step, max_steps, every))


def same_skel(got, want, what, upto=None):
    """bit for bit (NaN == NaN by its bits); upto: the point arrays of `got` hold the first upto slots only"""
    for k, name in enumerate(NAMES):
        w = want[k] if upto is None or k < 10 else want[k][:upto]
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (what, name, got[k].dtype, got[k].shape, w.shape)
        assert got[k].tobytes() == w.tobytes(), (what, name)


def default_ring(nring):
    """(c_j, s_j) of the angles 2 pi (j + 1/2) / nring"""
    ang = 2.0 * np.pi * (np.arange(nring) + 0.5) / max(nring, 1)
    return np.stack([np.cos(ang), np.sin(ang)], axis=1).reshape(nring, 2)


def model_run(mesh, b, nulls=None, radius=0.5, nring=16, ring=None, capture=None, step=0.5, max_steps=None, every=1,
              **_kw):
    """the restatement behind the interface of VecPot.skeleton (the library's own Python layer forms the Skeleton)"""
    from ndsm_amd import _lib
    if nulls is None:
        import null_model
        nulls = null_model.model_run(mesh, b)
    pos, jac = _lib._skeleton_nulls(nulls)
    ring = _lib._skeleton_ring(nring, ring)
    if max_steps is None:
        max_steps = int(np.ceil(4.0 * sum(len(q) for q in mesh) / step))
    sk = skeleton_numpy(mesh, b, pos, jac, ring, radius, radius if capture is None else capture, step, max_steps, every)
    return _lib._skeleton_tuple(pos, len(ring), list(sk[:4]), list(sk[4:9]), sk.offsets, sk.points, sk.bpt)


# ---------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------
SEP_FRACTIONS = np.array([0.47, 0.52, 0.45])


def separator_field(mesh, a=0.2, k=1.0):
    """B = (x'^2 - a^2, k x' y', -(2 + k) x' z') about the point at the fractions SEP_FRACTIONS of the box, a in units
    of the x extent: divergence-free, nulls at x' = -+a with signs (-1, +1) whose fans are both the plane z' = 0 and meet
    along the separator y' = z' = 0.  Only x'^2 is not reproduced by the interpolant; the planes y' = 0 and z' = 0
    stay invariant.  Returns b, the centre and a in physical units."""
    lo, _h, hi, _n = box(mesh)
    rc = lo + (hi - lo) * SEP_FRACTIONS
    aa = a * (hi[0] - lo[0])
    X, Y, Z = grids(mesh)
    x, y, z = X - rc[0], Y - rc[1], Z - rc[2]
    return np.stack([x * x - aa * aa, k * x * y, -(2.0 + k) * x * z]), rc, aa


def noise_nulls(mesh, seed=11):
    """white noise U(-1, 1) on the mesh and the records of its nulls (nulls_numpy): b, pos (n,3), jac (n,3,3)"""
    n = [len(q) for q in mesh]
    b = np.random.default_rng(seed).uniform(-1.0, 1.0, (3, n[2], n[1], n[0]))
    rec = nulls_numpy(mesh, b, 1 << 20)
    return b, rec[2], rec[3]


# ---------------------------------------------------------------------------------------------------------------
# the closed-form checks (each takes the runner)
# ---------------------------------------------------------------------------------------------------------------
def check_structure(sk, pos, nring, every):
    """what holds for every call: shapes, offsets from nsteps, the last point the end, hit only on captured lines"""
    n, L = len(pos), 2 + nring
    nl = n * L
    assert sk.kind.shape == (n,) and sk.kind.dtype == np.int32
    assert sk.eig.shape == sk.spine.shape == sk.normal.shape == (n, 3)
    assert sk.ends.shape == (nl, 3) and sk.length.shape == sk.status.shape == sk.nsteps.shape == sk.hit.shape == (nl,)
    assert sk.offsets.dtype == np.int64 and sk.offsets.shape == (nl + 1,)
    assert np.array_equal(sk.offsets, np.concatenate([[0], np.cumsum(npts_of(sk.nsteps, every))]))
    total = int(sk.offsets[-1])
    assert sk.points.shape == sk.bpt.shape == (total, 3)
    last = sk.offsets[1:] - 1
    assert sk.points[last].tobytes() == sk.ends.tobytes(), "the last point is not the end"
    assert np.array_equal(sk.hit >= 0, sk.status == CAPTURED)
    assert np.all(sk.hit < n) and np.all(sk.hit != np.repeat(np.arange(n), L))
    none = np.repeat(sk.kind == 0, L)
    assert np.array_equal(sk.status == NONE, none)
    assert np.all(sk.nsteps[none] == 0) and not np.any(sk.length[none])


def linear_case(mesh, name):
    """the linear null `name` of null_model.LINEAR at place(mesh, "generic"): b, r0, M"""
    M = LINEAR[name][0]
    r0 = place(mesh, "generic")
    return linear_field(mesh, M, r0), r0, M


def check_linear(run, mesh, name, nring=8, radius=0.5, step=0.5):
    """A linear field is reproduced by the interpolant, so the null's record is (r0, M) up to rounding (the record is
    taken from nulls_numpy: the nulls entry's bits).  kind, eig, spine and normal against numpy.linalg.eig of M and M^T
    (eigenvalues within 1e-12 relative, vectors parallel within 1e-12); every spine point on r0 + tau v within 1e-12 of
    the extent (the direction is constant along that line, so RK4 is exact), both spine lines end on the face where
    the straight line leaves the box; every fan point within 1e-12 of the extent of the plane w.(r - r0) = 0."""
    b, r0, M = linear_case(mesh, name)
    rec = nulls_numpy(mesh, b, 16)
    assert rec[0][1] == 1
    pos, jac = rec[2], rec[3]
    lo, h, hi, _n = box(mesh)
    extent = (hi - lo).max()
    ring = default_ring(nring)
    max_steps = int(np.ceil(4.0 * sum(len(q) for q in mesh) / step))
    sk = run(mesh, b, pos, jac, ring, radius, 0.0, step, max_steps, 1)
    check_structure(sk, pos, nring, 1)
    # the type against numpy.linalg.eig
    lam, vec = np.linalg.eig(M)
    sdet = np.sign(np.linalg.det(M))
    lone = [k for k in range(3) if abs(lam[k].imag) == 0.0 and np.sign(lam[k].real) == sdet]
    assert len(lone) == 1
    k = lone[0]
    rest = [q for q in range(3) if q != k]
    assert np.sign(sk.kind[0]) == -sdet == LINEAR[name][1]
    spiral = LINEAR[name][2]
    if spiral:
        assert abs(sk.kind[0]) == 2, "the spiral null is not marked"
    elif abs(lam[rest[0]] - lam[rest[1]]) > 0.0:
        # (two equal fan eigenvalues - the radial nulls - sit on the boundary of the spiral test, where the rounding
        # of the record decides: only the sign of kind is asserted there)
        assert abs(sk.kind[0]) == 1
    want = np.array([lam[k].real, (lam[rest[0]] + lam[rest[1]]).real, (lam[rest[0]] * lam[rest[1]]).real])
    e_eig = np.abs(sk.eig[0] - want).max() / np.abs(lam).max()
    v = vec[:, k].real
    lamT, vecT = np.linalg.eig(M.T)
    w = vecT[:, int(np.argmin(np.abs(lamT - lam[k])))].real
    e_v = 1.0 - abs(sk.spine[0] @ v) / np.linalg.norm(v)
    e_w = 1.0 - abs(sk.normal[0] @ w) / np.linalg.norm(w)
    print("linear", name, "kind", sk.kind[0], "eig error", e_eig, "spine, normal misalignment", e_v, e_w)
    assert e_eig <= 1e-12 and abs(e_v) <= 1e-12 and abs(e_w) <= 1e-12
    assert abs(np.linalg.norm(sk.spine[0]) - 1.0) <= 1e-15 and abs(np.linalg.norm(sk.normal[0]) - 1.0) <= 1e-15
    assert sk.spine[0][np.argmax(np.abs(sk.spine[0]))] > 0.0 and sk.normal[0][np.argmax(np.abs(sk.normal[0]))] > 0.0
    # the spine lines: straight, away from the null, to the face where the straight line leaves the box
    vh = v / np.linalg.norm(v)
    e_line = 0.0
    for q, side in ((0, 1.0), (1, -1.0)):
        P = sk.points[sk.offsets[q]:sk.offsets[q + 1]]
        d = P - r0
        tau = d @ vh
        e_line = max(e_line, np.abs(d - tau[:, None] * vh).max() / extent)
        dirn = side * np.sign(sk.spine[0] @ vh) * vh
        assert np.all(np.diff(tau * np.sign(dirn @ vh)) > 0.0), "a spine line does not run away from its null"
        with np.errstate(divide="ignore"):
            tt = np.where(dirn > 0.0, (hi - r0) / dirn, np.where(dirn < 0.0, (lo - r0) / dirn, np.inf))
        ax = int(np.argmin(tt))
        assert sk.status[q] == 1 + 2 * ax + (1 if dirn[ax] > 0.0 else 0), (q, sk.status[q], ax)
        assert np.abs(sk.ends[q] - (r0 + tt[ax] * dirn)).max() <= 1e-12 * extent
    # every seed at rho = radius min(h) from the null
    rho = radius * h.min()
    first = sk.points[sk.offsets[:-1]]
    assert np.abs(np.linalg.norm(first - pos[0], axis=1) - rho).max() <= 1e-14 * extent, "a seed is not at rho"
    # the fan lines: in the fan plane, away from the null
    wh = w / np.linalg.norm(w)
    F = sk.points[sk.offsets[2]:]
    e_fan = np.abs((F - r0) @ wh).max() / extent
    print("   spine points off the line / extent", e_line, "fan points off the plane / extent", e_fan)
    assert e_line <= 1e-12 and e_fan <= 1e-12
    assert np.all(sk.status[2:] <= 6) and np.all(sk.nsteps[2:] >= 2)
    # a capture radius that reaches back to the line's own null changes nothing: there is no other null
    same_skel(run(mesh, b, pos, jac, ring, radius, 3.0, step, max_steps, 1), sk, "capture 3 with one null")
    for q in range(2, 2 + nring):
        P = sk.points[sk.offsets[q]:sk.offsets[q + 1]]
        dist = np.linalg.norm(P - r0, axis=1)
        assert dist[-1] > dist[0], "a fan line does not run away from its null"
    return sk


def check_equals_paths(sk, mesh, b, pos, jac, ring, radius, step, max_steps, every, captured_of=None):
    """the property of the header: every line of sk equals path_numpy of its seed and direction bit for bit - all of it
    for a line that was not captured, its first n steps for a captured line (its end is that line's point n)"""
    _pernull, seeds, sgn = seeds_numpy(mesh, pos, jac, ring, radius)
    for sg in (1.0, -1.0):
        idx = np.nonzero(sgn == sg)[0]
        if len(idx) == 0:
            continue
        ref = path_numpy(mesh, b, None, seeds[idx], step, max_steps, sg, every)
        ref1 = ref if every == 1 else path_numpy(mesh, b, None, seeds[idx], step, max_steps, sg, 1)
        for a, l in enumerate(idx):
            P = sk.points[sk.offsets[l]:sk.offsets[l + 1]]
            Bp = sk.bpt[sk.offsets[l]:sk.offsets[l + 1]]
            R = ref.points[ref.offsets[a]:ref.offsets[a + 1]]
            Rb = ref.bpt[ref.offsets[a]:ref.offsets[a + 1]]
            if sk.status[l] != CAPTURED:
                assert sk.ends[l].tobytes() == ref.ends[a].tobytes() and sk.length[l] == ref.length[a], l
                assert sk.status[l] == ref.status[a] and sk.nsteps[l] == ref.nsteps[a], l
                assert P.tobytes() == R.tobytes() and Bp.tobytes() == Rb.tobytes(), l
            else:
                n = int(sk.nsteps[l])
                assert 1 <= n <= ref.nsteps[a], l
                full = ref1.points[ref1.offsets[a]:ref1.offsets[a + 1]]
                fullb = ref1.bpt[ref1.offsets[a]:ref1.offsets[a + 1]]
                rows = list(range(0, n, every)) + [n]
                assert P.tobytes() == full[rows].tobytes(), l
                # (point n of the uncaptured line carries the B interpolated at the same r: its stage-1 value, or its
                # own last evaluation)
                assert Bp.tobytes() == fullb[rows].tobytes(), l
                assert sk.ends[l].tobytes() == full[n].tobytes(), l
    none = sgn == 0.0
    first = sk.offsets[:-1]
    assert np.all(np.diff(sk.offsets)[none] == 1)
    own_pos = np.repeat(np.asarray(pos).reshape(-1, 3), 2 + len(ring), axis=0)
    assert sk.points[first[none]].tobytes() == own_pos[none].tobytes()
    assert not np.any(sk.bpt[first[none]])


def check_separator(run, mesh, radius, nring=8, capture=0.5, step=0.5, max_steps=4000):
    """The separator field: the two nulls (nulls_numpy, merged by the Python layer's rule) with signs (-1, +1) in x
    order; of each ring exactly the seeds on the side facing the other null are captured by it, within about 50 steps;
    the others leave through an x face and never come within 4.5 min(h) of the other null.  Returns the Skel, the
    nulls' pos and jac and the connections [(m, m', ring indices)]."""
    from ndsm_amd import _lib
    b, rc, aa = separator_field(mesh)
    hmin = min(q[1] - q[0] for q in mesh)
    rec = nulls_numpy(mesh, b, 64)
    nul = _lib._nulls_tuple(list(rec[1:]), int(rec[0][0]), int(rec[0][1]), 1e-6 * hmin)
    assert len(nul.cell) == 2, len(nul.cell)
    order = np.argsort(nul.position[:, 0])
    pos, jac = nul.position[order], nul.jacobian[order]
    assert nul.sign[order].tolist() == [-1, 1]
    ring = np.stack([np.cos((np.arange(nring) + 0.5) * 2.0 * np.pi / nring),
                     np.sin((np.arange(nring) + 0.5) * 2.0 * np.pi / nring)], axis=1)
    sk = run(mesh, b, pos, jac, ring, radius, capture, step, max_steps, 1)
    check_structure(sk, pos, nring, 1)
    assert sk.kind.tolist() == [-1, 1]
    L = 2 + nring
    _pernull, seeds, _sgn = seeds_numpy(mesh, pos, jac, ring, radius)
    out = []
    for m, other in ((0, 1), (1, 0)):
        fan = np.arange(m * L + 2, (m + 1) * L)
        facing = (seeds[fan] - pos[m]) @ (pos[other] - pos[m]) > 0.0
        assert facing.sum() == nring // 2
        assert np.array_equal(sk.status[fan] == CAPTURED, facing), (m, sk.status[fan], facing)
        assert np.all(sk.hit[fan][facing] == other)
        print("separator: null", m, "captured lines' steps", sk.nsteps[fan][facing], "others'", sk.nsteps[fan][~facing],
              sk.status[fan][~facing])
        assert np.all(sk.nsteps[fan][facing] <= 60)
        assert np.all(np.isin(sk.status[fan][~facing], (1, 2)))
        for l in fan[~facing]:
            P = sk.points[sk.offsets[l]:sk.offsets[l + 1]]
            assert np.linalg.norm(P - pos[other], axis=1).min() >= 4.5 * hmin
        # the spines leave the fan plane z' = 0 along z and are not captured
        assert np.all(sk.hit[m * L:m * L + 2] == -1)
        out.append((m, other, np.nonzero(facing)[0]))
    return sk, pos, jac, out


def check_no_type(run, mesh, nring=3):
    """an all-zero Jacobian, a NaN Jacobian and diag(1, 2, 3) (a source: no lone eigenvalue) next to a proper null:
    status NONE on all L lines of each, one point each with pos's bits, zeros elsewhere; the proper null's lines are
    what they are without the others (capture off)"""
    b, r0, M = linear_case(mesh, "improper")
    lo, _h, hi, _n = box(mesh)
    c = 0.5 * (lo + hi)
    pos = np.stack([c, r0, c + 0.01, np.array([np.nan, c[1], c[2]]), c - 0.02])
    jac = np.stack([np.zeros((3, 3)), M, np.full((3, 3), np.nan), M, np.diag([1.0, 2.0, 3.0])])
    jac[3] = 0.0
    ring = default_ring(nring)
    sk = run(mesh, b, pos, jac, ring, 0.5, 0.0, 0.5, 200, 2)
    check_structure(sk, pos, nring, 2)
    L = 2 + nring
    assert sk.kind.tolist() == [0, sk.kind[1], 0, 0, 0] and sk.kind[1] != 0
    for m in (0, 2, 3, 4):
        sl = slice(m * L, (m + 1) * L)
        assert np.all(sk.status[sl] == NONE) and np.all(sk.nsteps[sl] == 0) and np.all(sk.hit[sl] == -1)
        assert np.all(np.diff(sk.offsets)[sl] == 1)
        rows = sk.offsets[:-1][sl]
        assert sk.points[rows].tobytes() == np.repeat(pos[[m]], L, axis=0).tobytes()
        assert sk.ends[sl].tobytes() == np.repeat(pos[[m]], L, axis=0).tobytes()
        assert not np.any(sk.bpt[rows]) and not np.any(sk.length[sl])
        assert not np.any(sk.eig[m]) and not np.any(sk.spine[m]) and not np.any(sk.normal[m])
    alone = run(mesh, b, pos[[1]], jac[[1]], ring, 0.5, 0.0, 0.5, 200, 2)
    a, e = int(sk.offsets[L]), int(sk.offsets[2 * L])
    assert sk.points[a:e].tobytes() == alone.points.tobytes() and sk.bpt[a:e].tobytes() == alone.bpt.tobytes()
    for name in ("ends", "length", "status", "nsteps", "hit"):
        assert getattr(sk, name)[L:2 * L].tobytes() == getattr(alone, name).tobytes(), name
    return sk
