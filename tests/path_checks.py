"""The checks of the field-line paths that do not need the bitwise restatement, written once as functions of a runner:
test_paths_model.py runs them on path_model.paths_numpy, test_gpu_paths.py on the device entries.

    run(mesh, b, g, seeds, step, max_steps, direction, every) -> path_model.Paths

direction +1, -1 or 0 (lane order: the forward block, then the backward block); gpt and ipt are zeros without g."""
import numpy as np

from line_model import (FACES, NULL, OUTSIDE, UNFINISHED, axis_of, box, face_seeds, grids, helical, inner_seeds,
                        uniform_b)
from path_model import npts_of

BV = np.array([0.3, -0.2, 0.9])


def default_max_steps(mesh, step):
    return int(np.ceil(4.0 * sum(len(q) for q in mesh) / step))


def lanes(seeds, direction):
    """(seed, sgn) of every lane"""
    S = np.asarray(seeds, dtype=np.float64)
    if direction == 0:
        return np.concatenate([S, S]), np.concatenate([np.ones(len(S)), -np.ones(len(S))])
    return S, np.full(len(S), float(direction))


def check_structure(p, seeds, direction, every):
    """what holds for every call: offsets from nsteps, the first point the seed, the last point the end, the last
    running integral the integral, the running integral 0 at the seed"""
    S, _sgn = lanes(seeds, direction)
    nl = len(S)
    assert p.offsets.dtype == np.int64 and p.offsets.shape == (nl + 1,)
    counts = npts_of(p.nsteps, every)
    assert np.array_equal(p.offsets, np.concatenate([[0], np.cumsum(counts)])), "offsets are not the formula's"
    total = int(p.offsets[-1])
    assert p.points.shape == (total, 3) and p.bpt.shape == (total, 3) and p.gpt.shape == (total, 3)
    assert p.ipt.shape == (total,)
    first, last = p.offsets[:-1], p.offsets[1:] - 1
    assert p.points[first].tobytes() == S.tobytes(), "the first point is not the seed"
    assert p.points[last].tobytes() == p.ends.tobytes(), "the last point is not the end"
    assert p.ipt[last].tobytes() == p.integral.tobytes(), "the last running integral is not the integral"
    moved = p.nsteps > 0
    assert not np.any(p.ipt[first[moved]]), "the running integral does not start at 0"
    out = p.status == OUTSIDE
    assert np.all(counts[out] == 1) and not np.any(p.bpt[first[out]]) and not np.any(p.gpt[first[out]])
    assert not np.any(p.ipt[first[out]])


def check_stride(p1, pk, k):
    """the rows of every = k are rows 0, k, 2 k, ..., last of every = 1, bit for bit"""
    for a in range(5):
        assert p1[a].tobytes() == pk[a].tobytes()
    rows = []
    for l in range(len(p1.nsteps)):
        a, e = int(p1.offsets[l]), int(p1.offsets[l + 1])
        idx = list(range(a, e - 1, k))
        rows += idx + [e - 1]
    rows = np.array(rows, dtype=np.int64)
    assert len(rows) == int(pk.offsets[-1]), (len(rows), int(pk.offsets[-1]), k)
    for name in ("points", "bpt", "gpt", "ipt"):
        assert getattr(pk, name).tobytes() == getattr(p1, name)[rows].tobytes(), (name, k)


def arc_lengths(p, l, ds, every):
    """the arc length at each stored point of line l: j every ds, and the line's length at the last"""
    n = int(p.offsets[l + 1] - p.offsets[l])
    s = np.arange(n) * (every * ds)
    s[-1] = p.length[l]
    return s


# ---------------------------------------------------------------------------------------------------------------
# uniform field
# ---------------------------------------------------------------------------------------------------------------
def uniform_case(mesh):
    X, Y, Z = grids(mesh)
    return uniform_b(mesh, BV), np.stack([BV[1] * Z, BV[2] * X, BV[0] * Y])


def check_uniform(run, mesh, step=0.37, everys=(1, 3)):
    """B = (0.3, -0.2, 0.9), G = (b_y z, b_z x, b_x y) (test_gpu_trace's field: G.b is linear in arc length, which RK4
    integrates exactly).  Point j lies at seed + sgn j every ds b^ within 1e-12 of the extent (rounding over <= 1e3
    steps, DESIGN's bound for the end points), bpt is B exactly (v0 + f (v1 - v0) with v1 = v0), gpt is G(point) and
    ipt the arc length times G.b^ at the midpoint of seed and point, both within 1e-12 of max |G|."""
    b, g = uniform_case(mesh)
    bh = BV / np.sqrt((BV * BV).sum())
    lo, h, hi, _n = box(mesh)
    scale = np.abs(np.concatenate([lo, hi])).max()
    gmax = np.abs(g).max()
    ds = step * h.min()
    rng = np.random.default_rng(2116)
    seeds = np.concatenate([inner_seeds(mesh, rng, 40), face_seeds(mesh, rng, 2)])

    def gfun(P):
        return np.stack([BV[1] * P[:, 2], BV[2] * P[:, 0], BV[0] * P[:, 1]], axis=1)

    worst = {}
    for every in everys:
        p = run(mesh, b, g, seeds, step, default_max_steps(mesh, step), 0, every)
        check_structure(p, seeds, 0, every)
        assert np.all(np.isin(p.status, list(FACES)))
        S, sgn = lanes(seeds, 0)
        assert np.array_equal(p.bpt, np.broadcast_to(BV, p.bpt.shape)), "bpt is not B exactly"
        e_pos = e_g = e_i = 0.0
        for l in range(len(S)):
            a, e = int(p.offsets[l]), int(p.offsets[l + 1])
            s = arc_lengths(p, l, ds, every)
            want = S[l] + sgn[l] * s[:, None] * bh
            e_pos = max(e_pos, np.abs(p.points[a:e] - want).max() / scale)
            e_g = max(e_g, np.abs(p.gpt[a:e] - gfun(p.points[a:e])).max() / gmax)
            mid = 0.5 * (p.points[a:e] + S[l])
            e_i = max(e_i, np.abs(p.ipt[a:e] - s * (gfun(mid) * bh).sum(axis=1)).max() / gmax)
        print("uniform field, every", every, "errors (position, gpt, ipt):", e_pos, e_g, e_i)
        worst[every] = (e_pos, e_g, e_i)
        assert e_pos <= 1e-12 and e_g <= 1e-12 and e_i <= 1e-12, (every, e_pos, e_g, e_i)
    return worst


# ---------------------------------------------------------------------------------------------------------------
# helical field
# ---------------------------------------------------------------------------------------------------------------
def check_helical(run, mesh, eps=1.5, b0=1.0):
    """Lines of B = (-eps (y - yc), eps (x - xc), B0) from the bottom face wind round the axis at a constant distance
    rho and climb at the constant rate B0 / sqrt(B0^2 + eps^2 rho^2).  Over ALL stored points, the largest error of the
    distance from the axis and of z_j - z_0 - s_j B0 / sqrt(B0^2 + eps^2 rho^2) (s_j = j ds, the length at the last)
    falls by >= 10 per halving of the step while it is above 1e-11 - the factor of the end-point test of the trace
    entries - and the first halving is above it, so the order is shown.  bpt is the field at the point (the field is
    linear: trilinear interpolation is exact) within 1e-12 of max |B|, at the snapped end point too - also on lines
    that leave through the side faces, whose snap moves the point along an axis B depends on.  Returns the errors per
    step."""
    b, _a = helical(mesh, eps, b0)
    lo, h, hi, _n = box(mesh)
    xc, yc = axis_of(mesh)
    rho = np.repeat([0.05, 0.15, 0.3], 4)
    phi0 = np.tile(np.arange(4) * (2 * np.pi / 4) + 0.1, 3)
    seeds = np.stack([xc + rho * np.cos(phi0), yc + rho * np.sin(phi0), np.full(len(rho), lo[2])], axis=1)
    rate = b0 / np.sqrt(b0 * b0 + (eps * rho) ** 2)
    bmax = np.abs(b).max()
    e_rho, e_z = [], []
    for step in (1.0, 0.5, 0.25):
        ds = step * h.min()
        p = run(mesh, b, None, seeds, step, default_max_steps(mesh, step), 1, 1)
        check_structure(p, seeds, 1, 1)
        assert np.all(p.status == 6)
        er = ez = eb = 0.0
        for l in range(len(seeds)):
            a, e = int(p.offsets[l]), int(p.offsets[l + 1])
            P = p.points[a:e]
            s = arc_lengths(p, l, ds, 1)
            er = max(er, np.abs(np.hypot(P[:, 0] - xc, P[:, 1] - yc) - rho[l]).max())
            ez = max(ez, np.abs(P[:, 2] - seeds[l, 2] - s * rate[l]).max())
            want = np.stack([-eps * (P[:, 1] - yc), eps * (P[:, 0] - xc), np.full(len(P), b0)], axis=1)
            eb = max(eb, np.abs(p.bpt[a:e] - want).max() / bmax)
        assert eb <= 1e-12, ("bpt is not the field at the point", step, eb)
        e_rho.append(er)
        e_z.append(ez)
    # lines round the axis from near the four vertical edges leave through the side faces, where the snap moves the
    # end point along an axis B depends on: bpt is the field at the stored point there too, in both directions
    f = np.array([[0.9, 0.9], [0.1, 0.9], [0.1, 0.1], [0.9, 0.1]])
    side = np.stack([lo[0] + f[:, 0] * (hi[0] - lo[0]), lo[1] + f[:, 1] * (hi[1] - lo[1]),
                     np.full(4, 0.5 * (lo[2] + hi[2]))], axis=1)
    p = run(mesh, b, None, side, 0.5, default_max_steps(mesh, 0.5), 0, 2)
    check_structure(p, side, 0, 2)
    assert np.all(p.status <= 4) and np.all(p.nsteps >= 3), (p.status, p.nsteps)
    P = p.points
    want = np.stack([-eps * (P[:, 1] - yc), eps * (P[:, 0] - xc), np.full(len(P), b0)], axis=1)
    eb = np.abs(p.bpt - want).max() / bmax
    assert eb <= 1e-12, ("bpt is not the field at the point on lines that leave through the side faces", eb)
    print("helical field: distance-from-axis errors", e_rho, "height errors", e_z)
    assert e_rho[0] > 1e-11 and e_rho[1] > 1e-11, "rounding took over: the steps are too fine to show the order"
    for e in (e_rho, e_z):
        for coarse, fine in zip(e[:-1], e[1:]):
            if fine > 1e-11:
                assert coarse / fine >= 10.0, e
    return e_rho, e_z


# ---------------------------------------------------------------------------------------------------------------
# other ends
# ---------------------------------------------------------------------------------------------------------------
def check_other_ends(run, mesh):
    """NULL lines at a zero block and at a NaN block, UNFINISHED lines, seeds outside the box and non-finite seeds, a
    seed on a face whose B points outward"""
    lo, h, hi, n = box(mesh)
    X, _Y, _Z = grids(mesh)
    up = np.stack([np.zeros(X.shape), np.zeros(X.shape), np.ones(X.shape)])
    g = np.stack([np.zeros(X.shape), np.zeros(X.shape), np.full(X.shape, 2.0)])
    ci, cj, ck = 2, 1, 3

    def col(i, j, fz):
        return [lo[0] + (i + 0.5) * h[0], lo[1] + (j + 0.5) * h[1], lo[2] + fz * (hi[2] - lo[2])]

    seeds = np.array([col(ci, cj, 0.1), col(ci + 2, cj + 2, 0.1)])
    zc = lo[2] + ck * h[2]
    for bad in (0.0, np.nan):
        b = up.copy()
        b[:, ck:ck + 2, cj:cj + 2, ci:ci + 2] = bad
        for every in (1, 2, 3):
            p = run(mesh, b, g, seeds, 0.5, 200, 1, every)
            check_structure(p, seeds, 1, every)
            assert p.status.tolist() == [NULL, 6], (bad, p.status)
            k = int(p.offsets[1]) - 1
            # the last point is the last accepted point: below the block, within a step of the cells that touch it
            # (a NaN corner spoils the whole cell below the block, a zero corner only the block itself)
            assert zc - h[2] - 0.5 * h.min() < p.points[k, 2] <= zc
            assert p.points[k].tobytes() == p.ends[0].tobytes()
            assert abs(p.points[k, 2] - (seeds[0, 2] + p.length[0])) <= 1e-12
            # B there is stored as it is: between the field below the block and the block's value
            assert not np.any(p.bpt[k, :2]) and (np.isnan(p.bpt[k, 2]) if bad != 0.0 and np.isnan(p.bpt[k, 2])
                                                 else 0.0 <= p.bpt[k, 2] <= 1.0)
            # G.b = 2 along what was traced
            s = p.points[:int(p.offsets[1]), 2] - seeds[0, 2]
            assert np.abs(p.ipt[:int(p.offsets[1])] - 2.0 * s).max() <= 1e-12
    # a seed in the block itself: no step, one point, bpt stored as it is
    for bad in (0.0, np.nan):
        b = up.copy()
        b[:, ck:ck + 2, cj:cj + 2, ci:ci + 2] = bad
        s0 = np.array([[lo[0] + (ci + 0.5) * h[0], lo[1] + (cj + 0.5) * h[1], zc + 0.5 * h[2]]])
        p = run(mesh, b, g, s0, 0.5, 200, 0, 1)
        check_structure(p, s0, 0, 1)
        assert p.status.tolist() == [NULL, NULL] and p.nsteps.tolist() == [0, 0] and p.offsets.tolist() == [0, 1, 2]
        assert np.array_equal(p.bpt, np.full((2, 3), bad), equal_nan=True)
        assert np.array_equal(p.gpt, np.array([[0.0, 0.0, 2.0]] * 2)) and not np.any(p.ipt)
    # closed lines: max_steps steps, (max_steps - 1) / every + 2 points
    b, a = helical(mesh, 1.5, 0.0)
    c = 0.5 * (lo + hi)
    rho = np.array([0.05, 0.1, 0.05, 0.1])
    phi = np.arange(4) * (np.pi / 2) + 0.2
    cs = np.stack([c[0] + rho * np.cos(phi), c[1] + rho * np.sin(phi), lo[2] + (hi[2] - lo[2]) * np.linspace(0, 1, 4)],
                  axis=1)
    for every in (1, 2, 3, 7, 49, 50, 1000):
        p = run(mesh, b, a, cs, 0.5, 50, 0, every)
        check_structure(p, cs, 0, every)
        assert np.all(p.status == UNFINISHED) and np.all(p.nsteps == 50)
        assert np.all(np.diff(p.offsets) == (50 - 1) // every + 2)
        radius = np.hypot(p.points[:, 0] - c[0], p.points[:, 1] - c[1])
        want = np.repeat(np.concatenate([rho, rho]), (50 - 1) // every + 2)
        # RK4 shrinks the radius by theta^6 / 144 of itself per step, theta = ds / rho (the bound of the trace tests)
        ds = 0.5 * h.min()
        assert np.all(np.abs(radius / want - 1.0) <= 50 * (ds / want) ** 6 / 72 + 1e-12)
    # seeds that are not in the box: one point with the seed's bits, NaN included, and zeros
    b, g = uniform_case(mesh)
    out = np.array([[lo[0] - 0.1, c[1], c[2]], [c[0], hi[1] + 1e-9, c[2]], [np.nan, c[1], c[2]],
                    [c[0], np.inf, c[2]], [c[0], c[1], -np.inf], [c[0], c[1], c[2]]])
    for direction in (0, 1, -1):
        p = run(mesh, b, g, out, 0.5, 100, direction, 2)
        check_structure(p, out, direction, 2)
        nd = 2 if direction == 0 else 1
        st = p.status.reshape(nd, len(out))
        assert np.all(st[:, :5] == OUTSIDE) and np.all(st[:, 5] != OUTSIDE)
        assert np.all(np.diff(p.offsets).reshape(nd, len(out))[:, :5] == 1)
    # a seed on a face whose B points outward: one step of length 0, two points - the seed and the end
    top = np.array([[c[0], c[1], hi[2]], [c[0], lo[1], c[2]]])      # b_z > 0 at the top, b_y < 0 at y = lo
    for every in (1, 5):
        p = run(mesh, b, g, top, 0.5, 100, 1, every)
        check_structure(p, top, 1, every)
        assert p.nsteps.tolist() == [1, 1] and p.status.tolist() == [6, 3] and p.offsets.tolist() == [0, 2, 4]
        assert p.points[0::2].tobytes() == top.tobytes() and p.points[1::2].tobytes() == top.tobytes()
        assert not np.any(p.ipt) and np.array_equal(p.bpt, np.broadcast_to(BV, (4, 3)))


# ---------------------------------------------------------------------------------------------------------------
# whole_line (ndsm_amd.whole_line on a FieldPaths made of a runner's result)
# ---------------------------------------------------------------------------------------------------------------
def field_paths(p, nseeds, direction, with_g=True):
    """the ndsm_amd.FieldPaths of a Paths"""
    from ndsm_amd import _lib
    nd = 2 if direction == 0 else 1
    out = [p.ends.reshape(nd, nseeds, 3), p.length.reshape(nd, nseeds), p.integral.reshape(nd, nseeds),
           p.status.reshape(nd, nseeds), p.nsteps.reshape(nd, nseeds)]
    return _lib._field_paths(out, direction, p.offsets, p.points, p.bpt, p.gpt if with_g else None,
                             p.ipt if with_g else None)


def check_whole_line(run, mesh, step=0.37):
    """on the uniform field the joined line is one straight polyline from the foot where B enters to the foot where it
    leaves, equally spaced by ds except for the two exit steps, the seed once; its integral runs from 0 at the entry
    foot to flh at the exit foot"""
    import ndsm_amd
    b, g = uniform_case(mesh)
    bh = BV / np.sqrt((BV * BV).sum())
    lo, h, hi, _n = box(mesh)
    ds = step * h.min()
    seeds = inner_seeds(mesh, np.random.default_rng(2117), 6, margin=0.2)
    p = run(mesh, b, g, seeds, step, default_max_steps(mesh, step), 0, 1)
    fp = field_paths(p, len(seeds), 0)
    for i in range(len(seeds)):
        pts, bb, gg, integ = ndsm_amd.whole_line(fp, i)
        nb, nf = int(fp.lines.nsteps[1, i]), int(fp.lines.nsteps[0, i])
        assert len(pts) == nb + nf + 1 and len(bb) == len(gg) == len(integ) == len(pts)
        assert (pts == seeds[i]).all(axis=1).sum() == 1 and pts[nb].tobytes() == seeds[i].tobytes()
        assert pts[0].tobytes() == fp.lines.ends[1, i].tobytes() and pts[-1].tobytes() == fp.lines.ends[0, i].tobytes()
        d = np.diff(pts, axis=0)
        seg = np.sqrt((d * d).sum(axis=1))
        assert np.abs(d / seg[:, None] - bh).max() <= 1e-9                   # straight, along B everywhere
        assert np.abs(seg[1:-1] - ds).max() <= 1e-12 and seg[0] <= ds + 1e-12 and seg[-1] <= ds + 1e-12
        assert integ[0] == 0.0 and integ[-1] == fp.lines.flh[i]
        path_forward = ndsm_amd.path_of(fp, i)
        assert path_forward[0].tobytes() == pts[nb:].tobytes()
