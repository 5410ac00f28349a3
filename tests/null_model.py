"""What the null-point tests share (test_nulls_model.py on the CPU, test_gpu_nulls.py on the GPU): nulls_numpy, the
numpy restatement of the semantics of ndsm_hip_vecpot_nulls in include/ndsm_hip.h (the screen, the nine starts, the
guards, the record; the device matches it bit for bit), closed-form fields with known nulls, and the closed-form
checks as functions of a runner `run(mesh, b, max_nulls=4096, merge=1e-6) -> Nulls`, so that the same checks run with
the library (VecPot.nulls) and with the restatement behind the same Python layer (model_run)."""
import numpy as np

from line_model import Lines, box, grids, trace_numpy

ITERS, WANDER, CONVERGED, ACCEPT = 20, 2.5, 2.0 ** -40, 2.0 ** -30
STARTS = [(0.5, 0.5, 0.5)] + [(0.75 if s & 1 else 0.25, 0.75 if s & 2 else 0.25, 0.75 if s & 4 else 0.25)
                              for s in range(8)]


# ---------------------------------------------------------------------------------------------------------------
# the numpy restatement of include/ndsm_hip.h
# ---------------------------------------------------------------------------------------------------------------
def _corners(m, base):
    """the 8 corner values of the three components at the cells `base`: (3, 8, n)"""
    nx, nxy = m.nx, m.nx * m.ny
    offs = [0, 1, nx, nx + 1, nxy, nxy + 1, nxy + nx, nxy + nx + 1]
    return np.stack([np.stack([m.bf[c][base + o] for o in offs]) for c in range(3)])


def _value_fgrad(v, fx, fy, fz):
    """value and gradient with respect to the fractions of one component (v: its 8 corners): the expressions of
    Lines.lerp without the quotients by h"""
    d00, d10, d01, d11 = v[1] - v[0], v[3] - v[2], v[5] - v[4], v[7] - v[6]
    c00 = v[0] + fx * d00
    c10 = v[2] + fx * d10
    c01 = v[4] + fx * d01
    c11 = v[6] + fx * d11
    e0, e1 = c10 - c00, c11 - c01
    c0 = c00 + fy * e0
    c1 = c01 + fy * e1
    dz = c1 - c0
    dx0 = d00 + fy * (d10 - d00)
    dx1 = d01 + fy * (d11 - d01)
    return c0 + fz * dz, [dx0 + fz * (dx1 - dx0), e0 + fz * (e1 - e0), dz]


def _det3(J):
    a00 = J[1][1] * J[2][2] - J[1][2] * J[2][1]
    a10 = J[1][2] * J[2][0] - J[1][0] * J[2][2]
    a20 = J[1][0] * J[2][1] - J[1][1] * J[2][0]
    return (J[0][0] * a00 + J[0][1] * a10) + J[0][2] * a20, a00, a10, a20


def _newton(v, nstarts=9):
    """the Newton stage on the corner values v (3, 8, n): accepted (n), the fractions (3, n), iters (n)"""
    n = v.shape[2]
    done = np.zeros(n, dtype=bool)
    F = np.zeros((3, n))
    code = np.zeros(n, dtype=np.int32)
    for s in range(nstarts):
        idx = np.nonzero(~done)[0]
        if len(idx) == 0:
            break
        f = [np.full(len(idx), STARTS[s][d]) for d in range(3)]
        vv = v[:, :, idx]
        alive = np.ones(len(idx), dtype=bool)
        conv = np.zeros(len(idx), dtype=bool)
        its = np.zeros(len(idx), dtype=np.int32)
        for it in range(1, ITERS + 1):
            a = np.nonzero(alive & ~conv)[0]
            if len(a) == 0:
                break
            fa = [f[d][a] for d in range(3)]
            b, J = [], []
            for c in range(3):
                val, g = _value_fgrad(vv[c][:, a], fa[0], fa[1], fa[2])
                b.append(val)
                J.append(g)
            det, a00, a10, a20 = _det3(J)
            a01 = J[0][2] * J[2][1] - J[0][1] * J[2][2]
            a02 = J[0][1] * J[1][2] - J[0][2] * J[1][1]
            a11 = J[0][0] * J[2][2] - J[0][2] * J[2][0]
            a12 = J[0][2] * J[1][0] - J[0][0] * J[1][2]
            a21 = J[0][1] * J[2][0] - J[0][0] * J[2][1]
            a22 = J[0][0] * J[1][1] - J[0][1] * J[1][0]
            ok = np.abs(det) > 0.0
            dd = np.where(ok, det, 1.0)
            delta = [((a00 * b[0] + a01 * b[1]) + a02 * b[2]) / dd, ((a10 * b[0] + a11 * b[1]) + a12 * b[2]) / dd,
                     ((a20 * b[0] + a21 * b[1]) + a22 * b[2]) / dd]
            fn = [fa[d] - delta[d] for d in range(3)]
            for d in range(3):
                ok = ok & (np.abs(fn[d] - 0.5) <= WANDER)
            big = np.maximum(np.maximum(np.abs(delta[0]), np.abs(delta[1])), np.abs(delta[2]))
            cv = ok & (big <= CONVERGED)
            for d in range(3):
                f[d][a] = np.where(ok, fn[d], fa[d])
            alive[a] = ok
            conv[a] = cv
            its[a] = it
        acc = conv.copy()
        for d in range(3):
            acc &= (f[d] >= -ACCEPT) & (f[d] <= 1.0 + ACCEPT)
        done[idx[acc]] = True
        for d in range(3):
            F[d, idx[acc]] = f[d][acc]
        code[idx[acc]] = 32 * s + its[acc]
    return done, F, code


def nulls_numpy(mesh, b, max_nulls, screen=True, nstarts=9):
    """(counts, cell, pos, jac, det, resid, sign, iters) of ndsm_hip_vecpot_nulls: counts = [candidates, found],
    the first max_nulls records in ascending cell.  screen=False: the Newton stage runs on EVERY cell (counts[0] is
    still the screen's)."""
    m = Lines(mesh, b, None, 1.0)
    nx, ny, nz = (int(v) for v in m.n)
    K, J, I = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    base = (I + nx * (J + ny * K)).reshape(-1).astype(np.int64)          # ascending
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = _corners(m, base)
        one_sign = ((v > 0.0).all(axis=1) | (v < 0.0).all(axis=1)).any(axis=0)
        cand = ~one_sign & ~np.isnan(v).any(axis=(0, 1))
        ncand = int(cand.sum())
        if screen:
            base, v = base[cand], v[:, :, cand]
        ok, F, code = _newton(v, nstarts)
        cell, F, code, v = base[ok], F[:, ok], code[ok], v[:, :, ok]
        nfound = len(cell)
        cell, F, code, v = cell[:max_nulls], F[:, :max_nulls], code[:max_nulls], v[:, :, :max_nulls]
        cobj = (cell, F[0], F[1], F[2])
        bv, M = [], []
        for c in range(3):
            val, g = m.lerp(m.bf[c], cobj, grad=True)
            bv.append(val)
            M.append(g)
        det = _det3(M)[0]
        ci = [cell % nx, (cell // nx) % ny, cell // (nx * ny)]
        pos = np.stack([m.lo[d] + (ci[d].astype(np.float64) + F[d]) * m.h[d] for d in range(3)], axis=1)
        jac = np.stack([np.stack(M[c], axis=1) for c in range(3)], axis=1)
        resid = np.sqrt((bv[0] * bv[0] + bv[1] * bv[1]) + bv[2] * bv[2])
        sign = np.where(det < 0.0, 1, np.where(det > 0.0, -1, 0)).astype(np.int32)
    return (np.array([ncand, nfound], dtype=np.int64), cell, pos.reshape(-1, 3), jac.reshape(-1, 3, 3), det, resid,
            sign, code.astype(np.int32))


def model_run(mesh, b, max_nulls=4096, merge=1e-6, device=False, **kw):
    """the restatement behind the interface of VecPot.nulls (the library's own Python layer types the records)"""
    from ndsm_amd import _lib
    out = nulls_numpy(mesh, b, max_nulls, **kw)
    if out[0][1] > max_nulls > 0:
        out = nulls_numpy(mesh, b, int(out[0][1]), **kw)
    hmin = min(q[1] - q[0] for q in mesh)
    return _lib._nulls_tuple(list(out[1:]), int(out[0][0]), int(out[0][1]), None if merge is None else merge * hmin)


def same_records(a, b):
    """two record tuples of nulls_numpy's layout agree bit for bit (NaN == NaN)"""
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=x.dtype.kind == "f") and x.dtype == y.dtype
               for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------
LINEAR = {
    # name: (M, sign, spiral, the analytic spine)
    "radial": (np.diag([2.0, -1.0, -1.0]), -1, False, np.array([1.0, 0.0, 0.0])),
    "radial_neg": (np.diag([-2.0, 1.0, 1.0]), +1, False, np.array([1.0, 0.0, 0.0])),
    "spiral": (np.array([[1.0, -3.0, 0.0], [3.0, 1.0, 0.0], [0.0, 0.0, -2.0]]), +1, True, np.array([0.0, 0.0, 1.0])),
    # upper triangular, not symmetric, three different real eigenvalues 1, 1.5, -2.5 (an improper null, trace 0);
    # (M + 2.5) v = 0: v = (-0.1, -0.075, 1)
    "improper": (np.array([[1.0, 2.0, 0.5], [0.0, 1.5, 0.3], [0.0, 0.0, -2.5]]), +1, False,
                 np.array([-0.1, -0.075, 1.0])),
}
PLACES = {"generic": (0, 1), "face": (1, 2), "edge": (2, 4), "node": (3, 8)}    # axes on a node plane, raw records


def linear_field(mesh, M, r0):
    X, Y, Z = grids(mesh)
    d = [X - r0[0], Y - r0[1], Z - r0[2]]
    return np.stack([M[a][0] * d[0] + M[a][1] * d[1] + M[a][2] * d[2] for a in range(3)])


def place(mesh, where):
    """r0 inside the cell (5, 4, 6): generic fractions, or with the first 1, 2, 3 axes on the cell's low node plane.
    There r0_d is the mesh's own coordinate, so that the field's component is exactly 0 on the plane's nodes (a
    rounded coordinate would leave +-1e-17 there, and the screen rightly drops the cell on the other side: the
    interpolant has no zero in it)"""
    lo, h, _hi, _n = box(mesh)
    c = [5, 4, 6]
    r0 = lo + (np.array(c, dtype=np.float64) + np.array([0.37, 0.61, 0.29])) * h
    for d in range(PLACES[where][0]):
        r0[d] = mesh[d][c[d]]
    return r0


def null_pair(mesh, a=0.1):
    """B = (x'^2 - a^2 + 0.3 y' z', -x' y' + 0.2 z', -x' z' - 0.4 y') about a point near the box's centre (off every
    node plane): divergence-free, nulls at x' = +a (sign -1) and -a (sign +1), y' = z' = 0.  Returns b, centre."""
    lo, _h, hi, _n = box(mesh)
    rc = lo + (hi - lo) * np.array([0.5 + 0.0131, 0.5 - 0.0173, 0.5 + 0.0097])
    X, Y, Z = grids(mesh)
    x, y, z = X - rc[0], Y - rc[1], Z - rc[2]
    return np.stack([x * x - a * a + 0.3 * y * z, -x * y + 0.2 * z, -x * z - 0.4 * y]), rc


def smooth_noise(mesh, seed, amp):
    """a few seeded low-order Fourier modes per component"""
    rng = np.random.default_rng(seed)
    lo, _h, hi, _n = box(mesh)
    X, Y, Z = grids(mesh)
    u = [(X - lo[0]) / (hi[0] - lo[0]), (Y - lo[1]) / (hi[1] - lo[1]), (Z - lo[2]) / (hi[2] - lo[2])]
    out = []
    for _c in range(3):
        f = np.zeros(X.shape)
        for _m in range(4):
            k = rng.integers(1, 4, 3)
            ph = rng.uniform(0.0, 2.0 * np.pi, 3)
            f = f + rng.uniform(-1.0, 1.0) * (np.sin(np.pi * k[0] * u[0] + ph[0]) * np.sin(np.pi * k[1] * u[1] + ph[1]) *
                                              np.sin(np.pi * k[2] * u[2] + ph[2]))
        out.append(amp * f)
    return np.stack(out)


def second_start_cell(mesh):
    """A field, linear plus one bilinear term, with a null that the centre start of its cell misses:
    B = ((x' - a)(y' - b) + e, x' + y' - s, z' - 1/2) in the fractions x', y', z' of the cell (5, 4, 6).  B_y and B_z
    are linear, so after one step every iterate lies on the line y' = s - x', where B_x is a parabola in x' with its
    vertex (x' = 0.4) between two roots: x1' = 0.2 (y1' = 0.3, inside the cell) and x2' = 0.6 (y2' = -0.1, outside).
    Newton on a parabola stays on its side of the vertex: the centre start lands beyond it and converges to x2' -
    outside the cell, so the start fails -; the start (1/4, 1/4, 1/4) lands before it and converges to the null
    inside.  Returns b and the null's position."""
    lo, h, _hi, _n = box(mesh)
    c = np.array([5.0, 4.0, 6.0])
    X, Y, Z = grids(mesh)
    xf, yf, zf = (X - lo[0]) / h[0] - c[0], (Y - lo[1]) / h[1] - c[1], (Z - lo[2]) / h[2] - c[2]
    s, x1, x2, a = 0.5, 0.2, 0.6, 0.1
    # on y' = s - x': (x' - a)(s - b - x') + e = -(x' - x1)(x' - x2)
    bb = a + s - (x1 + x2)
    e = -x1 * x2 + a * (s - bb)
    b = np.stack([(xf - a) * (yf - bb) + e, xf + yf - s, zf - 0.5])
    return b, lo + (c + np.array([x1, s - x1, 0.5])) * h


# ---------------------------------------------------------------------------------------------------------------
# the closed-form checks (each takes the runner)
# ---------------------------------------------------------------------------------------------------------------
def check_linear(run, mesh, name, where):
    """a linear field is reproduced by the interpolant: the position, the Jacobian, the type, the raw record counts
    1, 2, 4, 8 of a null in a cell, on a face, an edge, a node, and one null after merging"""
    M, sign, spiral, spine = LINEAR[name]
    lo, _h, hi, _n = box(mesh)
    r0 = place(mesh, where)
    b = linear_field(mesh, M, r0)
    raw = run(mesh, b, merge=None)
    got = run(mesh, b)
    perr = np.abs(raw.position - r0).max() / (hi - lo).max()
    print("linear", name, where, "raw", len(raw.cell), "merged", len(got.cell), "position error / extent", perr,
          "candidates", got.ncandidates)
    assert len(raw.cell) == PLACES[where][1] == raw.nfound
    assert np.all(np.diff(raw.cell) > 0)                                 # ascending cell order
    assert perr <= 1e-12
    assert len(got.cell) == 1 and got.nfound == raw.nfound and got.cell[0] == raw.cell[0]
    assert np.abs(raw.jacobian - M).max() <= 1e-12 * np.abs(M).max()
    assert np.all(raw.sign == sign) and got.sign[0] == sign
    assert bool(got.spiral[0]) == spiral
    want = np.linalg.eigvals(M)
    assert np.abs(np.sort_complex(got.eigenvalues[0]) - np.sort_complex(want)).max() <= 1e-10
    assert np.sign(np.linalg.det(M)) == -sign and np.all(np.sign(raw.det) == -sign)
    sp = got.spine[0] / np.linalg.norm(got.spine[0])
    assert abs(abs(sp @ spine) / np.linalg.norm(spine) - 1.0) <= 1e-10
    # the lone eigenvalue comes first, and the fan's two span the rest
    lone = got.eigenvalues[0][0]
    assert lone.imag == 0.0 and np.sign(lone.real) == -np.sign(got.eigenvalues[0][1].real) == -np.sign(
        got.eigenvalues[0][2].real)
    assert got.fan.shape == (1, 2, 3)
    assert np.all(raw.residual <= 1e-13 * np.abs(M).max())
    return raw


def check_null_pair(run, meshf, n, a=0.1):
    """the two nulls of null_pair: only x'^2 is not reproduced, its linear-interpolation error lies in [0, h_x^2 / 4],
    so |dx| <= h_x^2 / (8 a) to first order: asserted with 10 % for the second-order term (h_x^2 / (16 a^2) of it)"""
    mesh = meshf([n, n + 3, n - 2])
    b, rc = null_pair(mesh, a)
    hx = mesh[0][1] - mesh[0][0]
    got = run(mesh, b)
    bound = 1.1 * hx * hx / (8.0 * a)
    print("null pair n", n, "found", len(got.cell), "raw", got.nfound, "candidates", got.ncandidates)
    assert len(got.cell) == 2
    order = np.argsort(got.position[:, 0])
    p = got.position[order]
    dx = np.abs(p[:, 0] - (rc[0] + np.array([-a, a])))
    dyz = np.abs(p[:, 1:] - rc[1:]).max()
    print("   |dx|", dx, "bound", bound, "|dy|, |dz| max", dyz)
    assert np.all(dx <= bound)
    assert dyz <= 1e-12
    assert got.sign[order].tolist() == [+1, -1]
    return dx, bound


def check_no_nulls(run, mesh):
    from line_model import helical, hyperbolic, uniform_b
    got = run(mesh, uniform_b(mesh))
    assert got.ncandidates == 0 and got.nfound == 0 and len(got.cell) == 0
    for b in (helical(mesh, 1.5, 1.0)[0], hyperbolic(mesh, 0.8, 1.0), helical(mesh, 0.7, -0.5)[0]):
        got = run(mesh, b)
        assert got.nfound == 0 and len(got.cell) == 0 and got.position.shape == (0, 3)


def failure_fields(mesh):
    """(name, field, candidates or None) of the fields on which the iteration must fail everywhere: all zero (every
    cell a candidate, every start stops at det = 0); a linear null with a NaN block over its cell; the same null with
    +-Inf at corners of its cell"""
    n = [len(q) for q in mesh]
    yield "zero", np.zeros((3, n[2], n[1], n[0])), (n[0] - 1) * (n[1] - 1) * (n[2] - 1)
    b = linear_field(mesh, LINEAR["radial"][0], place(mesh, "generic"))
    bn = b.copy()
    bn[:, 5:9, 3:7, 4:8] = np.nan                     # (k, j, i): covers the cell (5, 4, 6)
    yield "nan block", bn, None
    bi = b.copy()
    bi[0, 6, 4, 5] = np.inf                           # corners of the null's cell
    bi[0, 7, 5, 6] = -np.inf
    bi[1, 6, 5, 5] = -np.inf
    yield "inf corners", bi, None


def check_failure_ends(run, mesh):
    """no null on any of failure_fields (the null they hide is found without the damage)"""
    assert run(mesh, linear_field(mesh, LINEAR["radial"][0], place(mesh, "generic"))).nfound == 1
    for name, b, ncand in failure_fields(mesh):
        got = run(mesh, b)
        assert got.nfound == 0 and len(got.cell) == 0 and got.position.shape == (0, 3), name
        assert ncand is None or got.ncandidates == ncand, name


def check_near_plane(run, mesh, eps=1e-11):
    """The acceptance tolerance at work by construction: the nulls of the spiral and the improper field eps h_x to
    the high side of the node plane x = x_5.  Their B_x changes sign over the corners of both cells that share the
    plane, so both are candidates; the iteration of the lower cell converges to f_x = 1 + eps - outside the cell,
    inside the tolerance 2^-30 - and both cells report the null: two raw records, one after merging.  With a
    tolerance of 0 the lower cell's record is lost."""
    lo, h, hi, _n = box(mesh)
    for name in ("spiral", "improper"):
        r0 = place(mesh, "face")
        r0[0] = r0[0] + eps * h[0]
        b = linear_field(mesh, LINEAR[name][0], r0)
        raw = run(mesh, b, merge=None)
        print("near plane", name, "raw", len(raw.cell), raw.cell)
        assert len(raw.cell) == 2 and raw.cell[1] - raw.cell[0] == 1, (name, raw.cell)
        assert np.abs(raw.position - r0).max() <= 1e-12 * (hi - lo).max()
        assert len(run(mesh, b).cell) == 1


def check_second_start(run, mesh):
    """the null of second_start_cell is found, and not from the centre start"""
    b, r0 = second_start_cell(mesh)
    lo, _h, hi, n = box(mesh)
    raw = run(mesh, b, merge=None)
    cell = 5 + int(n[0]) * (4 + int(n[1]) * 6)
    assert cell in raw.cell.tolist(), raw.cell
    i = raw.cell.tolist().index(cell)
    assert np.abs(raw.position[i] - r0).max() <= 1e-12 * (hi - lo).max()
    return raw


def spine_approach(run, tracer, mesh, steps=(1.0, 0.25), dist=4.4):
    """On the linear null "radial" a line is started on the spine at `dist` min(h) from the null found by `run` and
    traced towards it for ceil(dist / step) steps with tracer(mesh, b, seeds, step, max_steps, sgn) -> ends: the
    distances of its end from the null, per step"""
    M = LINEAR["radial"][0]
    r0 = place(mesh, "generic")
    b = linear_field(mesh, M, r0)
    got = run(mesh, b)
    assert len(got.cell) == 1
    hmin = min(q[1] - q[0] for q in mesh)
    seed = got.position[0] + dist * hmin * got.spine[0] / np.linalg.norm(got.spine[0])
    sgn = -1.0 if got.eigenvalues[0][0].real > 0.0 else 1.0           # B leaves the null along this spine: go back
    out = []
    for step in steps:
        end = tracer(mesh, b, seed[None, :], step, int(np.ceil(dist / step)), sgn)
        out.append(float(np.linalg.norm(end - got.position[0])) / hmin)
    print("spine approach: distance of the line's end from the null / min(h), per step", dict(zip(steps, out)))
    return out


def numpy_tracer(mesh, b, seeds, step, max_steps, sgn):
    return trace_numpy(mesh, b, None, seeds, step, max_steps, sgn)[0][0]
