"""What the field-line tests share (test_gpu_trace.py, test_gpu_squash.py): the box of a mesh as the library forms
it, closed-form fields, seed generators, and the numpy restatements of the line semantics in include/ndsm_hip.h -
trace_numpy (ndsm_hip_vecpot_trace) and squash_numpy (ndsm_hip_vecpot_squash), which the device matches bit for
bit.  The two restatements share one cell / corner gather / trilinear blend (value, and value with gradient) /
first-face search / snap: the class Lines, the counterpart of ndsm_amd/csrc/line.hpp."""
import numpy as np

FACES = range(1, 7)          # TRACE_XLO .. TRACE_ZHI
NULL, UNFINISHED, OUTSIDE = 7, 8, 9


# ---------------------------------------------------------------------------------------------------------------
# mesh, box, grids
# ---------------------------------------------------------------------------------------------------------------
def box(mesh):
    """lo, h, hi per axis as the library forms them: h = q[1] - q[0], hi = lo + (n - 1) h"""
    lo = np.array([q[0] for q in mesh])
    h = np.array([q[1] - q[0] for q in mesh])
    n = np.array([len(q) for q in mesh])
    return lo, h, lo + (n - 1.0) * h, n


def grids(mesh):
    return np.meshgrid(mesh[2], mesh[1], mesh[0], indexing="ij")[::-1]   # X, Y, Z, each (nz, ny, nx)


def weights1(q):
    w = np.full(len(q), q[1] - q[0])
    w[0] = w[-1] = 0.5 * (q[1] - q[0])
    return w


def centre(mesh):
    lo, _h, hi, _n = box(mesh)
    return 0.5 * (lo + hi)


def axis_of(mesh, axis=(0.5, 0.5)):
    lo, _h, hi, _n = box(mesh)
    return lo[0] + axis[0] * (hi[0] - lo[0]), lo[1] + axis[1] * (hi[1] - lo[1])


# ---------------------------------------------------------------------------------------------------------------
# the numpy restatements of include/ndsm_hip.h
# ---------------------------------------------------------------------------------------------------------------
class Lines:
    """the mesh, the fields and the step of one call, and what every line does with them (points P: (n,3) arrays)"""

    def __init__(self, mesh, b, g, step):
        self.lo, self.h, self.hi, self.n = box(mesh)
        self.nx, self.ny = int(self.n[0]), int(self.n[1])
        self.ds = step * min(self.h[0], self.h[1], self.h[2])
        self.bf = b.reshape(3, -1)
        self.gf = None if g is None else g.reshape(3, -1)

    def cell(self, P):
        """base index and the fractions fx, fy, fz (not clamped) of the cell of each point"""
        u = (P - self.lo) / self.h
        c = np.minimum(np.maximum(np.floor(u), 0.0), self.n - 2.0)
        f = u - c
        ci = c.astype(np.int64)
        return ci[:, 0] + self.nx * (ci[:, 1] + self.ny * ci[:, 2]), f[:, 0], f[:, 1], f[:, 2]

    def lerp(self, q, cell, grad=False):
        """the trilinear value of the component q at `cell`; grad: (value, [d/dx, d/dy, d/dz])"""
        base, fx, fy, fz = cell
        nx, nxy = self.nx, self.nx * self.ny
        v = [q[base], q[base + 1], q[base + nx], q[base + nx + 1], q[base + nxy], q[base + nxy + 1],
             q[base + nxy + nx], q[base + nxy + nx + 1]]
        d00, d10, d01, d11 = v[1] - v[0], v[3] - v[2], v[5] - v[4], v[7] - v[6]
        c00 = v[0] + fx * d00
        c10 = v[2] + fx * d10
        c01 = v[4] + fx * d01
        c11 = v[6] + fx * d11
        e0, e1 = c10 - c00, c11 - c01
        c0 = c00 + fy * e0
        c1 = c01 + fy * e1
        dz = c1 - c0
        val = c0 + fz * dz
        if not grad:
            return val
        dx0 = d00 + fy * (d10 - d00)
        dx1 = d01 + fy * (d11 - d01)
        h = self.h
        return val, [(dx0 + fz * (dx1 - dx0)) / h[0], (e0 + fz * (e1 - e0)) / h[1], dz / h[2]]

    def values(self, F, cell):
        return [self.lerp(F[c], cell) for c in range(3)]

    def inside(self, r):
        with np.errstate(invalid="ignore"):
            return np.all((r >= self.lo) & (r <= self.hi), axis=1)

    def first_face(self, ra, rn):
        """t and the face code (0: none, t = 2) of the first face the chords ra -> rn meet"""
        lo, hi = self.lo, self.hi
        t = np.full(len(ra), 2.0)
        face = np.zeros(len(ra), dtype=np.int32)
        for d in range(3):
            below, above = rn[:, d] < lo[d], rn[:, d] > hi[d]
            den = np.where(below | above, rn[:, d] - ra[:, d], 1.0)
            td = np.where(below, (lo[d] - ra[:, d]) / den, np.where(above, (hi[d] - ra[:, d]) / den, 2.0))
            fd = np.where(below, 1 + 2 * d, np.where(above, 2 + 2 * d, 0))
            take = td < t
            t = np.where(take, td, t)
            face = np.where(take, fd, face).astype(np.int32)
        return t, face

    def snap(self, rn, face):
        """rn on its face exactly along the face's axis, clamped to the box along the others (face 0: clamped only)"""
        ax = (face - 1) >> 1
        fv = np.where(((face - 1) & 1)[:, None] == 1, self.hi[None, :], self.lo[None, :])
        snapped = np.minimum(np.maximum(rn, self.lo), self.hi)
        return np.where(np.arange(3)[None, :] == ax[:, None], fv, snapped)


def trace_numpy(mesh, b, g, seeds, step, max_steps, sgn):
    """(ends, length, integral, status, nsteps) of the lines of one direction (sgn +1 or -1), vectorised over them"""
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
        if m.gf is None:
            q = np.zeros(len(P))
        else:
            gx, gy, gz = m.values(m.gf, c)
            q = (gx * ex + gy * ey) + gz * ez
        return ok, k, q

    def rk4(r, k1, q1, s):
        """stages 2-4 of a step of length s (per line); a line that met a null stays at r for the later stages"""
        hs, s6 = (0.5 * s)[:, None], s / 6.0
        ok2, k2, q2 = stage(r + hs * k1)
        ok3, k3, q3 = stage(np.where(ok2[:, None], r + hs * k2, r))
        ok = ok2 & ok3
        ok4, k4, q4 = stage(np.where(ok[:, None], r + s[:, None] * k3, r))
        ok = ok & ok4
        rn = r + s6[:, None] * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)
        dI = s6 * (((q1 + 2.0 * q2) + 2.0 * q3) + q4)
        return ok, rn, dI

    ns = len(seeds)
    r = np.array(seeds, dtype=np.float64)
    length, integral = np.zeros(ns), np.zeros(ns)
    status = np.full(ns, UNFINISHED, dtype=np.int32)
    nsteps = np.zeros(ns, dtype=np.int32)
    inside = m.inside(r)
    status[~inside] = OUTSIDE
    act = np.nonzero(inside)[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for it in range(max_steps):
            if len(act) == 0:
                break
            ra = r[act]
            ok1, k1, q1 = stage(ra)
            okr, rn, dI = rk4(ra, np.where(ok1[:, None], k1, 0.0), q1, np.full(len(act), ds))
            ok = ok1 & okr
            rn = np.where(ok[:, None], rn, ra)
            t, face = m.first_face(ra, rn)
            leave = ok & (face != 0)
            # the exit step, redone with s = t ds
            s = np.where(leave, t * ds, ds)
            ok2, rn2, dI2 = rk4(ra, np.where(ok1[:, None], k1, 0.0), q1, s)
            null = ~ok | (leave & ~ok2)
            leave = leave & ok2
            snapped = m.snap(rn2, face)
            go = ok & ~leave & ~null
            ia = act
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
    return r, length, integral, status, nsteps


def squash_numpy(mesh, b, g, seeds, step, max_steps, integrand=0):
    """(q, ends, length, integral, status, nsteps) with the shapes of QMap: q (ns), the others (2, ns[, 3]);
    vectorised over the 2 nseeds lines"""
    m = Lines(mesh, b, g, step)
    lo, hi, ds = m.lo, m.hi, m.ds

    def field(P):
        return m.values(m.bf, m.cell(P))

    def stage(P, U, V, sgn):
        """ok, the ten slopes (k of r, U, V as (n,3) arrays and of I), e = B/|B| and |B|^2 at P"""
        cell = m.cell(P)
        bv, M = [], []
        for c in range(3):
            val, gr = m.lerp(m.bf[c], cell, grad=True)
            bv.append(val)
            M.append(gr)
        m2 = (bv[0] * bv[0] + bv[1] * bv[1]) + bv[2] * bv[2]
        mag = np.sqrt(m2)
        ok = mag > 0.0
        ms = np.where(ok, mag, 1.0)
        e = [bv[c] / ms for c in range(3)]
        kr = np.stack([sgn * e[c] for c in range(3)], axis=1)
        kU = np.stack([sgn * (((M[c][0] * U[:, 0] + M[c][1] * U[:, 1]) + M[c][2] * U[:, 2]) / ms) for c in range(3)],
                      axis=1)
        kV = np.stack([sgn * (((M[c][0] * V[:, 0] + M[c][1] * V[:, 1]) + M[c][2] * V[:, 2]) / ms) for c in range(3)],
                      axis=1)
        if m.gf is None:
            q = np.zeros(len(P))
        else:
            gv = m.values(m.gf, cell)
            q = (gv[0] * e[0] + gv[1] * e[1]) + gv[2] * e[2]
            if integrand == 1:
                q = q / ms
        return ok, (kr, kU, kV, q), e, m2

    def rk4(r, U, V, sgn, k1, s):
        """stages 2-4 of a step of length s (per line) from (r, U, V) with the slopes k1; a line that met a null
        stays where it is for the later stages (its result is not used)"""
        hs, s6 = (0.5 * s)[:, None], (s / 6.0)[:, None]
        sc = s[:, None]
        ok2, k2, _e, _m = stage(r + hs * k1[0], U + hs * k1[1], V + hs * k1[2], sgn)
        acc = [k1[i] + 2.0 * k2[i] for i in range(4)]
        k2 = [np.where(ok2[:, None], k2[i], 0.0) for i in range(3)]
        ok3, k3, _e, _m = stage(r + hs * k2[0], U + hs * k2[1], V + hs * k2[2], sgn)
        acc = [acc[i] + 2.0 * k3[i] for i in range(4)]
        ok = ok2 & ok3
        k3 = [np.where(ok[:, None], k3[i], 0.0) for i in range(3)]
        ok4, k4, _e, _m = stage(r + sc * k3[0], U + sc * k3[1], V + sc * k3[2], sgn)
        acc = [acc[i] + k4[i] for i in range(4)]
        ok = ok & ok4
        return ok, r + s6 * acc[0], U + s6 * acc[1], V + s6 * acc[2], s6[:, 0] * acc[3]

    ns = len(seeds)
    nl = 2 * ns
    r = np.concatenate([np.array(seeds, dtype=np.float64)] * 2)
    sg = np.concatenate([np.full(ns, 1.0), np.full(ns, -1.0)])
    U, V = np.zeros((nl, 3)), np.zeros((nl, 3))
    length, integral = np.zeros(nl), np.zeros(nl)
    status = np.full(nl, UNFINISHED, dtype=np.int32)
    nsteps = np.zeros(nl, dtype=np.int32)
    bs2 = np.full(nl, np.nan)
    inside = m.inside(r)
    status[~inside] = OUTSIDE
    act = np.nonzero(inside)[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for it in range(max_steps):
            if len(act) == 0:
                break
            ra, sa = r[act], sg[act]
            if it == 0:
                # the frame at the seed: U0 perpendicular to e from the axis of the smallest |e_d|, V0 = e x U0
                e = np.stack(field(ra), axis=1)
                m2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
                mm = np.sqrt(m2)
                okm = mm > 0.0
                e = e / np.where(okm, mm, 1.0)[:, None]
                ae = np.abs(e)
                j = np.zeros(len(act), dtype=np.int64)
                small = ae[:, 0].copy()
                for d in (1, 2):
                    take = ae[:, d] < small
                    j = np.where(take, d, j)
                    small = np.where(take, ae[:, d], small)
                ej = e[np.arange(len(act)), j]
                w = np.stack([np.where(j == d, 1.0, 0.0) - ej * e[:, d] for d in range(3)], axis=1)
                wn = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
                u0 = w / wn[:, None]
                v0 = np.stack([e[:, 1] * u0[:, 2] - e[:, 2] * u0[:, 1], e[:, 2] * u0[:, 0] - e[:, 0] * u0[:, 2],
                               e[:, 0] * u0[:, 1] - e[:, 1] * u0[:, 0]], axis=1)
                U[act] = np.where(okm[:, None], u0, 0.0)
                V[act] = np.where(okm[:, None], v0, 0.0)
                bs2[act] = m2
            Ua, Va = U[act], V[act]
            ok1, k1, _e, _m2 = stage(ra, Ua, Va, sa)
            k1 = [np.where(ok1[:, None], k1[i], 0.0) for i in range(3)] + [k1[3]]
            okr, rn, Un, Vn, dI = rk4(ra, Ua, Va, sa, k1, np.full(len(act), ds))
            ok = ok1 & okr
            rn = np.where(ok[:, None], rn, ra)
            t, face = m.first_face(ra, rn)
            leave = ok & (face != 0)
            go = ok & ~leave
            ia = act
            r[ia[go]], U[ia[go]], V[ia[go]] = rn[go], Un[go], Vn[go]
            length[ia[go]] = length[ia[go]] + ds
            integral[ia[go]] = integral[ia[go]] + dI[go]
            nsteps[ia[go]] = it + 1
            status[ia[~ok]] = NULL
            act = ia[go]
            if not leave.any():
                continue
            # the exit step: redone with s = t ds, then two refinements of s, each a full step from the same state
            il = ia[leave]
            rl, Ul, Vl, sl = ra[leave], Ua[leave], Va[leave], sa[leave]
            kl = [k[leave] for k in k1]
            fl = face[leave]
            ax = (fl - 1) >> 1
            rows = np.arange(len(il))
            fv = np.where((fl - 1) & 1, hi[ax], lo[ax])
            s = t[leave] * ds
            okx, rx, Ux, Vx, dIx = rk4(rl, Ul, Vl, sl, kl, s)
            for _pass in range(2):
                den = rx[rows, ax] - rl[rows, ax]
                can = okx & (den != 0.0)
                s = np.where(can, s * (fv - rl[rows, ax]) / np.where(can, den, 1.0), s)
                okn, rx2, Ux2, Vx2, dIx2 = rk4(rl, Ul, Vl, sl, kl, s)
                okx = okx & okn
                rx, Ux, Vx, dIx = rx2, Ux2, Vx2, dIx2
            snapped = m.snap(rx, fl)
            done = okx
            r[il[done]], U[il[done]], V[il[done]] = snapped[done], Ux[done], Vx[done]
            length[il[done]] = length[il[done]] + s[done]
            integral[il[done]] = integral[il[done]] + dIx[done]
            nsteps[il[done]] = it + 1
            status[il[done]] = fl[done]
            status[il[~done]] = NULL
        # the two ends of each seed: deviation vectors projected onto the face along B there
        onface = (status >= 1) & (status <= 6)
        ax = np.where(onface, (status - 1) >> 1, 0)
        rows = np.arange(nl)
        be = np.stack(field(np.where(onface[:, None], r, lo[None, :])), axis=1)
        bax = be[rows, ax]
        Ut = U - (U[rows, ax] / bax)[:, None] * be
        Vt = V - (V[rows, ax] / bax)[:, None] * be
        uu = (Ut[:, 0] * Ut[:, 0] + Ut[:, 1] * Ut[:, 1]) + Ut[:, 2] * Ut[:, 2]
        vv = (Vt[:, 0] * Vt[:, 0] + Vt[:, 1] * Vt[:, 1]) + Vt[:, 2] * Vt[:, 2]
        uv = (Ut[:, 0] * Vt[:, 0] + Ut[:, 1] * Vt[:, 1]) + Ut[:, 2] * Vt[:, 2]
        bn = np.abs(bax)
        F, B = slice(0, ns), slice(ns, nl)
        num = (uu[F] * vv[B] + uu[B] * vv[F]) - 2.0 * (uv[F] * uv[B])
        q = ((num * bn[F]) * bn[B]) / bs2[F]
        good = onface[F] & onface[B] & (bn[F] > 0.0) & (bn[B] > 0.0)
        q = np.where(good, q, np.nan)
    return (q, r.reshape(2, ns, 3), length.reshape(2, ns), integral.reshape(2, ns), status.reshape(2, ns),
            nsteps.reshape(2, ns))


# ---------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------
def abc(mesh, k=np.pi, phase=0.0):
    X, Y, Z = grids(mesh)
    return np.stack([np.sin(k * Z + phase) + np.cos(k * Y), np.sin(k * X) + np.cos(k * Z + phase),
                     np.sin(k * Y) + np.cos(k * X)])


def helical(mesh, eps=1.5, b0=1.0, axis=(0.5, 0.5)):
    """B = (-eps (y - yc), eps (x - xc), b0) and a vector potential of it, A = (-b0 y / 2, b0 x / 2,
    -eps ((x - xc)^2 + (y - yc)^2) / 2); the axis (xc, yc) at the fractions `axis` of the box's x and y extent"""
    X, Y, Z = grids(mesh)
    xc, yc = axis_of(mesh, axis)
    b = np.stack([-eps * (Y - yc), eps * (X - xc), np.full(X.shape, b0)])
    a = np.stack([-0.5 * b0 * Y, 0.5 * b0 * X, -0.5 * eps * ((X - xc) ** 2 + (Y - yc) ** 2)])
    return b, a


def uniform_b(mesh, bv=(0.3, -0.2, 0.9)):
    X, _Y, _Z = grids(mesh)
    return np.stack([np.full(X.shape, v) for v in bv])


def hyperbolic(mesh, alpha, b0=1.0):
    X, Y, _Z = grids(mesh)
    xc, yc = axis_of(mesh)
    return np.stack([alpha * (X - xc), -alpha * (Y - yc), np.full(X.shape, b0)])


def sheared(mesh, alpha=0.5, beta=0.8, gamma=1.0, b0=1.0):
    """B = (alpha x' + beta y' z' + gamma y'^2, -alpha y' + beta x' z' + gamma x'^2, B0): divergence-free, no null,
    a foot-point mapping that is not linear in (x, y)"""
    X, Y, Z = grids(mesh)
    xc, yc = axis_of(mesh)
    x, y, z = X - xc, Y - yc, Z - mesh[2][0]
    return np.stack([alpha * x + beta * y * z + gamma * y * y, -alpha * y + beta * x * z + gamma * x * x,
                     np.full(X.shape, b0)])


# ---------------------------------------------------------------------------------------------------------------
# seeds
# ---------------------------------------------------------------------------------------------------------------
def face_seeds(mesh, rng, per_face):
    """random points exactly on each of the six faces"""
    lo, _h, hi, _n = box(mesh)
    out = []
    for d in range(3):
        for v in (lo[d], hi[d]):
            p = lo + (hi - lo) * rng.uniform(0.0, 1.0, (per_face, 3))
            p[:, d] = v
            out.append(p)
    return np.concatenate(out)


def inner_seeds(mesh, rng, count, margin=0.0):
    lo, _h, hi, _n = box(mesh)
    return lo + (hi - lo) * rng.uniform(margin, 1.0 - margin, (count, 3))


def patch_feet(mesh, n=6, span=(0.3, 0.7)):
    lo, _h, hi, _n = box(mesh)
    u = np.linspace(span[0], span[1], n)
    gx, gy = np.meshgrid(lo[0] + u * (hi[0] - lo[0]), lo[1] + u * (hi[1] - lo[1]), indexing="ij")
    return np.stack([gx.reshape(-1), gy.reshape(-1), np.full(n * n, lo[2])], axis=1)


def entering_feet(mesh, b):
    """the nodes of the six faces where B points into the box: seeds (m,3) and |B.n| times the trapezoid weight of
    the node in its face"""
    ws = [weights1(q) for q in mesh]
    X, Y, Z = grids(mesh)
    P = np.stack([X, Y, Z], axis=-1)                        # (nz, ny, nx, 3)
    W = [ws[2][:, None, None] * ws[1][None, :, None] * np.ones(len(mesh[0]))[None, None, :],
         ws[2][:, None, None] * np.ones(len(mesh[1]))[None, :, None] * ws[0][None, None, :],
         np.ones(len(mesh[2]))[:, None, None] * ws[1][None, :, None] * ws[0][None, None, :]]   # weight without axis d
    lo, _h, hi, _n = box(mesh)
    seeds, flux = [], []
    for d in range(3):
        for side, inward in ((0, 1.0), (-1, -1.0)):
            sl = [slice(None)] * 3
            sl[2 - d] = side
            sl = tuple(sl)
            bn = inward * b[d][sl]
            p = P[sl].reshape(-1, 3).copy()
            p = np.minimum(np.maximum(p, lo), hi)          # (a mesh's last point can exceed the library's hi by an ulp)
            p[:, d] = lo[d] if side == 0 else hi[d]
            m = bn.reshape(-1) > 0.0
            seeds.append(p[m])
            flux.append((bn * W[d][sl]).reshape(-1)[m])
    return np.concatenate(seeds), np.concatenate(flux)
