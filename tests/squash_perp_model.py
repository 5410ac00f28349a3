"""What the tests of the perpendicular squashing factor share (test_squash_perp_model.py on the CPU,
test_gpu_squash_perp.py on the device): squash_perp_numpy, the numpy restatement of ndsm_hip_vecpot_squash_perp in
include/ndsm_hip.h, which the device matches bit for bit, and the closed-form checks as functions of a
`run(mesh, b, seeds, **options)` callable with the interface of VecPot.squashing_perp - model_run here, the library
in the GPU tests - so that every check runs on the restatement without a GPU.

squash_perp_numpy restates the stepping of line_model.squash_numpy (which does not return its deviation vectors) on
the same class Lines; its q and line outputs are squash_numpy's bit for bit (test_squash_perp_model.py asserts it)."""
import numpy as np

from line_model import (FACES, NULL, UNFINISHED, OUTSIDE, Lines, axis_of, box, centre, face_seeds, grids, helical,
                        hyperbolic, inner_seeds, patch_feet, sheared, trace_numpy, uniform_b)


# ---------------------------------------------------------------------------------------------------------------
# the numpy restatement of include/ndsm_hip.h, ndsm_hip_vecpot_squash_perp
# ---------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def deviation_lines(mesh, b, g, seeds, step, max_steps, integrand=0):
    """the 2 nseeds lines of the squash entries, vectorised over them (the forward block, then the backward block):
    the Lines object, r, U, V (nl,3), length, integral, status, nsteps (nl) at the ends and |B_s|^2 (nl)"""
    m = Lines(mesh, b, g, step)
    lo, hi, ds = m.lo, m.hi, m.ds

    def stage(P, U, V, sgn):
        """ok and the ten slopes (k of r, U, V as (n,3) arrays and of I) at P"""
        cell = m.cell(P)
        bv, M = [], []
        for c in range(3):
            val, gr = m.lerp(m.bf[c], cell, grad=True)
            bv.append(val)
            M.append(gr)
        mag = np.sqrt((bv[0] * bv[0] + bv[1] * bv[1]) + bv[2] * bv[2])
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
        return ok, (kr, kU, kV, q)

    def rk4(r, U, V, sgn, k1, s):
        """stages 2-4 of a step of length s (per line) from (r, U, V) with the slopes k1; a line that met a null
        stays where it is for the later stages (its result is not used)"""
        hs, s6 = (0.5 * s)[:, None], (s / 6.0)[:, None]
        sc = s[:, None]
        ok2, k2 = stage(r + hs * k1[0], U + hs * k1[1], V + hs * k1[2], sgn)
        acc = [k1[i] + 2.0 * k2[i] for i in range(4)]
        k2 = [np.where(ok2[:, None], k2[i], 0.0) for i in range(3)]
        ok3, k3 = stage(r + hs * k2[0], U + hs * k2[1], V + hs * k2[2], sgn)
        acc = [acc[i] + 2.0 * k3[i] for i in range(4)]
        ok = ok2 & ok3
        k3 = [np.where(ok[:, None], k3[i], 0.0) for i in range(3)]
        ok4, k4 = stage(r + sc * k3[0], U + sc * k3[1], V + sc * k3[2], sgn)
        acc = [acc[i] + k4[i] for i in range(4)]
        ok = ok & ok4
        return ok, r + s6 * acc[0], U + s6 * acc[1], V + s6 * acc[2], s6[:, 0] * acc[3]

    ns = len(seeds)
    nl = 2 * ns
    r = np.concatenate([np.array(seeds, dtype=np.float64).reshape(ns, 3)] * 2)
    sg = np.concatenate([np.full(ns, 1.0), np.full(ns, -1.0)])
    U, V = np.zeros((nl, 3)), np.zeros((nl, 3))
    length, integral = np.zeros(nl), np.zeros(nl)
    status = np.full(nl, UNFINISHED, dtype=np.int32)
    nsteps = np.zeros(nl, dtype=np.int32)
    bs2 = np.full(nl, np.nan)
    inside = m.inside(r)
    status[~inside] = OUTSIDE
    act = np.nonzero(inside)[0]
    for it in range(max_steps):
        if len(act) == 0:
            break
        ra, sa = r[act], sg[act]
        if it == 0:
            # the frame at the seed: U0 perpendicular to e from the axis of the smallest |e_d|, V0 = e x U0
            e = np.stack(m.values(m.bf, m.cell(ra)), axis=1)
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
            wn = np.sqrt(_dot(w, w))
            u0 = w / wn[:, None]
            v0 = np.stack([e[:, 1] * u0[:, 2] - e[:, 2] * u0[:, 1], e[:, 2] * u0[:, 0] - e[:, 0] * u0[:, 2],
                           e[:, 0] * u0[:, 1] - e[:, 1] * u0[:, 0]], axis=1)
            U[act] = np.where(okm[:, None], u0, 0.0)
            V[act] = np.where(okm[:, None], v0, 0.0)
            bs2[act] = m2
        Ua, Va = U[act], V[act]
        ok1, k1 = stage(ra, Ua, Va, sa)
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
            okn, rx, Ux, Vx, dIx = rk4(rl, Ul, Vl, sl, kl, s)
            okx = okx & okn
        snapped = m.snap(rx, fl)
        done = okx
        r[il[done]], U[il[done]], V[il[done]] = snapped[done], Ux[done], Vx[done]
        length[il[done]] = length[il[done]] + s[done]
        integral[il[done]] = integral[il[done]] + dIx[done]
        nsteps[il[done]] = it + 1
        status[il[done]] = fl[done]
        status[il[~done]] = NULL
    return m, r, U, V, length, integral, status, nsteps, bs2


def squash_perp_numpy(mesh, b, g, seeds, step, max_steps, integrand=0):
    """(q, q_perp, ends, length, integral, status, nsteps) with the shapes of QPerpMap: q, q_perp (ns), the others
    (2, ns[, 3])"""
    ns = len(seeds)
    nl = 2 * ns
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m, r, U, V, length, integral, status, nsteps, bs2 = deviation_lines(mesh, b, g, seeds, step, max_steps,
                                                                            integrand)
        onface = (status >= 1) & (status <= 6)
        ax = np.where(onface, (status - 1) >> 1, 0)
        rows = np.arange(nl)
        be = np.stack(m.values(m.bf, m.cell(np.where(onface[:, None], r, m.lo[None, :]))), axis=1)
        F, B = slice(0, ns), slice(ns, nl)
        # Q: the deviation vectors projected onto the face along B at each end
        bax = be[rows, ax]
        Ut = U - (U[rows, ax] / bax)[:, None] * be
        Vt = V - (V[rows, ax] / bax)[:, None] * be
        uu, vv, uv = _dot(Ut, Ut), _dot(Vt, Vt), _dot(Ut, Vt)
        bn = np.abs(bax)
        num = (uu[F] * vv[B] + uu[B] * vv[F]) - 2.0 * (uv[F] * uv[B])
        q = ((num * bn[F]) * bn[B]) / bs2[F]
        q = np.where(onface[F] & onface[B] & (bn[F] > 0.0) & (bn[B] > 0.0), q, np.nan)
        # Q-perp: the same vectors projected onto the plane perpendicular to B at each end
        me = np.sqrt(_dot(be, be))
        e = be / me[:, None]
        Up = U - _dot(U, e)[:, None] * e
        Vp = V - _dot(V, e)[:, None] * e
        puu, pvv, puv = _dot(Up, Up), _dot(Vp, Vp), _dot(Up, Vp)
        num = (puu[F] * pvv[B] + puu[B] * pvv[F]) - 2.0 * (puv[F] * puv[B])
        qp = ((num * me[F]) * me[B]) / bs2[F]
        qp = np.where(onface[F] & onface[B] & (me[F] > 0.0) & (me[B] > 0.0), qp, np.nan)
    return (q, qp, r.reshape(2, ns, 3), length.reshape(2, ns), integral.reshape(2, ns), status.reshape(2, ns),
            nsteps.reshape(2, ns))


class _Map:
    def __init__(self, out, twist):
        self.q, self.q_perp, self.ends, self.length, self.integral, self.status, self.nsteps = out
        self.twist = twist


def curl_numpy(mesh, b):
    """second-order differences of b (3,nz,ny,nx), one-sided on the end planes: exact for a linear field (the
    closed-form checks with twist=True use linear fields only, so the model needs no more than that)"""
    d = [[np.gradient(b[c], mesh[a], axis=2 - a, edge_order=2) for a in range(3)] for c in range(3)]
    return np.stack([d[2][1] - d[1][2], d[0][2] - d[2][0], d[1][0] - d[0][1]])


def model_run(mesh, b, seeds, g=None, integrand=0, twist=False, step=0.5, max_steps=None, device=False):
    """the restatement behind the interface of VecPot.squashing_perp"""
    seeds = np.asarray(seeds, dtype=np.float64)
    if max_steps is None:
        max_steps = int(np.ceil(4.0 * sum(len(q) for q in mesh) / step))
    if twist:
        g, integrand = curl_numpy(mesh, b), 1
    out = squash_perp_numpy(mesh, b, g, seeds, step, max_steps, integrand)
    tw = None
    if twist:
        tw = np.where(np.isnan(out[1]), np.nan, (out[4][0] + out[4][1]) / (4.0 * np.pi))
    return _Map(out, tw)


def numpy_tracer(mesh, b, seeds, step=0.5, max_steps=None, direction="both"):
    """trace_numpy behind the interface of VecPot.trace, both directions"""
    class FL:
        pass
    assert direction == "both"
    if max_steps is None:
        max_steps = int(np.ceil(4.0 * sum(len(q) for q in mesh) / step))
    outs = [trace_numpy(mesh, b, None, seeds, step, max_steps, sgn) for sgn in (1.0, -1.0)]
    fl = FL()
    fl.ends, fl.length, fl.integral, fl.status, fl.nsteps = [np.stack([o[i] for o in outs]) for i in range(5)]
    return fl


def perp_as_q(run):
    """`run` with q_perp in the place of q: the checks of test_gpu_squash.py that read m.q then look at Q-perp"""
    def wrapped(mesh, b, seeds, **kw):
        m = run(mesh, b, seeds, **kw)
        return _Map((m.q_perp, m.q_perp, m.ends, m.length, m.integral, m.status, m.nsteps), m.twist)
    return wrapped


def rel(a, b):
    return np.abs(a - b) / np.abs(b)


def axes_of(status):
    return (status[0] - 1) >> 1, (status[1] - 1) >> 1


MIXED_PAIRS = {(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)}


# ---------------------------------------------------------------------------------------------------------------
# the closed-form checks (each takes the runner: the library on the GPU, model_run for the restatement)
# ---------------------------------------------------------------------------------------------------------------
def uniform_seeds(mesh, seed=2201):
    """scattered through the volume and on faces, and the edges and corners of the box"""
    lo, _h, hi, _n = box(mesh)
    rng = np.random.default_rng(seed)
    edge = []
    for fx in (0.0, 0.4, 1.0):
        for fy in (0.0, 0.6, 1.0):
            for fz in (0.0, 0.3, 1.0):
                if sum(f in (0.0, 1.0) for f in (fx, fy, fz)) >= 2:
                    edge.append([lo[d] if f == 0.0 else hi[d] if f == 1.0 else lo[d] + f * (hi[d] - lo[d])
                                 for d, f in enumerate((fx, fy, fz))])
    return np.concatenate([inner_seeds(mesh, rng, 300), face_seeds(mesh, rng, 8), np.array(edge)])


def check_uniform(run, mesh, seeds):
    """Q-perp = 2 whatever the pair of faces, where Q on the same seeds is |B|^2 / |B_a B_c| between faces normal to
    different axes a, c.  Returns max |Q-perp - 2| and the largest Q"""
    bv = np.array([0.3, -0.2, 0.9])
    m = run(mesh, uniform_b(mesh, bv), seeds)
    assert np.all(np.isin(m.status, list(FACES)))
    a, c = axes_of(m.status)
    pairs = set(zip(a.tolist(), c.tolist()))
    assert not np.isnan(m.q_perp).any()
    err = np.abs(m.q_perp - 2.0).max()
    want_q = np.where(a == c, 2.0, (bv * bv).sum() / np.abs(bv[a] * bv[c]))
    errq = rel(m.q, want_q).max()
    mixed = a != c
    print("uniform field: max |Q-perp - 2|", err, "max relative error of Q", errq, "Q up to", m.q.max(),
          "axis pairs (forward, backward)", sorted(pairs))
    assert err <= 1e-12
    assert errq <= 1e-12
    # both kinds of pair occur, and on the mixed ones Q is not 2: what Q-perp is for
    assert (2, 2) in pairs and pairs >= MIXED_PAIRS, pairs
    assert np.all(np.abs(m.q[mixed] - 2.0) > 0.1) and np.all(np.abs(m.q[~mixed] - 2.0) <= 1e-11)
    return err, m.q.max()


HELICAL_STEPS = (1.0, 0.5, 0.25)


def helical_seeds(mesh, seed=2202, count=48):
    return inner_seeds(mesh, np.random.default_rng(seed), count, margin=0.04)


def helix_dz(mesh, seeds, eps, b0):
    """the z extent of the helix of B = (-eps y', eps x', b0) through each seed inside the box: z(forward end) -
    z(backward end), from the closed form x' + i y' = rho exp(i (phi + eps dz / b0)) by a scan and bisection"""
    lo, _h, hi, _n = box(mesh)
    xc, yc = axis_of(mesh)
    x0, y0 = seeds[:, 0] - xc, seeds[:, 1] - yc

    def inside(dz):
        c, s = np.cos(eps * dz / b0), np.sin(eps * dz / b0)
        x, y, z = xc + (x0 * c - y0 * s), yc + (x0 * s + y0 * c), seeds[:, 2] + dz
        return (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (z >= lo[2]) & (z <= hi[2])

    out = []
    for sgn in (1.0, -1.0):
        span = hi[2] - lo[2]
        a, bb = np.zeros(len(seeds)), np.full(len(seeds), np.nan)
        for t in np.linspace(0.0, 1.0, 4001)[1:] * span * 1.001:
            ins = inside(sgn * t)
            new = np.isnan(bb) & ~ins
            bb = np.where(new, t, bb)
            a = np.where(np.isnan(bb) & ins, t, a)
        for _ in range(60):
            mid = 0.5 * (a + bb)
            ins = inside(sgn * mid)
            a, bb = np.where(ins, mid, a), np.where(ins, bb, mid)
        out.append(sgn * 0.5 * (a + bb))
    return out[0] - out[1]


def helical_errors(run, mesh, steps=HELICAL_STEPS):
    """max |Q-perp - 2| / 2 and the max relative error of T_w per step, for seeds through the volume whose lines end
    on all kinds of face pairs: the flow of B = (-eps y', eps x', b0) is a screw motion and |B| is constant along a
    line, so Q-perp = 2 on every line, and T_w = eps dz / (2 pi sqrt(b0^2 + eps^2 rho^2)) over the line's z extent"""
    eps, b0 = 1.5, 1.0
    b, _a = helical(mesh, eps, b0)
    xc, yc = axis_of(mesh)
    seeds = helical_seeds(mesh)
    rho = np.hypot(seeds[:, 0] - xc, seeds[:, 1] - yc)
    want_tw = eps * helix_dz(mesh, seeds, eps, b0) / (2.0 * np.pi * np.sqrt(b0 ** 2 + eps ** 2 * rho ** 2))
    eq, et = [], []
    for step in steps:
        m = run(mesh, b, seeds, twist=True, step=step)
        assert np.all(np.isin(m.status, list(FACES)))
        a, c = axes_of(m.status)
        pairs = set(zip(a.tolist(), c.tolist()))
        assert (2, 2) in pairs and len(pairs & MIXED_PAIRS) >= 3 and np.any((a != 2) & (c != 2)), pairs
        eq.append(rel(m.q_perp, 2.0).max())
        et.append(rel(m.twist, want_tw).max())
    return eq, et


HYPERBOLIC_STEPS = (2.0, 1.0, 0.5, 0.25)


def hyperbolic_case(mesh, alpha_lz, seed=2203, count=36):
    """(b, seeds, want Q-perp, forward and backward face) of B = (alpha x', -alpha y', b0), alpha Lz = alpha_lz: seeds
    on and off the axis at random heights.  The closed form of the docstring of hyperbolic_qperp"""
    lo, _h, hi, _n = box(mesh)
    xc, yc = axis_of(mesh)
    lz = hi[2] - lo[2]
    b0 = 1.0
    alpha = alpha_lz * b0 / lz
    rng = np.random.default_rng(seed)
    X, Y = 0.5 * (hi[0] - lo[0]), 0.5 * (hi[1] - lo[1])
    # every line of the first kind stays inside from bottom to top: |x'| e^(kappa (hi - z)) < X, |y'| e^(kappa (z -
    # lo)) < Y; the second kind is scattered through the box and reaches the x and y faces too
    z = lo[2] + lz * rng.uniform(0.05, 0.95, count)
    u, v = rng.uniform(-0.9, 0.9, count), rng.uniform(-0.9, 0.9, count)
    u[:4], v[:4] = 0.0, 0.0                                # on the axis
    u[4:7] = 0.0                                           # on the plane x' = 0, and on y' = 0
    v[7:10] = 0.0
    if alpha_lz <= 1.0:
        xs = u * X * np.exp(-alpha * (hi[2] - z) / b0)
        ys = v * Y * np.exp(-alpha * (z - lo[2]) / b0)
    else:
        xs, ys = u * X, v * Y
    seeds = np.stack([xc + xs, yc + ys, z], axis=1)
    want, ff, fb = hyperbolic_qperp(mesh, seeds, alpha, b0)
    return hyperbolic(mesh, alpha, b0), seeds, want, ff, fb


def hyperbolic_qperp(mesh, seeds, alpha, b0):
    """Q-perp of B = (alpha x', -alpha y', b0) at seeds, kappa = alpha / b0, and the faces the two ends are on.
    The line through (x', y', z) is (x' e^(kappa dz), y' e^(-kappa dz), z + dz): each end is where the first face is
    reached.  A displacement W perpendicular to B_s at the seed is moved along B_s into the seed's z-plane, W -
    (W_z / B_s,z) B_s, mapped by diag(e^(kappa dz), e^(-kappa dz), 0) to the end's z-plane, and projected
    perpendicular to the analytic B at the end (which removes the difference between that plane and the face).  With
    a, b the images of an orthonormal pair U0, V0 perpendicular to B_s, Q-perp = ((a_F.a_F)(b_B.b_B) + (a_B.a_B)
    (b_F.b_F) - 2 (a_F.b_F)(a_B.b_B)) |B_F| |B_B| / |B_s|^2, whatever the pair."""
    lo, _h, hi, _n = box(mesh)
    xc, yc = axis_of(mesh)
    kappa = alpha / b0
    x, y, z = seeds[:, 0] - xc, seeds[:, 1] - yc, seeds[:, 2]
    with np.errstate(divide="ignore"):
        # forward: |x'| grows towards the x face of its sign, or the top; backward: |y'| grows, or the bottom
        dxf = np.where(x > 0, np.log((hi[0] - xc) / np.abs(x)), np.where(x < 0, np.log((xc - lo[0]) / np.abs(x)),
                                                                         np.inf)) / kappa
        dyb = np.where(y > 0, np.log((hi[1] - yc) / np.abs(y)), np.where(y < 0, np.log((yc - lo[1]) / np.abs(y)),
                                                                         np.inf)) / kappa
    dzf = np.minimum(hi[2] - z, dxf)
    dzb = -np.minimum(z - lo[2], dyb)
    face_f = np.where(dxf < hi[2] - z, np.where(x > 0, 2, 1), 6)
    face_b = np.where(dyb < z - lo[2], np.where(y > 0, 4, 3), 5)
    bs = np.stack([alpha * x, -alpha * y, np.full(len(x), b0)], axis=1)
    es = bs / np.linalg.norm(bs, axis=1)[:, None]
    # any orthonormal pair perpendicular to B_s
    t = np.where((np.abs(es[:, 0]) < 0.9)[:, None], np.array([1.0, 0.0, 0.0])[None], np.array([0.0, 1.0, 0.0])[None])
    u0 = t - (t * es).sum(1)[:, None] * es
    u0 = u0 / np.linalg.norm(u0, axis=1)[:, None]
    v0 = np.cross(es, u0)

    def image(w, dz):
        w = w - (w[:, 2] / bs[:, 2])[:, None] * bs
        w = np.stack([w[:, 0] * np.exp(kappa * dz), w[:, 1] * np.exp(-kappa * dz), np.zeros(len(dz))], axis=1)
        be = np.stack([alpha * x * np.exp(kappa * dz), -alpha * y * np.exp(-kappa * dz), np.full(len(x), b0)], axis=1)
        me = np.linalg.norm(be, axis=1)
        ee = be / me[:, None]
        return w - (w * ee).sum(1)[:, None] * ee, me

    (af, mf), (bf, _m) = image(u0, dzf), image(v0, dzf)
    (ab, mb), (bb, _m) = image(u0, dzb), image(v0, dzb)
    num = ((af * af).sum(1) * (bb * bb).sum(1) + (ab * ab).sum(1) * (bf * bf).sum(1)
           - 2.0 * (af * bf).sum(1) * (ab * bb).sum(1))
    return num * mf * mb / (bs * bs).sum(1), face_f, face_b


def hyperbolic_errors(run, mesh, alpha_lz, steps=HYPERBOLIC_STEPS):
    """max relative error of Q-perp per step; and the model-independent facts of the case"""
    b, seeds, want, ff, fb = hyperbolic_case(mesh, alpha_lz)
    lo, _h, hi, _n = box(mesh)
    # on the axis the closed form is 2 cosh(2 alpha Lz / b0)
    assert np.all(rel(want[:4], 2.0 * np.cosh(2.0 * alpha_lz)) <= 1e-12)
    if alpha_lz <= 1.0:
        assert np.all(ff == 6) and np.all(fb == 5)
    else:
        assert np.isin(ff, (1, 2)).sum() >= 5 and np.isin(fb, (3, 4)).sum() >= 5 and (ff == 6).any() and (fb == 5).any()
    errs = []
    for step in steps:
        m = run(mesh, b, seeds, step=step)
        assert np.array_equal(m.status[0], ff) and np.array_equal(m.status[1], fb)
        errs.append(rel(m.q_perp, want).max())
    return errs, want, m


FD_DELTAS = (1e-3, 1e-4, 1e-5)


def fd_seeds(mesh):
    """a 6x6 patch at 0.45 of the height over the middle [0.3, 0.7]^2 of x and y"""
    lo, _h, hi, _n = box(mesh)
    p = patch_feet(mesh, 6, (0.3, 0.7))
    p[:, 2] = lo[2] + 0.45 * (hi[2] - lo[2])
    return p


def fd_gap(run, tracer, mesh, delta_frac, step=0.5):
    """max relative gap between Q-perp and the finite-difference Q-perp from four neighbour lines per seed, each
    traced in both directions by `tracer` (VecPot.trace's interface, direction="both"): the neighbours at +-delta U0,
    +-delta V0 in the plane perpendicular to B at the seed, the end-point differences over 2 delta projected
    perpendicular to B at the mean end point.  Seeds whose neighbours end on different faces are left out: returns
    the gap, the fraction left out, Q-perp and Q of the seeds kept"""
    b = sheared(mesh)
    seeds = fd_seeds(mesh)
    lo, _h, hi, _n = box(mesh)
    m = Lines(mesh, b, None, step)
    delta = delta_frac * (hi - lo).min()

    def field(P):
        return np.stack(m.values(m.bf, m.cell(P)), axis=1)

    bs = field(seeds)
    es = bs / np.linalg.norm(bs, axis=1)[:, None]
    t = np.array([1.0, 0.0, 0.0])[None]
    u0 = t - (t * es).sum(1)[:, None] * es
    u0 = u0 / np.linalg.norm(u0, axis=1)[:, None]
    v0 = np.cross(es, u0)
    nb = np.concatenate([seeds + delta * u0, seeds - delta * u0, seeds + delta * v0, seeds - delta * v0])
    fl = tracer(mesh, b, nb, step=step, direction="both")
    ns = len(seeds)
    st = fl.status.reshape(2, 4, ns)
    e = fl.ends.reshape(2, 4, ns, 3)
    r = run(mesh, b, seeds, step=step)
    keep = np.all(st == r.status[:, None, :], axis=(0, 1)) & np.all(np.isin(r.status, list(FACES)), axis=0)
    # the differences are those of the seeds actually used
    hu = np.linalg.norm(nb[:ns] - nb[ns:2 * ns], axis=1)[:, None]
    hv = np.linalg.norm(nb[2 * ns:3 * ns] - nb[3 * ns:], axis=1)[:, None]
    parts = []
    for d in range(2):
        be = field(e[d].mean(axis=0))
        me = np.linalg.norm(be, axis=1)
        ee = be / me[:, None]
        a, c = (e[d, 0] - e[d, 1]) / hu, (e[d, 2] - e[d, 3]) / hv
        a = a - (a * ee).sum(1)[:, None] * ee
        c = c - (c * ee).sum(1)[:, None] * ee
        parts.append(((a * a).sum(1), (c * c).sum(1), (a * c).sum(1), me))
    (auu, avv, auv, mf), (buu, bvv, buv, mb) = parts
    qfd = ((auu * bvv + buu * avv) - 2.0 * auv * buv) * mf * mb / (bs * bs).sum(1)
    return rel(r.q_perp[keep], qfd[keep]).max(), 1.0 - keep.mean(), r.q_perp[keep], r.q[keep]


def failure_case(mesh, bad):
    """(b, seeds) of test_gpu_squash.py's failure ends: a vertical field with a 2x2x2 block of nodes set to `bad`
    (0 or NaN; None: no block), seeds in its column below it, in a clean column, outside, not finite, and inside the
    block"""
    lo, h, hi, _n = box(mesh)
    X, _Y, _Z = grids(mesh)
    b = np.stack([np.zeros(X.shape), np.zeros(X.shape), np.ones(X.shape)])
    ci, cj, ck = 7, 5, 11

    def col(i, j, fz=0.25):
        return [lo[0] + (i + 0.5) * h[0], lo[1] + (j + 0.5) * h[1], lo[2] + fz * (hi[2] - lo[2])]

    c = centre(mesh)
    seeds = np.array([col(ci, cj), col(ci + 4, cj + 3), [lo[0] - 1e-9, c[1], c[2]], [c[0], c[1], np.nan],
                      col(ci, cj, 0.0)[:2] + [lo[2] + (ck + 0.5) * h[2]]])
    if bad is not None:
        b[:, ck:ck + 2, cj:cj + 2, ci:ci + 2] = bad
    return b, seeds


def check_failure_ends(run, tracer, mesh):
    """a zero cell, a NaN cell, closed lines, seeds outside and not finite: q_perp NaN with trace's status codes"""
    lo, _h, hi, _n = box(mesh)
    for bad in (0.0, np.nan):
        b, seeds = failure_case(mesh, bad)
        m = run(mesh, b, seeds)
        fl = tracer(mesh, b, seeds, direction="both")
        print("bad value", bad, "status", m.status.tolist(), "q_perp", m.q_perp.tolist())
        assert np.array_equal(m.status, fl.status)
        assert m.status[0].tolist() == [NULL, 6, OUTSIDE, OUTSIDE, NULL]
        assert m.status[1].tolist() == [5, 5, OUTSIDE, OUTSIDE, NULL]
        assert np.isnan(m.q_perp[[0, 2, 3, 4]]).all() and abs(m.q_perp[1] - 2.0) <= 1e-12
        assert np.isnan(m.q[[0, 2, 3, 4]]).all() and abs(m.q[1] - 2.0) <= 1e-12
        assert np.all(m.nsteps[:, 2:4] == 0) and np.all(m.length[:, 2:4] == 0.0)
    up, seeds = failure_case(mesh, None)
    tw = run(mesh, up, seeds, twist=True)
    assert np.isnan(tw.twist[[2, 3]]).all() and np.all(tw.twist[[0, 1, 4]] == 0.0)
    assert np.array_equal(np.isnan(tw.twist), np.isnan(tw.q_perp))
    # closed lines: every lane stops after max_steps steps
    bc, _a = helical(mesh, 1.5, 0.0)
    c = centre(mesh)
    rho = np.array([0.05, 0.15, 0.3])
    sc = np.stack([c[0] + rho, c[1] + 0.0 * rho, lo[2] + (hi[2] - lo[2]) * np.array([0.0, 0.5, 1.0])], axis=1)
    m = run(mesh, bc, sc, max_steps=40)
    fl = tracer(mesh, bc, sc, max_steps=40, direction="both")
    assert np.all(m.status == UNFINISHED) and np.all(m.nsteps == 40) and np.isnan(m.q_perp).all()
    assert np.array_equal(m.status, fl.status) and np.array_equal(m.nsteps, fl.nsteps)

