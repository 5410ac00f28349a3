"""What the flow tests share (test_flow_model.py on the CPU, test_gpu_flow.py on the GPU): the vectorised numpy
restatements of the semantics in include/ndsm_hip.h - flow_fit_numpy (ndsm_hip_flow_fit), green_ap_numpy
(ndsm_hip_green_ap_points / _plane) and flow_flux_numpy (ndsm_hip_flow_flux); the device matches them bit for bit, and
they take nothing from the library -, closed-form fields, and the closed-form checks as functions of a runner, so that
the same checks run with the library and with the restatement:

    fit(xs, ys, b0, b1, dt, r, rcond) -> (v (3,nsy,nsx), coef (9,nsy,nsx), status (nsy,nsx) int32)
    ap(xs, ys, bz)                    -> ap (2,nsy,nsx)
    flux(xs, ys, b, v, ap)            -> (dens (4,nsy,nsx), out (8))

Arrays are numpy C order, x fastest: the library's component planes."""
import numpy as np

EPS = np.finfo(np.float64).eps
TWO_PI = 6.283185307179586


# ---------------------------------------------------------------------------------------------------------------
# the numpy restatement of include/ndsm_hip.h
# ---------------------------------------------------------------------------------------------------------------
def ddq2(v, axis, h):
    """diffq.hpp's ddq along one axis of a plane (axis 1: x, axis 0: y), in its operand order"""
    v = np.moveaxis(v, axis, -1)
    d = np.empty_like(v)
    half = 0.5
    d[..., 1:-1] = (0.0 + v[..., :-2] * (-1 * half / h)) + v[..., 2:] * (+1 * half / h)
    d[..., 0] = ((0.0 + v[..., 0] * (-3 * half / h)) + v[..., 1] * (+4 * half / h)) + v[..., 2] * (-1 * half / h)
    d[..., -1] = ((0.0 + v[..., -1] * (+3 * half / h)) + v[..., -2] * (-4 * half / h)) + v[..., -3] * (+1 * half / h)
    return np.moveaxis(d, -1, axis)


def flow_stage(xs, ys, b0, b1, dt):
    """the seven staged planes Bx, By, Bz, T, Zx, Zy, D"""
    hx, hy = xs[1] - xs[0], ys[1] - ys[0]
    b0, b1 = np.asarray(b0, dtype=np.float64), np.asarray(b1, dtype=np.float64)
    with np.errstate(all="ignore"):
        bm = 0.5 * (b0 + b1)
        t = (b1[2] - b0[2]) / dt
        zx, zy = ddq2(bm[2], 1, hx), ddq2(bm[2], 0, hy)
        d = ddq2(bm[0], 1, hx) + ddq2(bm[1], 0, hy)
    return [bm[0], bm[1], bm[2], t, zx, zy, d]


def flow_fit_core(xs, ys, b0, b1, dt, r):
    """everything of ndsm_hip_flow_fit that does not depend on rcond, vectorised over the target pixels: p (9,nsy,nsx),
    the pixels with a value that is not finite in their window, those with every G_kk > 0, and the nine pivots"""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    hx, hy = xs[1] - xs[0], ys[1] - ys[0]
    ny, nx = len(ys), len(xs)
    st = flow_stage(xs, ys, b0, b1, dt)
    pad = [np.pad(q, r) for q in st]
    inside = np.pad(np.ones((ny, nx), dtype=bool), r)
    fin = np.ones((ny, nx), dtype=bool)
    for q in st:
        fin &= np.isfinite(q)
    bad_pix = np.pad(~fin, r)
    G = [[np.zeros((ny, nx)) for _l in range(9)] for _k in range(9)]       # (k <= l used)
    g = [np.zeros((ny, nx)) for _k in range(9)]
    bad = np.zeros((ny, nx), dtype=bool)
    with np.errstate(all="ignore"):
        for b in range(-r, r + 1):
            yp = float(b) * hy
            for a in range(-r, r + 1):
                xp = float(a) * hx
                win = (slice(r + b, r + b + ny), slice(r + a, r + a + nx))
                on = inside[win]
                if not on.any():
                    continue
                bad |= on & bad_pix[win]
                Bx, By, Bz, T, Zx, Zy, D = (q[win] for q in pad)
                s = [Zx, Zx * xp + Bz, Zx * yp, Zy, Zy * xp, Zy * yp + Bz, -D, -(D * xp) - Bx, -(D * yp) - By]
                nT = -T
                for k in range(9):
                    for l in range(k, 9):
                        G[k][l] = np.where(on, G[k][l] + s[k] * s[l], G[k][l])
                    g[k] = np.where(on, g[k] + nT * s[k], g[k])
        solved = np.ones((ny, nx), dtype=bool)
        d = []
        for k in range(9):
            solved &= G[k][k] > 0.0
            d.append(1.0 / np.sqrt(G[k][k]))
        for k in range(9):
            for l in range(k, 9):
                G[k][l] = (G[k][l] * d[k]) * d[l]
            g[k] = g[k] * d[k]
        L = [[None] * 9 for _k in range(9)]
        Dg = [None] * 9
        for k in range(9):
            w = [None] * 9
            for j in range(k):
                acc = np.zeros((ny, nx))
                for m in range(j):
                    acc = acc + w[m] * L[j][m]
                w[j] = G[j][k] - acc
                L[k][j] = w[j] / Dg[j]
            acc = np.zeros((ny, nx))
            for j in range(k):
                acc = acc + w[j] * L[k][j]
            Dg[k] = G[k][k] - acc
        y = [None] * 9
        for k in range(9):
            acc = np.zeros((ny, nx))
            for j in range(k):
                acc = acc + L[k][j] * y[j]
            y[k] = g[k] - acc
        for k in range(9):
            y[k] = y[k] / Dg[k]
        for k in range(8, -1, -1):
            acc = np.zeros((ny, nx))
            for j in range(k + 1, 9):
                acc = acc + L[j][k] * y[j]
            y[k] = y[k] - acc
        p = np.stack([y[k] * d[k] for k in range(9)])
    return p, bad, solved, np.stack(Dg)


def flow_fit_finish(core, rcond):
    """(v, coef, status) from flow_fit_core's tuple"""
    p, bad, solved, piv = core
    with np.errstate(invalid="ignore"):
        solved = solved & np.all(piv > rcond, axis=0)
    status = np.where(bad, 2, np.where(solved, 0, 1)).astype(np.int32)
    coef = np.where(status == 0, p, np.where(status == 1, 0.0, np.nan))
    return coef[[0, 3, 6]].copy(), coef, status


def flow_fit_numpy(xs, ys, b0, b1, dt, r, rcond):
    """(v, coef, status) of ndsm_hip_flow_fit"""
    return flow_fit_finish(flow_fit_core(xs, ys, b0, b1, dt, r), rcond)


fit_model = flow_fit_numpy


def slices_of(npix):
    ns = min(64, -(-npix // 4096))
    ln = -(-npix // ns)
    return [(s * ln, min(npix, (s + 1) * ln)) for s in range(ns)]


def green_ap_numpy(xs, ys, bz, pts=None):
    """ndsm_hip_green_ap_plane: ap (2,nsy,nsx) on the source's nodes; with pts (npts,2): ndsm_hip_green_ap_points,
    ap (npts,2)"""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    nx, ny = len(xs), len(ys)
    c = ((xs[1] - xs[0]) * (ys[1] - ys[0])) / TWO_PI
    q = np.asarray(bz, dtype=np.float64).reshape(-1) * c
    if pts is None:
        X, Y = np.tile(xs, ny), np.repeat(ys, nx)
    else:
        X, Y = np.asarray(pts, dtype=np.float64)[:, 0].copy(), np.asarray(pts, dtype=np.float64)[:, 1].copy()
    tot = None
    with np.errstate(all="ignore"):
        for p0, p1 in slices_of(nx * ny):
            ax, ay = np.zeros(len(X)), np.zeros(len(X))
            for p in range(p0, p1):
                dx, dy = X - xs[p % nx], Y - ys[p // nx]
                r2 = dx * dx + dy * dy
                t = q[p] / r2
                on = r2 > 0.0
                ax = np.where(on, ax + (-dy) * t, ax)
                ay = np.where(on, ay + dx * t, ay)
            tot = [ax, ay] if tot is None else [tot[0] + ax, tot[1] + ay]
    if pts is None:
        return np.stack(tot).reshape(2, ny, nx)
    return np.stack(tot, axis=1)


def ap_model(xs, ys, bz):
    return green_ap_numpy(xs, ys, bz)


def _tree(a):
    """the halving tree over the last axis of 256 lanes"""
    a = a.copy()
    o = 128
    while o > 0:
        a[..., :o] = a[..., :o] + a[..., o:2 * o]
        o //= 2
    return a[..., 0]


def reduce_rows(terms):
    """the sum of terms (nsy,nsx) in the order of descent.hpp's block_part / block_final over the rows"""
    ny, nx = terms.shape
    nb = min(ny, 2048)
    acc = np.zeros((nb, 256))
    for j in range(ny):
        for i0 in range(0, nx, 256):
            seg = terms[j, i0:i0 + 256]
            acc[j % nb, :len(seg)] = acc[j % nb, :len(seg)] + seg
    part = _tree(acc)
    v = np.zeros(256)
    for b0 in range(0, nb, 256):
        seg = part[b0:b0 + 256]
        v[:len(seg)] = v[:len(seg)] + seg
    return _tree(v)


def flow_flux_numpy(xs, ys, b, v, ap):
    """(dens (4,nsy,nsx), out (8)) of ndsm_hip_flow_flux"""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    hx, hy = xs[1] - xs[0], ys[1] - ys[0]
    nx, ny = len(xs), len(ys)
    b, v, ap = (np.asarray(q, dtype=np.float64) for q in (b, v, ap))
    with np.errstate(all="ignore"):
        hem = 2.0 * ((ap[0] * b[0] + ap[1] * b[1]) * v[2])
        hsh = -2.0 * ((ap[0] * v[0] + ap[1] * v[1]) * b[2])
        sem = (b[0] * b[0] + b[1] * b[1]) * v[2]
        ssh = -((b[0] * v[0] + b[1] * v[1]) * b[2])
        wx, wy = np.full(nx, hx), np.full(ny, hy)
        wx[[0, -1]] = 0.5 * hx
        wy[[0, -1]] = 0.5 * hy
        w = wx[None, :] * wy[:, None]
        s = [reduce_rows(w * t) for t in (hem, hsh, sem, ssh, np.abs(b[2]), b[2])]
    out = np.array([s[0], s[1], s[0] + s[1], s[2], s[3], s[2] + s[3], s[4], s[5]])
    return np.stack([hem, hsh, sem, ssh]), out


def flux_model(xs, ys, b, v, ap):
    return flow_flux_numpy(xs, ys, b, v, ap)


# ---------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------
def mesh2(n, h, lo=(0.3, -0.7)):
    """xs, ys of n = (nsx, nsy) nodes with the spacings h = (hx, hy), no origin at 0"""
    return lo[0] + np.arange(n[0]) * h[0], lo[1] + np.arange(n[1]) * h[1]


def white_noise(n, seed, ncomp=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (ncomp, n[1], n[0]))


class Poly:
    """a random polynomial of total degree <= deg in the centred, scaled coordinates X, Y of a mesh, with the closed
    form of its centred difference quotients on that mesh: f' + h^2 f''' / 6, exactly"""

    def __init__(self, rng, deg):
        self.c = {(p, q): rng.uniform(-1.0, 1.0) for p in range(deg + 1) for q in range(deg + 1 - p)}

    @staticmethod
    def _pow(X, p):
        return np.ones_like(X) if p == 0 else X ** p

    def __call__(self, X, Y):
        return sum(c * self._pow(X, p) * self._pow(Y, q) for (p, q), c in self.c.items())

    def dx(self, X, Y, h):
        """the centred quotient along X with spacing h (in units of X)"""
        out = np.zeros_like(X)
        for (p, q), c in self.c.items():
            if p >= 1:
                out = out + c * p * self._pow(X, p - 1) * self._pow(Y, q)
            if p == 3:
                out = out + c * h * h * self._pow(Y, q)
        return out

    def dy(self, X, Y, h):
        out = np.zeros_like(X)
        for (p, q), c in self.c.items():
            if q >= 1:
                out = out + c * q * self._pow(X, p) * self._pow(Y, q - 1)
            if q == 3:
                out = out + c * h * h * self._pow(X, p)
        return out


def affine_case(n, h, deg, seed, dt=0.37):
    """(xs, ys, b0, b1, dt, vtrue (3,nsy,nsx)): Bm with each component a random polynomial of degree deg, a global
    affine flow V = V0 + M (x - x_c), and T from the closed form of the discrete quotients, so that the affine model
    has no residual wherever the quotients are centred"""
    rng = np.random.default_rng(seed)
    xs, ys = mesh2(n, h)
    xc, yc = 0.5 * (xs[0] + xs[-1]), 0.5 * (ys[0] + ys[-1])
    sx, sy = 0.5 * (xs[-1] - xs[0]), 0.5 * (ys[-1] - ys[0])
    X, Y = np.meshgrid((xs - xc) / sx, (ys - yc) / sy)           # the polynomials live on [-1, 1]^2
    f = [Poly(rng, deg) for _c in range(3)]
    bm = np.stack([p(X, Y) for p in f])
    zx, zy = f[2].dx(X, Y, h[0] / sx) / sx, f[2].dy(X, Y, h[1] / sy) / sy
    d = f[0].dx(X, Y, h[0] / sx) / sx + f[1].dy(X, Y, h[1] / sy) / sy
    v0, m = rng.uniform(-1.0, 1.0, 3), rng.uniform(-1.0, 1.0, (3, 2)) / np.array([sx, sy])
    px, py = np.meshgrid(xs - xc, ys - yc)
    u, v, w = (v0[c] + m[c, 0] * px + m[c, 1] * py for c in range(3))
    t = -(zx * u + bm[2] * m[0, 0] + zy * v + bm[2] * m[1, 1]) + (w * d + m[2, 0] * bm[0] + m[2, 1] * bm[1])
    b0, b1 = bm.copy(), bm.copy()
    b0[2] = bm[2] - (0.5 * dt) * t
    b1[2] = bm[2] + (0.5 * dt) * t
    return xs, ys, b0, b1, dt, np.stack([u, v, w])


def interior(n, r):
    """the pixels whose window stays at least one row from the edge"""
    m = np.zeros((n[1], n[0]), dtype=bool)
    m[r + 1:n[1] - r - 1, r + 1:n[0] - r - 1] = True
    return m


# ---------------------------------------------------------------------------------------------------------------
# the closed-form checks, as functions of a runner
# ---------------------------------------------------------------------------------------------------------------
RECOVERY = [((20, 18), (0.1, 0.13), 2), ((20, 18), (0.1, 0.13), 3), ((24, 22), (1.0, 0.7), 5)]
# max |V - V_affine| over the interior pixels as flow_fit_numpy gives it on the CPU for the three cases above (values of
# order 1, smallest scaled pivots 4.2e-6, 3.9e-5 and 3.6e-4; test_flow_model.py prints them) by r.  The tolerance is ten
# times that, for a rounding that is different and equally valid - the device has none: it gives the restatement's bits
RECOVERY_SEEN = {2: 3.2e-8, 3: 1.7e-9, 5: 3.3e-10}


def recovery_tol(r):
    return 10.0 * RECOVERY_SEEN[r]


def check_recovery(fit, n, h, r, tol):
    xs, ys, b0, b1, dt, vtrue = affine_case(n, h, 3, seed=11)
    v, coef, status = fit(xs, ys, b0, b1, dt, r, 1e-10)
    m = interior(n, r)
    assert m.sum() >= 4
    assert np.all(status[m] == 0), "%d of %d interior pixels not solved" % ((status[m] != 0).sum(), m.sum())
    err = float(np.abs(v - vtrue)[:, m].max())
    print("recovery n", n, "h", h, "r", r, "max error %.3e (tolerance %.3e)" % (err, tol))
    assert err <= tol, (err, tol)
    assert np.array_equal(coef[[0, 3, 6]], v)
    return err


def check_rank_deficient(fit):
    """status 1 with zeros: quadratic components (nine columns in the 6-dimensional space of quadratics), cubic
    components with r = 1 (on 3 x 3 pixels x'^3 = h^2 x': the polynomials of degree <= 3 span 8 dimensions), and a
    zero field"""
    for n, h, deg, r in (((20, 18), (0.1, 0.13), 2, 2), ((20, 18), (0.1, 0.13), 2, 3), ((24, 22), (1.0, 0.7), 2, 5),
                         ((20, 18), (0.1, 0.13), 3, 1), ((24, 22), (1.0, 0.7), 3, 1)):
        xs, ys, b0, b1, dt, _vtrue = affine_case(n, h, deg, seed=11)
        v, coef, status = fit(xs, ys, b0, b1, dt, r, 1e-10)
        m = interior(n, r)
        assert np.all(status[m] == 1), (n, deg, r, np.unique(status[m], return_counts=True))
        assert not v[:, status == 1].any() and not coef[:, status == 1].any()
    xs, ys = mesh2((9, 7), (0.5, 0.25))
    z = np.zeros((3, 7, 9))
    v, coef, status = fit(xs, ys, z, z, 1.0, 2, 0.0)
    assert np.all(status == 1) and not v.any() and not coef.any()


def check_zero_pivot(fit):
    """a pivot that is exactly 0 is not > rcond = 0.  On a mesh of whole numbers with B_z = x + y + 3 and B_x = x the
    columns Zx and Zy are both 1 everywhere (the one-sided rows are exact on whole numbers); with r = 1 a corner's
    window holds 4 pixels, so G_00 = G_03 = G_33 = 4 and d_0 = d_3 = 0.5 exactly, scaling by them commutes with every
    rounding, column 3 repeats column 0 bit for bit, and D_3 = 1 - 1 1 = 0 with every other G_kk > 0: status 1"""
    xs, ys = np.arange(6.0), np.arange(5.0)
    X, Y = np.meshgrid(xs, ys)
    b = np.stack([X, np.zeros_like(X), X + Y + 3.0])
    v, coef, status = fit(xs, ys, b, b, 1.0, 1, 0.0)
    for j, i in ((0, 0), (0, 5), (4, 0), (4, 5)):
        assert status[j, i] == 1 and not v[:, j, i].any() and not coef[:, j, i].any(), (i, j, status[j, i])


def check_pivot_rule(fit):
    """a pivot equal to rcond is not > rcond.  The cubic case of check_recovery with r = 3; at the interior pixels whose
    smallest pivot is the last one, D_8 (nothing is computed from it but the solution), rcond is set to the
    restatement's own D_8 - the bits the device has too: status 1 with zeros there; and with the next double below it,
    status 0 and the clean run's solution"""
    n, h, r = RECOVERY[1]
    xs, ys, b0, b1, dt, _vtrue = affine_case(n, h, 3, seed=11)
    core = flow_fit_core(xs, ys, b0, b1, dt, r)
    piv = core[3]
    last = interior(n, r) & (piv.argmin(axis=0) == 8)
    assert last.sum() >= 3
    clean = fit(xs, ys, b0, b1, dt, r, 1e-10)
    for j, i in list(zip(*np.nonzero(last)))[:3]:
        d8 = float(piv[8, j, i])
        assert 1e-10 < d8 < 1.0
        v, coef, status = fit(xs, ys, b0, b1, dt, r, d8)
        assert status[j, i] == 1 and not v[:, j, i].any() and not coef[:, j, i].any(), (i, j, status[j, i])
        v, coef, status = fit(xs, ys, b0, b1, dt, r, float(np.nextafter(d8, 0.0)))
        assert status[j, i] == 0 and np.array_equal(coef[:, j, i], clean[1][:, j, i]), (i, j, status[j, i])


def check_clipping(fit):
    """windows are clipped, not padded and not clamped: once r reaches across the magnetogram from every pixel each
    window is the whole magnetogram, and a larger r changes no bit"""
    for n, r in (((3, 3), 2), ((5, 4), 4)):
        xs, ys = mesh2(n, (0.5, 0.25))
        b0, b1 = white_noise(n, 1), white_noise(n, 2)
        a = fit(xs, ys, b0, b1, -0.5, r, 0.0)
        for big in (r + 1, 16):
            for g, w in zip(fit(xs, ys, b0, b1, -0.5, big, 0.0), a):
                assert np.array_equal(g, w, equal_nan=True), (n, r, big)


def reach(n, at, comp, r):
    """the pixels that ndsm_hip_flow_fit answers with status 2 when component comp of the pixel at = (i, j) is not
    finite: those whose clipped window holds a pixel whose staged quantities read it.  Bm and (z) T at the pixel itself;
    the quotient along x (z: Zx; x: D) where its stencil holds the pixel, likewise along y (z: Zy; y: D)"""
    nx, ny = n
    i, j = at
    staged = np.zeros((ny, nx), dtype=bool)
    staged[j, i] = True

    def stencil(q, m):
        return [0, 1, 2] if q == 0 else ([m - 1, m - 2, m - 3] if q == m - 1 else [q - 1, q + 1])
    if comp in (0, 2):
        for q in range(nx):
            if i in stencil(q, nx):
                staged[j, q] = True
    if comp in (1, 2):
        for q in range(ny):
            if j in stencil(q, ny):
                staged[q, i] = True
    out = np.zeros_like(staged)
    for jj, ii in zip(*np.nonzero(staged)):
        out[max(jj - r, 0):jj + r + 1, max(ii - r, 0):ii + r + 1] = True
    return out


def check_bad_values(fit):
    n, h, r = (20, 18), (0.1, 0.13), 2
    xs, ys, b0, b1, dt, _vtrue = affine_case(n, h, 3, seed=11)
    clean = fit(xs, ys, b0, b1, dt, r, 1e-10)
    for value in (np.nan, np.inf, -np.inf):
        for comp, at in ((2, (9, 8)), (0, (9, 8)), (1, (3, 0)), (2, (0, 17)), (2, (19, 1)), (0, (1, 5))):
            bad = b1.copy()
            bad[comp, at[1], at[0]] = value
            v, coef, status = fit(xs, ys, b0, bad, dt, r, 1e-10)
            want = reach(n, at, comp, r)
            assert np.array_equal(status == 2, want), (value, comp, at)
            assert np.all(np.isnan(v[:, want])) and np.all(np.isnan(coef[:, want]))
            for g, c in zip((v, coef, status), clean):
                assert np.array_equal(g[..., ~want], c[..., ~want]), (value, comp, at)


def check_single_pixel(ap):
    """one non-zero pixel: Ap = c bz (-dy, dx) / r2 at every node, to the last bit of that expression, 0 at the pixel"""
    for n, h, at in (((9, 7), (0.5, 0.25), (4, 2)), ((70, 63), (0.1, 0.13), (69, 62)), ((70, 63), (0.1, 0.13), (0, 0))):
        xs, ys = mesh2(n, h)
        bz = np.zeros((n[1], n[0]))
        bz[at[1], at[0]] = -1.75
        got = ap(xs, ys, bz)
        c = ((xs[1] - xs[0]) * (ys[1] - ys[0])) / TWO_PI
        X, Y = np.meshgrid(xs, ys)
        dx, dy = X - xs[at[0]], Y - ys[at[1]]
        r2 = dx * dx + dy * dy
        with np.errstate(all="ignore"):
            t = (bz[at[1], at[0]] * c) / r2
            want = np.stack([(-dy) * t, dx * t])
        want[:, at[1], at[0]] = 0.0
        assert np.array_equal(got, want), (n, at)


# the Gaussian B_z = exp(-rho^2 / sigma^2), sigma = 1, on [-4, 4]^2 against A_phi = sigma^2 (1 - exp(-rho^2 / sigma^2)) /
# (2 rho): the max error over the nodes seen on the CPU, 4.3e-3 at h = 0.25 and 2.8e-3 at h = 0.2 on values up to 0.32
GAUSS_SEEN = {0.25: 4.3e-3, 0.2: 2.8e-3}


def gaussian_error(ap, h):
    n = int(round(8.0 / h)) + 1
    xs = ys = -4.0 + h * np.arange(n)
    X, Y = np.meshgrid(xs, ys)
    rho2 = X * X + Y * Y
    got = ap(xs, ys, np.exp(-rho2))
    with np.errstate(all="ignore"):
        f = np.where(rho2 > 0.0, (1.0 - np.exp(-rho2)) / (2.0 * rho2), 0.5)       # A_phi / rho
    want = np.stack([-Y * f, X * f])
    return float(np.abs(got - want).max()), float(np.abs(want).max())


def check_gaussian(ap):
    err = {h: gaussian_error(ap, h) for h in (0.25, 0.2)}
    ratio = err[0.25][0] / err[0.2][0]
    print("gaussian: max error %.3e at h = 0.25, %.3e at h = 0.2 (values up to %.3f), ratio %.3f"
          % (err[0.25][0], err[0.2][0], err[0.25][1], ratio))
    assert abs(ratio - 1.55) <= 0.15, ratio
    for h, seen in GAUSS_SEEN.items():
        assert err[h][0] < 1.5 * seen, (h, err[h][0])


def check_aligned_flow(flux):
    """adding lambda(x, y) B to V changes neither h_em + h_sh nor s_em + s_sh at any pixel: a field-aligned flow
    carries no flux.  Bound: 16 eps of the sum of the magnitudes of the terms of the two sums compared"""
    for n, h in (((9, 7), (0.5, 0.25)), ((70, 63), (0.1, 0.13))):
        xs, ys = mesh2(n, h)
        b, v, a = white_noise(n, 21), white_noise(n, 22), white_noise(n, 23, 2)
        lam = white_noise(n, 24, 1)[0] * 3.0
        v2 = v + lam * b

        def mags(vv):
            mh = 2.0 * (np.abs(a[0] * b[0] * vv[2]) + np.abs(a[1] * b[1] * vv[2]) + np.abs(a[0] * vv[0] * b[2]) +
                        np.abs(a[1] * vv[1] * b[2]))
            ms = (np.abs(b[0] * b[0] * vv[2]) + np.abs(b[1] * b[1] * vv[2]) + np.abs(b[0] * vv[0] * b[2]) +
                  np.abs(b[1] * vv[1] * b[2]))
            return mh, ms
        d1, _o1 = flux(xs, ys, b, v, a)
        d2, _o2 = flux(xs, ys, b, v2, a)
        (mh1, ms1), (mh2, ms2) = mags(v), mags(v2)
        eh = np.abs((d1[0] + d1[1]) - (d2[0] + d2[1]))
        es = np.abs((d1[2] + d1[3]) - (d2[2] + d2[3]))
        print("aligned flow", n, "worst error / bound: helicity %.3f, energy %.3f"
              % ((eh / (16 * EPS * (mh1 + mh2))).max(), (es / (16 * EPS * (ms1 + ms2))).max()))
        assert np.all(eh <= 16 * EPS * (mh1 + mh2)) and np.all(es <= 16 * EPS * (ms1 + ms2))


def check_uniform_totals(flux):
    """uniform B, V and Ap: every total is its density times the area - the trapezoid weights sum to the area.  Bound:
    npix roundings of a sum of terms of one sign, and the weights' own"""
    for n, h in (((9, 7), (0.5, 0.25)), ((70, 63), (0.1, 0.13)), ((3, 2), (1.0, 2.0))):
        xs, ys = mesh2(n, h)
        bc, vc, ac = np.array([0.7, -1.1, 0.4]), np.array([0.3, 0.9, -0.6]), np.array([-0.8, 0.5])
        one = np.ones((n[1], n[0]))
        dens, out = flux(xs, ys, bc[:, None, None] * one, vc[:, None, None] * one, ac[:, None, None] * one)
        area = (xs[-1] - xs[0]) * (ys[-1] - ys[0])
        hem = 2.0 * (ac[0] * bc[0] + ac[1] * bc[1]) * vc[2]
        hsh = -2.0 * (ac[0] * vc[0] + ac[1] * vc[1]) * bc[2]
        sem = (bc[0] ** 2 + bc[1] ** 2) * vc[2]
        ssh = -(bc[0] * vc[0] + bc[1] * vc[1]) * bc[2]
        want = np.array([hem, hsh, hem + hsh, sem, ssh, sem + ssh, abs(bc[2]), bc[2]]) * area
        tol = 2.0 * (n[0] * n[1] + 8) * EPS
        scale = np.array([abs(hem), abs(hsh), abs(hem) + abs(hsh), abs(sem), abs(ssh), abs(sem) + abs(ssh), abs(bc[2]),
                          abs(bc[2])]) * area
        assert np.all(np.abs(out - want) <= tol * scale), (n, out, want)
        for q, val in enumerate((hem, hsh, sem, ssh)):
            assert np.all(np.abs(dens[q] - val) <= 8 * EPS * abs(val))
