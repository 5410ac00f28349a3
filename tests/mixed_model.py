"""CPU model of the mixed-precision solve (mg_solve_mixed, fsrc/ndsmh_mg.f90; csrc/mixed.hip has the algebra).

TEST INFRASTRUCTURE - plain numpy plus the `port` oracle.  Two parts:

  vcycle_from    the reference's V-cycle composed from the oracle's own pieces (relax3d, residual3d, restrict,
                 interp and the coarsest-grid loop), started at any level - the fp64 levels >= 2 of the mixed cycle;
  mixed_cycles   the iterative refinement around it: r = rhs - L u in fp64, ONE V-cycle on L e = r from e = 0 whose
                 level 1 (sweeps, residual, the fine side of both transfers) runs in `dtype`, u += e in fp64.

The level-1 operators are written here in numpy (sweep, residual, restrict_from, prolong_add) so that they can run in
float32 the way the `T = float` kernels do: every operand is a float32 value, the weights are the fp64 weights rounded
once, every operation rounds once (numpy never contracts a * b + c, the kernels are built with -ffp-contract=off), and
the operations come in the order of smooth_fused.hip / mixed.hip / transfer.hip / restrict_stream.hip:

  sweep      s = (u[xh] + u[xl]) * wx + (u[yh] + u[yl]) * wy + (u[zh] + u[zl]) * wz - rhs ;  u = w1 * s
  residual   v = (u[xl] + u[xh]) * wx + (u[yl] + u[yh]) * wy + (u[zl] + u[zh]) * wz - rhs - u * wc ;  r = -v
  restrict   the fine residual is converted to fp64 on load, taps and weights are fp64
  prolong    e = dtype(float64(e) + P u_c): interpolation and addition in fp64, ONE rounding on the way out

With dtype = float64 the same functions are the oracle's relax3d / residual3d / restrict / interp bit for bit
(test_mixed_model.py): that is what ties their indices, colours, mirrors and bounds to the reference.

Arrays are numpy C order (nz, ny, nx); `ns` is Fortran order [nx, ny, nz]; `bcs` six letters, lower x, y, z then upper.
"""
import math

import numpy as np

from golden_inputs import BCS3, aniso_mesh, uniform_mesh

DBL_MAX = float(np.finfo(np.float64).max)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_mixed.py (kept here so that test_mixed_model.py can check their coverage without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
# update_residual_k tiles x in 128 interior columns and y in 13 rows and cuts z into chunks of >= 16 planes:
MIXED_SHAPES = (
    ([64, 32, 32], uniform_mesh),     # the smallest level the gate admits (level 2: 32 x 16 x 16); two z chunks of 16
    ([64, 33, 35], uniform_mesh),     # odd ny, nz: y tiles of 13, 13, 7 rows; chunks of 16, 16, 3 planes
    ([64, 33, 35], aniso_mesh),
    ([130, 34, 33], uniform_mesh),    # second x tile of ONE column pair; last chunk of one plane; level 2 has odd nx
    ([128, 39, 32], uniform_mesh),    # exactly one x tile, exactly three y tiles
    ([132, 40, 49], aniso_mesh),      # second x tile of two pairs; a y tile of one row; chunks of 16, 16, 16, 1
    ([258, 32, 34], uniform_mesh),    # three x tiles; level 2 is 129 x 16 x 17
)
# every face Neumann somewhere (BCS3), every face Dirichlet opposite a Neumann face somewhere (the last three)
MIXED_BCS = BCS3 + ("DDDDDD", "NDDDND", "DNNNDD", "DDDNDN")
MIXED_MS = (1, 2, 5, 6)
CASES_PER_SHAPE = 5


def mixed_cases():
    """(ns, mesh function, bcs, ms, mean, has_rhs): five per shape - four consecutive entries of MIXED_MS and one
    more (so odd and even counts), the metric alternating, the third case with a declared-zero right-hand side, the
    boundary letters walking through MIXED_BCS"""
    out = []
    for si, (ns, meshf) in enumerate(MIXED_SHAPES):
        for c in range(CASES_PER_SHAPE):
            out.append((ns, meshf, MIXED_BCS[(2 * si + c) % len(MIXED_BCS)], MIXED_MS[(si + c) % len(MIXED_MS)],
                        (si + c) % 2 == 1, c != 2))
    return out


def case_id(case):
    ns, meshf, bcs, ms, mean, has_rhs = case
    return "%s%s-%s-ms%d-%s-%s" % ("aniso-" if meshf is aniso_mesh else "", "x".join(str(n) for n in ns), bcs, ms,
                                   "mean" if mean else "max", "rhs" if has_rhs else "zero")


# ---------------------------------------------------------------------------------------------------------------------
# level-1 operators in `dtype`
# ---------------------------------------------------------------------------------------------------------------------
def _weights(mesh):
    """wx, wy, wz, wc = 2 (wx + wy + wz), w1 = 1 / wc in fp64 (ndsm_optimized.f90:79-94)"""
    w = [1.0 / ((float(q[1]) - float(q[0])) * (float(q[1]) - float(q[0]))) for q in mesh]
    wc = 2 * (w[0] + w[1] + w[2])
    return w[0], w[1], w[2], wc, 1.0 / wc


def _in_bounds(shape, bcs):
    """points the sweep and the residual update: all but the Dirichlet faces (:68-76)"""
    m = np.ones(shape, dtype=bool)
    for d, ax in ((0, 2), (1, 1), (2, 0)):
        sl = [slice(None)] * 3
        if bcs[d] == "D":
            sl[ax] = 0
            m[tuple(sl)] = False
        if bcs[3 + d] == "D":
            sl[ax] = -1
            m[tuple(sl)] = False
    return m


def _neighbour_sums(u):
    """u(xh) + u(xl), u(yh) + u(yl), u(zh) + u(zl) with the neighbours mirrored at all six faces (homogeneous
    Neumann, :109-120: index -1 reads 1, index n reads n - 2 - numpy's 'reflect')"""
    p = np.pad(u, 1, mode="reflect")
    c = slice(1, -1)
    return p[c, c, 2:] + p[c, c, :-2], p[c, 2:, c] + p[c, :-2, c], p[2:, c, c] + p[:-2, c, c]


def sweep(u, rhs, mesh, bcs, dtype=np.float64):
    """one red + black Gauss-Seidel sweep of L u = rhs (red_black_gauss_3D; rhs None: zero) in `dtype`"""
    assert set(bcs) != {"N"}, "the mixed mode never runs all-Neumann (no mean shift here)"
    u = np.array(u, dtype=dtype)
    rhs = np.zeros_like(u) if rhs is None else np.asarray(rhs, dtype=dtype)
    wx, wy, wz, _wc, w1 = (dtype(v) for v in _weights(mesh))
    k, j, i = np.ogrid[:u.shape[0], :u.shape[1], :u.shape[2]]
    colour = (i + j + k) & 1
    inb = _in_bounds(u.shape, bcs)
    first = 1 if bcs[0] == "D" else 0      # (:106: the first colour is the one of the first updated x index)
    for p in range(2):
        sx, sy, sz = _neighbour_sums(u)
        new = w1 * (sx * wx + sy * wy + sz * wz - rhs)
        u = np.where(inb & (colour == ((first + p) & 1)), new, u)
    assert u.dtype == dtype
    return u


def residual(u, rhs, mesh, bcs, dtype=np.float64):
    """r = rhs - L u inside the update bounds, 0 on the Dirichlet faces (poisson_residual_3D) in `dtype`"""
    u = np.asarray(u, dtype=dtype)
    rhs = np.zeros_like(u) if rhs is None else np.asarray(rhs, dtype=dtype)
    wx, wy, wz, wc, _w1 = (dtype(v) for v in _weights(mesh))
    sx, sy, sz = _neighbour_sums(u)
    v = sx * wx + sy * wy + sz * wz - rhs - u * wc
    r = np.where(_in_bounds(u.shape, bcs), -v, dtype(0))
    assert r.dtype == dtype
    return r


def _find_bracket(q, q0):
    """ndsm_interp.f90:373-435: 1-based (qil, qih, ierr)"""
    nq = len(q)
    if q0 <= q[0]:
        return 1, 2, -1
    if q0 >= q[nq - 1]:
        return nq - 1, nq, +1
    qil = int(math.floor((q0 - q[0]) / (q[1] - q[0]))) + 1
    if qil >= nq:
        return nq - 1, nq, 0
    return qil, qil + 1, 0


def _restrict_axis(qc, qf):
    """per coarse index: first fine tap (0-based), tap count, c2 per tap (nrestrict, ndsm_interp.f90:186-292)"""
    dq_c, dq_f = qc[1] - qc[0], qf[1] - qf[0]
    w2 = dq_f / (dq_c * dq_c)
    lo, cnt, c2 = [], [], []
    for q0 in qc:
        qil, qih, ierr = _find_bracket(qf, q0 - dq_c)
        b0 = qil if ierr < 0 else qih
        qil, qih, ierr = _find_bracket(qf, q0 + dq_c)
        b1 = qih if ierr > 0 else qil
        lo.append(b0 - 1)
        cnt.append(b1 - b0 + 1)
        c2.append([abs(dq_c - abs(qf[t] - q0)) for t in range(b0 - 1, b1)])
    mt = max(cnt)
    tab = np.zeros((len(qc), mt))
    for n, row in enumerate(c2):
        tab[n, :len(row)] = row
    return np.array(lo), np.array(cnt), tab, w2


def restrict_from(f, mesh_f, mesh_c):
    """R f onto the next coarser level (mg_restrict): the fine field - of any dtype - is converted to fp64 as it is
    read; taps in (z, y, x) order, x fastest, weight ((((c2x w2x) c2y) w2y) c2z) w2z, all in fp64"""
    f = np.asarray(f).astype(np.float64)
    (lx, cx, tx, w2x), (ly, cy, ty, w2y), (lz, cz, tz, w2z) = (_restrict_axis(np.asarray(mesh_c[d], dtype=np.float64),
                                                                              np.asarray(mesh_f[d], dtype=np.float64))
                                                               for d in range(3))
    nzf, nyf, nxf = f.shape
    out = np.zeros((len(lz), len(ly), len(lx)))
    K, J, I = np.ix_(np.arange(len(lz)), np.arange(len(ly)), np.arange(len(lx)))
    for c in range(tz.shape[1]):
        kk = np.minimum(lz + c, nzf - 1)[K]
        for b in range(ty.shape[1]):
            jj = np.minimum(ly + b, nyf - 1)[J]
            for a in range(tx.shape[1]):
                ii = np.minimum(lx + a, nxf - 1)[I]
                w = 1.0 * tx[:, a][I] * w2x
                w = w * ty[:, b][J] * w2y
                w = w * tz[:, c][K] * w2z
                have = (a < cx)[I] & (b < cy)[J] & (c < cz)[K]
                out = np.where(have, out + w * f[kk, jj, ii], out)
    return out


def _interp_axis(qf, qc):
    """per fine index: lower coarse bracket (0-based), wl, wh (ninterp, ndsm_interp.f90:85-158)"""
    lo, wl, wh = [], [], []
    for q0 in qf:
        il, ih, _ = _find_bracket(qc, q0)
        ql, qh = qc[il - 1], qc[ih - 1]
        dq = qh - ql
        lo.append(il - 1)
        wl.append(+(q0 - ql) / dq)
        wh.append(-(q0 - qh) / dq)
    return np.array(lo), np.array(wl), np.array(wh)


def interp_to(uc, mesh_f, mesh_c):
    """P u_c on the next finer level (mg_interp): fp64, last dimension first"""
    uc = np.asarray(uc, dtype=np.float64)
    (lx, wlx, whx), (ly, wly, why), (lz, wlz, whz) = (_interp_axis(np.asarray(mesh_f[d], dtype=np.float64),
                                                                   np.asarray(mesh_c[d], dtype=np.float64))
                                                      for d in range(3))
    a = whz[:, None, None] * uc[lz] + wlz[:, None, None] * uc[lz + 1]
    b = why[None, :, None] * a[:, ly, :] + wly[None, :, None] * a[:, ly + 1, :]
    return whx[None, None, :] * b[:, :, lx] + wlx[None, None, :] * b[:, :, lx + 1]


def leak_free_faces(port, ns, mesh, bcs):
    """The Dirichlet faces (axis d, side 0 / -1) that a V-cycle cannot touch.  Sweeps and residual skip a Dirichlet
    face and the coarse iterates start from zero, so only the prolongation can reach it - and it adds exactly zero
    there if, at EVERY level pair, the face's fine points take weight 1 from the coarse face and 0 from the plane
    inside.  A lower face always does (every level's mesh starts at the same number).  An upper face does not where
    the coarse mesh's last point, (n - 1) L / (n - 1) + q_0 (ndsm_multigrid_core.f90:243-263), misses the fine mesh's
    by a rounding error: then the reference itself moves that face by ~1e-17 |u_c| per cycle, and so may we."""
    _shapes, meshes = port.hierarchy(ns, mesh)
    out = []
    for d in range(3):
        for side, letter in ((0, bcs[d]), (-1, bcs[3 + d])):
            if letter != "D":
                continue
            ok = True
            for l in range(len(meshes) - 1):
                _lo, wl, wh = _interp_axis(meshes[l][d][[side]], meshes[l + 1][d])
                ok = ok and ((wl[0] == 0.0 and wh[0] == 1.0) if side == 0 else (wl[0] == 1.0 and wh[0] == 0.0))
            if ok:
                out.append((d, side))
    return out


def faces_kept(u, u0, faces):
    """do the listed faces (axis d of x, y, z; side 0 / -1) of u hold u0's bits?"""
    return all(np.array_equal(np.take(u, side, axis=2 - d), np.take(u0, side, axis=2 - d)) for d, side in faces)


def prolong_add(e, uc, mesh_f, mesh_c):
    """e + P u_c: the sum is formed in fp64 and rounded once to e's type (prolong_tile_k<TF>)"""
    return (e.astype(np.float64) + interp_to(uc, mesh_f, mesh_c)).astype(e.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the V-cycle from the oracle's pieces
# ---------------------------------------------------------------------------------------------------------------------
def vcycle_from(port, level, U, R, ns, mesh, bcs, ms=5, ex_tol=1e-13, du_max=True, nmax_exact=10000):
    """One V-cycle of the hierarchy rooted at (ns, mesh), entered at `level` (1-based) with iterate U and right-hand
    side R of that level: fine_to_coarse down to the coarsest grid, solve_exact there (the test du <= ex_tol comes
    BEFORE each sweep), coarse_to_fine back up to `level`; ms sweeps on each side.  Returns the level's new iterate."""
    shapes, meshes = port.hierarchy(ns, mesh)
    ng = len(shapes)
    u, rhs = {level: np.array(U, dtype=np.float64)}, {level: np.asarray(R, dtype=np.float64)}

    def relax(l, n):
        for _ in range(n):
            u[l] = port.relax3d(u[l], rhs[l], meshes[l - 1], bcs)

    for l in range(level, ng):                                      # fine_to_coarse
        relax(l, ms)
        rhs[l + 1] = port.restrict(port.residual3d(u[l], rhs[l], meshes[l - 1], bcs), ns, mesh, l)
        u[l + 1] = np.zeros_like(rhs[l + 1])
    sav, du = np.zeros_like(u[ng]), DBL_MAX                         # solve_exact
    for _ in range(nmax_exact):
        if du <= ex_tol:
            break
        relax(ng, 1)
        d = np.abs(sav - u[ng]).ravel()
        du = float(d.max()) if du_max else float(np.add.accumulate(d)[-1]) / d.size   # (the port's loop adds in index order)
        sav = u[ng].copy()
    for lc in range(ng, level, -1):                                 # coarse_to_fine
        relax(lc, ms)
        u[lc - 1] = u[lc - 1] + port.interp(u[lc], ns, mesh, lc - 1)
        relax(lc - 1, ms)
    return u[level]


# ---------------------------------------------------------------------------------------------------------------------
# the mixed-precision solve
# ---------------------------------------------------------------------------------------------------------------------
def mixed_cycles(port, u0, rhs, mesh, bcs, ms, ncycles, mean=False, dtype=np.float32, ex_tol=1e-13, nmax_exact=10000):
    """`ncycles` cycles of mg_solve_mixed from u0 (rhs None: zero).  Level 1 of the correction cycle - its arrays and
    its arithmetic - is `dtype`; the residual of u, the update u + e and levels >= 2 are fp64.
    Returns ([u_1 .. u_n], [du_1 .. du_n]) with du = max|e|, or sum|e| / N for the mean metric."""
    u = np.array(u0, dtype=np.float64)
    ns = list(u.shape[::-1])
    _shapes, meshes = port.hierarchy(ns, mesh)
    assert len(meshes) >= 2
    us, dus = [], []
    for _ in range(ncycles):
        r = residual(u, rhs, mesh, bcs, np.float64).astype(dtype)       # fp64 arithmetic, stored as dtype
        e = np.zeros(u.shape, dtype=dtype)
        for _s in range(ms):
            e = sweep(e, r, mesh, bcs, dtype)
        rhs2 = restrict_from(residual(e, r, mesh, bcs, dtype), meshes[0], meshes[1])
        u2 = vcycle_from(port, 2, np.zeros_like(rhs2), rhs2, ns, mesh, bcs, ms, ex_tol, not mean, nmax_exact)
        for _s in range(ms):
            u2 = port.relax3d(u2, rhs2, meshes[1], bcs)
        e = prolong_add(e, u2, meshes[0], meshes[1])
        for _s in range(ms):
            e = sweep(e, r, mesh, bcs, dtype)
        e64 = e.astype(np.float64)
        u = u + e64
        us.append(u.copy())
        dus.append(math.fsum(np.abs(e64).ravel()) / e64.size if mean else float(np.abs(e64).max()))
    return us, dus
