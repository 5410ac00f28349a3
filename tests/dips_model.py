"""What the dip tests share (test_dips_model.py on the CPU, test_gpu_dips.py on the GPU): dips_numpy, the vectorised
numpy restatement of the semantics of ndsm_hip_vecpot_dips in include/ndsm_hip.h (the nodal gradient, the crossing
rule, the interpolation, the record; the device matches it bit for bit - it takes nothing from the library),
closed-form fields with known dips, and the closed-form checks as functions of a runner
`run(mesh, b, plane_only=False) -> Dips`, so that the same checks run with the library (VecPot.dips) and with the
restatement behind the same Python layer (model_run)."""
import numpy as np

from line_model import abc, box, grids
from nlfff_model import ddq
from null_model import smooth_noise

NAMES = ("counts", "edge", "pos", "bpt", "grad", "curv", "flag")


# ---------------------------------------------------------------------------------------------------------------
# the numpy restatement of include/ndsm_hip.h
# ---------------------------------------------------------------------------------------------------------------
def dips_numpy(mesh, b, plane_only=False, max_dips=None):
    """(counts, edge, pos, bpt, grad, curv, flag) of ndsm_hip_vecpot_dips: counts = [crossings, dips, bald patches],
    the records in ascending edge (max_dips given: the first max_dips of them)"""
    b = np.asarray(b, dtype=np.float64)
    nz, ny, nx = b.shape[1:]
    lo, h, _hi, _n = box(mesh)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = [b[0], b[1], b[2]] + [ddq(b[2], d, h[d]) for d in range(3)]       # B_x, B_y, B_z, G_x, G_y, G_z
        rec = {name: [] for name in NAMES[1:]}
        ncross = 0
        for d in range(2 if plane_only else 3):
            lower = [slice(None)] * 3
            upper = [slice(None)] * 3
            lower[2 - d], upper[2 - d] = slice(None, -1), slice(1, None)
            if plane_only:
                lower[0] = upper[0] = slice(0, 1)
            lower, upper = tuple(lower), tuple(upper)
            a, bb = b[2][lower], b[2][upper]
            k, j, i = np.nonzero((a > 0.0) != (bb > 0.0))
            ncross += len(k)
            a, bb = a[k, j, i], bb[k, j, i]
            t = a / (a - bb)
            qt = []
            for v in q:
                v0, v1 = v[lower][k, j, i], v[upper][k, j, i]
                qt.append(v0 + t * (v1 - v0))
            idx = [i, j, k]
            pos = [lo[m] + idx[m].astype(np.float64) * h[m] for m in range(3)]
            pos[d] = lo[d] + (idx[d].astype(np.float64) + t) * h[d]
            curv = qt[0] * qt[3] + qt[1] * qt[4]
            dip = curv > 0.0
            rec["edge"].append((3 * (i + nx * (j + ny * k)) + d)[dip].astype(np.int64))
            rec["pos"].append(np.stack(pos, axis=1)[dip])
            rec["bpt"].append(np.stack(qt[:3], axis=1)[dip])
            rec["grad"].append(np.stack(qt[3:], axis=1)[dip])
            rec["curv"].append(curv[dip])
            rec["flag"].append(((k == 0) & (d != 2)).astype(np.int32)[dip])
    out = {name: np.concatenate(v) for name, v in rec.items()}
    order = np.argsort(out["edge"], kind="stable")
    counts = np.array([ncross, len(order), int(out["flag"].sum())], dtype=np.int64)
    if max_dips is not None:
        order = order[:max_dips]
    return (counts,) + tuple(out[name][order] for name in NAMES[1:])


def model_run(mesh, b, plane_only=False, max_dips=None, device=False):
    """the restatement behind the interface of VecPot.dips (the library's own Python layer forms the tuple)"""
    from ndsm_amd import _lib
    out = dips_numpy(mesh, b, plane_only, max_dips)
    if max_dips is not None and out[0][1] > max_dips > 0:
        out = dips_numpy(mesh, b, plane_only)
    return _lib._dips_tuple(list(out[1:]), out[0], len(mesh[0]), len(mesh[1]))


def same_records(a, b):
    """two record tuples of dips_numpy's layout agree bit for bit (NaN == NaN)"""
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=x.dtype.kind == "f") and x.dtype == y.dtype and
               x.shape == y.shape for x, y in zip(a, b))


def bald_subset(full):
    """the records of a full call that carry flag bit 0, as the plane_only call reports them (counts[0] is the
    plane's own and is not derived here: None)"""
    keep = (full[6] & 1) == 1
    return (None,) + tuple(a[keep] for a in full[1:])


# ---------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------
def inside(mesh, d, index, frac=0.37):
    """a coordinate strictly inside the edge (index, index + 1) of axis d"""
    return mesh[d][index] + frac * (mesh[d][index + 1] - mesh[d][index])


def rope(mesh, q, be, ba, xc, zc, along="y"):
    """a flux rope about an axis along y through (xc, zc): B = (be - q (z - zc), ba, q (x - xc)); along="x": the same
    about an axis along x through (y = xc, zc): B = (ba, be - q (z - zc), q (y - xc))"""
    X, Y, Z = grids(mesh)
    if along == "y":
        return np.stack([be - q * (Z - zc), np.full(X.shape, ba), q * (X - xc)])
    return np.stack([np.full(X.shape, ba), be - q * (Z - zc), q * (Y - xc)])


def tilted(mesh, b0, s, r, x0, z1, c=0.0):
    """B = (b0, 0, s (x - x0) + r (z - z1) + c (z - z1)^2): a zero surface of B_z that crosses x and z edges"""
    X, _Y, Z = grids(mesh)
    return np.stack([np.full(X.shape, b0), np.zeros(X.shape), s * (X - x0) + r * (Z - z1) + c * (Z - z1) ** 2])


def bitwise_fields(mesh):
    """(name, field) for the bitwise tests next to the closed forms: the ABC field plus smooth noise; the same with a
    zero and a NaN block; and with a small block of Inf in b_z alone - the lone Inf that the header says can pass"""
    b = abc(mesh, k=2.0 * np.pi) + smooth_noise(mesh, 11, 0.3)
    yield "abc+noise", b
    c = b.copy()
    c[:, 3:8, 4:9, 5:10] = 0.0
    c[:, 11:15, 10:14, 12:16] = np.nan
    yield "abc+noise, zero and NaN blocks", c
    c = c.copy()
    c[2, 16:18, 2:5, 3:6] = np.inf
    yield "abc+noise, zero and NaN blocks, Inf in b_z", c


def white_noise(shape, seed=3):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (3, shape[2], shape[1], shape[0]))


# ---------------------------------------------------------------------------------------------------------------
# the closed-form checks (each takes the runner)
# ---------------------------------------------------------------------------------------------------------------
def _ascending(got):
    assert np.all(np.diff(got.edge) > 0)
    assert got.ndips == len(got.edge) and got.nbald == int(got.bald.sum())


def grad_tol(b, h):
    """a bound on the rounding error of a nodal gradient of b_z and of its interpolation along an edge: the
    difference quotient adds at most three products of magnitude <= 2 |b_z| / h, each with a relative error of one
    eps, and the interpolation a few eps more: 16 eps max|b_z| / min(h)"""
    return 16.0 * np.finfo(np.float64).eps * np.abs(b[2]).max() / h.min()


def check_rope(run, mesh, along="y"):
    """closed form (a) / (b): dips exactly on the edges (family 0 for a rope along y, 1 along x) that contain xc, on the
    planes z_k < zc + be / q; ny (nx) bald patches when k = 0 qualifies; pos, curv, kappa in closed form; no record
    for a rope that is concave down; none on a plane where curv is exactly 0 (the strict rule)"""
    lo, h, hi, n = box(mesh)
    nx, ny, nz = (int(v) for v in n)
    fam = 0 if along == "y" else 1                  # the axis the crossed edges run along
    free = 1 - fam                                  # the axis along the rope
    ic = 4
    xc = inside(mesh, fam, ic)
    kc = nz // 2
    zc = inside(mesh, 2, kc, 0.41)
    q, be, ba = 1.3, 0.225 * (hi[2] - lo[2]), 0.7           # zc + be / q: a height inside the box, above zc
    zt = zc + be / q
    ks = np.nonzero(mesh[2] < zt)[0]
    assert 0 < len(ks) < nz and abs(mesh[2] - zt).min() > 1e-6 * h[2]
    b = rope(mesh, q, be, ba, xc, zc, along)
    got = run(mesh, b)
    nfree = int(n[free])
    print("rope along", along, "crossings", got.ncrossings, "dips", got.ndips, "bald", got.nbald, "planes", len(ks))
    _ascending(got)
    assert got.ncrossings == nfree * nz and got.ndips == nfree * len(ks) and got.nbald == nfree
    assert np.all(got.axis == fam) and np.all(got.node[:, fam] == ic)
    assert sorted(set(got.node[:, 2].tolist())) == ks.tolist()
    assert np.array_equal(got.bald, got.node[:, 2] == 0)
    ext = (hi - lo).max()
    assert np.abs(got.position[:, fam] - xc).max() <= 1e-12 * ext
    for m in (free, 2):                             # the other two axes: the node's own coordinates
        assert np.abs(got.position[:, m] - mesh[m][got.node[:, m]]).max() <= 1e-12 * ext
    zk = mesh[2][got.node[:, 2]]
    bt = be - q * (zk - zc)                         # the transverse component at the crossing
    curv = q * bt
    assert np.abs(got.curv - curv).max() <= 1e-12 * np.abs(curv).max()
    kappa = curv / (bt * bt + ba * ba)
    assert np.abs(got.kappa - kappa).max() <= 1e-12 * np.abs(kappa).max()
    want_b = np.zeros((len(zk), 3))
    want_b[:, fam], want_b[:, free] = bt, ba
    assert np.abs(got.b - want_b).max() <= 1e-12 * max(abs(be) + q * (hi[2] - lo[2]), abs(ba))
    want_g = np.zeros(3)
    want_g[fam] = q
    assert np.abs(got.grad - want_g).max() <= grad_tol(b, h)
    # concave down: the same crossings, no dip
    down = run(mesh, rope(mesh, -q, be, ba, xc, mesh[2][0] - 0.5 * (hi[2] - lo[2]), along))
    assert down.ncrossings == nfree * nz and down.ndips == 0 and down.nbald == 0 and len(down.edge) == 0
    assert down.position.shape == (0, 3) and down.kappa.shape == (0,)
    # curv exactly 0 on the node plane k = kc (be = 0, zc a mesh coordinate; ba = 0, so that the rounding residue of
    # the one-sided difference quotient along the rope is multiplied by 0): the strict rule leaves it out
    flat = run(mesh, rope(mesh, q, 0.0, 0.0, xc, mesh[2][kc], along))
    assert flat.ncrossings == nfree * nz and flat.ndips == nfree * kc and flat.nbald == nfree
    assert sorted(set(flat.node[:, 2].tolist())) == list(range(kc))
    return got


def check_tilted(run, mesh):
    """closed form (c): B_z = s (x - x0) + r (z - z1) crosses x and z edges; the crossed edges follow from the sign of
    the nodal values, pos on each is in closed form, curv = b0 s.  With b0 = 0 curv is exactly 0 - the z term is left
    out, not rounded in - and the strict rule reports nothing.  With a term c (z - z1)^2 B_z is still linear along x,
    and grad_z on the x edges is r + 2 c (z_k - z1) on every plane, the end planes included: the 3-point one-sided
    rows of the difference quotient are exact for it, first-order rows are not"""
    lo, h, hi, n = box(mesh)
    nx, ny, nz = (int(v) for v in n)
    ext = (hi - lo).max()
    x0, z1 = inside(mesh, 0, nx // 2, 0.23), inside(mesh, 2, nz // 2, 0.57)
    b0, s = 0.8, 1.7
    r = 0.6 * s * (hi[0] - lo[0]) / (hi[2] - lo[2])
    b = tilted(mesh, b0, s, r, x0, z1)
    pos_z = b[2] > 0.0
    cx = pos_z[:, :, :-1] != pos_z[:, :, 1:]
    cz = pos_z[:-1] != pos_z[1:]
    assert cx.sum() > ny and cz.sum() > ny and not (pos_z[:, :-1] != pos_z[:, 1:]).any()
    got = run(mesh, b)
    print("tilted: crossings", got.ncrossings, "x", int(cx.sum()), "z", int(cz.sum()), "dips", got.ndips)
    _ascending(got)
    assert got.ncrossings == got.ndips == int(cx.sum() + cz.sum())
    want = []
    for d, c in ((0, cx), (2, cz)):
        k, j, i = np.nonzero(c)
        want.append(3 * (i + nx * (j + ny * k)) + d)
    assert np.array_equal(got.edge, np.sort(np.concatenate(want)))
    assert got.nbald == int(cx[0].sum()) and np.array_equal(got.bald, (got.node[:, 2] == 0) & (got.axis == 0))
    onx, onz = got.axis == 0, got.axis == 2
    xs = x0 - r * (mesh[2][got.node[onx, 2]] - z1) / s
    zs = z1 - s * (mesh[0][got.node[onz, 0]] - x0) / r
    assert np.abs(got.position[onx, 0] - xs).max() <= 1e-12 * ext
    assert np.abs(got.position[onz, 2] - zs).max() <= 1e-12 * ext
    assert np.abs(got.position[onx, 2] - mesh[2][got.node[onx, 2]]).max() <= 1e-12 * ext
    assert np.abs(got.position[onz, 0] - mesh[0][got.node[onz, 0]]).max() <= 1e-12 * ext
    assert np.abs(got.position[:, 1] - mesh[1][got.node[:, 1]]).max() <= 1e-12 * ext
    assert np.abs(got.curv - b0 * s).max() <= b0 * grad_tol(b, h) + 1e-15 * b0 * s
    # the other sign of b0: the same crossings, no dip
    neg = run(mesh, tilted(mesh, -b0, s, r, x0, z1))
    assert neg.ncrossings == got.ncrossings and neg.ndips == 0
    # b0 = 0: curv = 0 G_x + 0 G_y, exactly 0
    zero = run(mesh, tilted(mesh, 0.0, s, r, x0, z1))
    assert zero.ncrossings == got.ncrossings and zero.ndips == 0 and len(zero.edge) == 0
    # the quadratic term: grad_z on the x edges
    c = 0.9 * r / (hi[2] - lo[2])
    bq = tilted(mesh, b0, s, r, x0, z1, c)
    quad = run(mesh, bq)
    on = quad.axis == 0
    ks = quad.node[on, 2]
    assert ks.min() == 0 and ks.max() == nz - 1 and quad.nbald > 0
    gz = r + 2.0 * c * (mesh[2][ks] - z1)
    err = np.abs(quad.grad[on, 2] - gz)
    print("   quadratic term: grad_z error on the x edges", err.max(), "at k = 0", err[ks == 0].max(),
          "first-order rows would be off by c h_z =", c * h[2])
    assert err.max() <= grad_tol(bq, h) and c * h[2] > 1e6 * grad_tol(bq, h)
    return got


def check_on_node_plane(run, mesh):
    """closed form (d): xc a mesh coordinate, so that B_z is exactly 0 on a node plane, with q of either sign: a zero
    counts as not positive, so exactly one record per (j, k): t = 0 on the edge above the plane for q > 0, t = 1 on
    the edge below it for q < 0"""
    lo, h, hi, n = box(mesh)
    nx, ny, nz = (int(v) for v in n)
    ic = nx // 2
    xc = mesh[0][ic]
    ext = (hi - lo).max()
    for q, be, edge_i in ((1.1, 5.0 * (hi[2] - lo[2]), ic), (-1.1, -5.0 * (hi[2] - lo[2]), ic - 1)):
        b = rope(mesh, q, be, 0.3, xc, mesh[2][0])
        assert np.all(b[2][:, :, ic] == 0.0)
        got = run(mesh, b)
        _ascending(got)
        assert got.ncrossings == got.ndips == ny * nz and got.nbald == ny, (q, got.ncrossings, got.ndips)
        assert np.all(got.axis == 0) and np.all(got.node[:, 0] == edge_i), q
        assert np.abs(got.position[:, 0] - xc).max() <= 1e-12 * ext
        assert np.all(got.b[:, 2] == 0.0)
        assert len(set((got.node[:, 1] + ny * got.node[:, 2]).tolist())) == ny * nz


def bad_value_fields(mesh):
    """(name, field, crossings or None): the fields of (f) - the rope of check_rope with a NaN block and with blocks of
    +Inf and -Inf (all three components) over its zero surface from face to face in y and z, and an all-zero field"""
    lo, _h, hi, n = box(mesh)
    nx, ny, nz = (int(v) for v in n)
    xc, zc = inside(mesh, 0, 4), inside(mesh, 2, nz // 2, 0.41)
    b = rope(mesh, 1.3, 0.225 * (hi[2] - lo[2]), 0.7, xc, zc)
    yield "zero", np.zeros(b.shape), 0
    for name, lo_v, hi_v in (("nan block", np.nan, np.nan), ("+inf block", np.inf, np.inf), ("-inf block", -np.inf, -np.inf),
                             ("inf blocks of both signs", np.inf, -np.inf)):
        c = b.copy()
        c[:, :, :, 2:5] = lo_v                      # i = 2 .. 4 holds the low end of every crossed edge
        c[:, :, :, 5:8] = hi_v
        yield name, c, None


def check_bad_values(run, mesh):
    """(f): no dip on any of bad_value_fields (the rope they damage has dips); crossings may be non-zero"""
    fields = list(bad_value_fields(mesh))
    for name, b, ncross in fields:
        got = run(mesh, b)
        print("bad values:", name, "crossings", got.ncrossings, "dips", got.ndips)
        assert got.ndips == 0 and got.nbald == 0 and len(got.edge) == 0, name
        assert ncross is None or got.ncrossings == ncross, name
        assert got.position.shape == (0, 3)
    return fields
