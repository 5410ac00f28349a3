"""CPU model of the coarse-to-fine cascade of the optimization method, with the device's own operand order.

TEST INFRASTRUCTURE - plain numpy.  ndsm_hip_resample (csrc/resample.hip) applies one 1-D rule along x, then y, then z;
each finished value depends on its own taps only, so applying the rule to the whole array axis by axis gives the bits
of the kernel's nesting.  The rule, ns source nodes and nd destination nodes on one axis, whole numbers throughout:

  mode "linear"   a = i (ns - 1), j = a div (nd - 1), r = a mod (nd - 1); r = 0 copies v[j], otherwise
                  theta = float(r) / float(nd - 1) and the value is (1.0 - theta) v[j] + theta v[j + 1].
  mode "average"  (nd <= ns) node 0 copies v[0], node nd - 1 copies v[ns - 1]; any other node takes the source nodes f,
                  ascending, with q_f = (ns - 1) - |f (nd - 1) - i (ns - 1)| > 0: one such node is copied, several give
                  (sum float(q_f) v[f]) / float(sum q_f), the sum left to right from its first term.
  ns = nd = 1     copied.

cascade() strings optimize_model.run calls together as vecpot_optimize_cascade does (start "given" only: the potential
start needs the solver).  No constant is taken from the device code.  Arrays are numpy C order (ncomp, nz, ny, nx) /
(nz, ny, nx); shapes are (nz, ny, nx)."""
import numpy as np

import optimize_model as M

MODES = ("linear", "average")


def taps(i, ns, nd, mode):
    """[(f, q_f)] of destination node i and the divisor (None: a copy or the linear rule), theta for the linear rule"""
    if ns == 1 and nd == 1:
        return [(0, None)], None, None
    if ns < 2 or nd < 2:
        raise ValueError("an axis needs at least 2 nodes on both sides, or 1 on both: %d -> %d" % (ns, nd))
    if mode == "linear":
        a = i * (ns - 1)
        j, r = a // (nd - 1), a % (nd - 1)
        if r == 0:
            return [(j, None)], None, None
        return [(j, None), (j + 1, None)], None, float(r) / float(nd - 1)
    if nd > ns:
        raise ValueError("the hat average cannot refine: %d -> %d" % (ns, nd))
    if i == 0:
        return [(0, None)], None, None
    if i == nd - 1:
        return [(ns - 1, None)], None, None
    t = [(f, (ns - 1) - abs(f * (nd - 1) - i * (ns - 1))) for f in range(ns)]
    t = [(f, q) for f, q in t if q > 0]
    return t, sum(q for _, q in t), None


def resample_axis(v, axis, nd, mode):
    """the 1-D rule along one axis of v"""
    v = np.moveaxis(v, axis, 0)
    ns = v.shape[0]
    out = np.empty((nd,) + v.shape[1:])
    for i in range(nd):
        t, qsum, theta = taps(i, ns, nd, mode)
        if len(t) == 1:
            out[i] = v[t[0][0]]
        elif theta is not None:
            out[i] = (1.0 - theta) * v[t[0][0]] + theta * v[t[1][0]]
        else:
            acc = float(t[0][1]) * v[t[0][0]]
            for f, q in t[1:]:
                acc = acc + float(q) * v[f]
            out[i] = acc / float(qsum)
    return np.moveaxis(out, 0, axis)


def resample(v, shape, mode):
    """v (ncomp, nz, ny, nx) or (nz, ny, nx) on the nodes of `shape` = (nz, ny, nx): x first, then y, then z"""
    assert mode in MODES, mode
    v = np.asarray(v, dtype=np.float64)
    assert v.ndim in (3, 4) and len(shape) == 3, (v.shape, shape)
    with np.errstate(all="ignore"):
        for axis, nd in ((-1, shape[2]), (-2, shape[1]), (-3, shape[0])):
            v = resample_axis(v, axis, int(nd), mode)
    return np.ascontiguousarray(v)


def cascade_shapes(shape, levels, min_nodes=4):
    """the rule of ndsm_amd.cascade_shapes, restated: n -> (n + 1) // 2 unless that falls below min_nodes"""
    out = [tuple(int(n) for n in shape)]
    for _ in range(levels - 1):
        nxt = tuple((n + 1) // 2 if (n + 1) // 2 >= min_nodes else n for n in out[-1])
        if nxt == out[-1]:
            raise ValueError("no axis of %r can shrink" % (out[-1],))
        out.append(nxt)
    return out


def shape_of(mesh):
    return (len(mesh[2]), len(mesh[1]), len(mesh[0]))


def faces(shape):
    m = np.ones(shape, dtype=bool)
    m[1:-1, 1:-1, 1:-1] = False
    return m


def per_level(v, n):
    return list(v) if isinstance(v, (list, tuple)) else [v] * n


def cascade(meshes, b, w=None, niter_max=10000, check=50, tol=1e-4, dt0=None, dt_min=None, hist_rows=None):
    """(B, [hist], [info], [start field of every level]) of the cascade with start "given"; meshes finest first, lists
    indexed by level.  niter_max, dt0, dt_min: one value for every level or one per level; defaults as
    optimize_model.run on each level's own mesh"""
    n = len(meshes)
    b = np.asarray(b, dtype=np.float64)
    nit, d0, dm = per_level(niter_max, n), per_level(dt0, n), per_level(dt_min, n)
    shapes = [shape_of(m) for m in meshes]
    G = [b] + [resample(b, s, "average") for s in shapes[1:]]
    W = [None] * n if w is None else [np.asarray(w, dtype=np.float64)] + [resample(w, s, "linear") for s in shapes[1:]]
    hist, info, starts = [None] * n, [None] * n, [None] * n
    cur = None
    for l in range(n - 1, -1, -1):
        if cur is None:
            start = G[l].copy()
        else:
            start = resample(cur, shapes[l], "linear")
            f = faces(shapes[l])
            start[:, f] = G[l][:, f]
        starts[l] = start
        cur, hist[l], info[l], _ = M.run(meshes[l], start, W[l], niter_max=nit[l], check=check, tol=tol, dt0=d0[l],
                                         dt_min=dm[l], hist_rows=hist_rows)
    return cur, hist, info, starts
