"""CPU model of the cascade of the measurement fit (ndsm_hip_vecpot_optimize_obs_cascade) and of the confidence-weighted
restriction behind it (ndsm_hip_resample_weighted, csrc/resample.hip), with the device's own operand order.

TEST INFRASTRUCTURE - plain numpy and Python loops, built on cascade_model's tap rule and optimize_obs_model.run.

  resample_weighted   the taps of an axis are the hat average's (cascade_model.taps, mode "average"); a destination node
                      with one tap copies it (q = 1, qsum = 1), any other takes the ascending source nodes f with
                      q_f > 0, qsum = sum q_f.  NOT normalised axis by axis: for every destination node and component
                      three sums run over the tensor of taps - for every z tap, for every y tap, the finished x sum;
                      then the y sum; then the z sum -, each left to right from its first term, each level
                      sum float(q_f) (inner value):  num from w[f] v[f], den from w[f], pln from v[f].  With
                      Q = (float(qsum_x) float(qsum_y)) float(qsum_z):  wdst = den / Q,  dst = num / den where
                      den > 0.0, otherwise pln / Q.  A node with one tap on every axis copies v[f] (and w[f]).
  paste_mask          the nodes a finer level takes from its own average G_l: 0 the k = 0 plane, 1 the six faces,
                      2 and 3 the same without the freed nodes (the k = 0 plane off its rim).
  cascade_obs         cascade_model.cascade with optimize_obs_model.run on every level (start "given" only: the
                      potential start needs the solver): (Bobs_l, wm_l) = the weighted restriction of the two planes
                      straight from the finest (without wm: the hat average of Bobs), free = 1 pastes with mask 3.

No constant is taken from the device code.  Arrays are numpy C order: fields (3, nz, ny, nx), w (nz, ny, nx), Bobs and
wm (3, ny, nx); shapes are (nz, ny, nx)."""
import numpy as np

import cascade_model as C
import optimize_obs_model as O


def wtaps(i, ns, nd):
    """([(f, q_f)], qsum) of destination node i: whole numbers; a single tap has q = 1 and qsum = 1"""
    t, qsum, _ = C.taps(i, ns, nd, "average")
    if len(t) == 1:
        return [(t[0][0], 1)], 1
    return t, qsum


def wsum(taps, inner):
    """one level of the rule: sum float(q_f) inner(f), left to right from its first term; inner gives (num, den, pln)"""
    if len(taps) == 1:
        return inner(taps[0][0])
    f, q = taps[0]
    acc = [float(q) * x for x in inner(f)]
    for f, q in taps[1:]:
        acc = [a + float(q) * x for a, x in zip(acc, inner(f))]
    return acc


def resample_weighted(v, wv, shape):
    """(dst, wdst) of v and its confidence wv, both (ncomp, nz, ny, nx) or (nz, ny, nx), on the nodes of `shape`; the
    components of a node are carried together (every operation is element by element)"""
    v, wv = np.asarray(v, dtype=np.float64), np.asarray(wv, dtype=np.float64)
    assert v.shape == wv.shape and v.ndim in (3, 4) and len(shape) == 3, (v.shape, wv.shape, shape)
    lead = v.shape[:-3]
    v4, w4 = v.reshape((-1,) + v.shape[-3:]), wv.reshape((-1,) + v.shape[-3:])
    nzs, nys, nxs = v4.shape[1:]
    nzd, nyd, nxd = (int(n) for n in shape)
    tx = [wtaps(i, nxs, nxd) for i in range(nxd)]
    ty = [wtaps(j, nys, nyd) for j in range(nyd)]
    tz = [wtaps(k, nzs, nzd) for k in range(nzd)]
    dst, wdst = np.empty((v4.shape[0], nzd, nyd, nxd)), np.empty((v4.shape[0], nzd, nyd, nxd))
    with np.errstate(all="ignore"):
        for k in range(nzd):
            for j in range(nyd):
                for i in range(nxd):
                    num, den, pln = wsum(tz[k][0], lambda fz: wsum(ty[j][0], lambda fy: wsum(
                        tx[i][0], lambda fx: (w4[:, fz, fy, fx] * v4[:, fz, fy, fx], w4[:, fz, fy, fx], v4[:, fz, fy, fx]))))
                    Q = (float(tx[i][1]) * float(ty[j][1])) * float(tz[k][1])
                    wdst[:, k, j, i] = den / Q
                    copy = len(tx[i][0]) == 1 and len(ty[j][0]) == 1 and len(tz[k][0]) == 1
                    dst[:, k, j, i] = pln if copy else np.where(den > 0.0, num / den, pln / Q)
    return dst.reshape(lead + dst.shape[1:]), wdst.reshape(lead + dst.shape[1:])


def paste_mask(shape, which):
    """the nodes (nz, ny, nx) that paste `which` overwrites"""
    assert which in (0, 1, 2, 3), which
    m = np.zeros(shape, dtype=bool)
    if which in (1, 3):
        m = C.faces(shape)
    else:
        m[0] = True
    if which >= 2:
        m[0, 1:-1, 1:-1] = False
    return m


def level_planes(shapes, bobs, wm):
    """([Bobs_l], [wm_l]) of every level, straight from the finest"""
    BO, WM = [bobs], [wm]
    for nz, ny, nx in shapes[1:]:
        if wm is None:
            BO.append(C.resample(bobs[:, None], (1, ny, nx), "average")[:, 0])
            WM.append(None)
        else:
            d, wd = resample_weighted(bobs[:, None], wm[:, None], (1, ny, nx))
            BO.append(np.ascontiguousarray(d[:, 0]))
            WM.append(np.ascontiguousarray(wd[:, 0]))
    return BO, WM


def cascade_obs(meshes, b, bobs=None, wm=None, nu=0.01, free=1, w=None, niter_max=10000, check=50, tol=1e-4, dt0=None,
                dt_min=None, hist_rows=None):
    """(B, [hist], [info], [start field of every level], [accepted L values], ([Bobs_l], [wm_l]), [result of every
    level]) of the cascade with start "given"; meshes finest first, lists indexed by level.  nu, niter_max, dt0, dt_min:
    one value for every level or one per level; defaults as optimize_obs_model.run on each level's own mesh"""
    assert free in (0, 1)
    n = len(meshes)
    b = np.asarray(b, dtype=np.float64)
    bobs = b[:, 0].copy() if bobs is None else np.asarray(bobs, dtype=np.float64)
    wm = None if wm is None else np.asarray(wm, dtype=np.float64)
    nus, nit, d0, dm = (C.per_level(v, n) for v in (nu, niter_max, dt0, dt_min))
    shapes = [C.shape_of(m) for m in meshes]
    G = [b] + [C.resample(b, s, "average") for s in shapes[1:]]
    W = [None] * n if w is None else [np.asarray(w, dtype=np.float64)] + [C.resample(w, s, "linear") for s in shapes[1:]]
    BO, WM = level_planes(shapes, bobs, wm)
    hist, info, starts, traces, results = [None] * n, [None] * n, [None] * n, [None] * n, [None] * n
    cur = None
    for l in range(n - 1, -1, -1):
        if cur is None:
            start = G[l].copy()
        else:
            start = C.resample(cur, shapes[l], "linear")
            m = paste_mask(shapes[l], 3 if free else 1)
            start[:, m] = G[l][:, m]
        starts[l] = start
        cur, hist[l], info[l], traces[l] = O.run(meshes[l], start, BO[l], WM[l], nus[l], free, W[l], niter_max=nit[l],
                                                 check=check, tol=tol, dt0=d0[l], dt_min=dm[l], hist_rows=hist_rows)
        results[l] = cur
    return cur, hist, info, starts, traces, (BO, WM), results
