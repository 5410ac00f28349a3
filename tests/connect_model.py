"""Numpy restatements of the flux partitioning and connectivity semantics of include/ndsm_hip.h (ndsm_hip_partition,
ndsm_hip_vecpot_connect, "the keyed sum"), in the header's operand order, so that the device matches them bit for bit.
Nothing here comes from the library: partition_numpy finds the pointers with nine shifted comparisons and the roots by
following them, keysum_numpy adds the lane runs of every key column by column and then the tree, connect_numpy stands
on line_model.trace_numpy.  Arrays of a plane are (nsy, nsx), pixel p = i + nsx j, as in the Python layer."""
import numpy as np

import line_model

CONNECT_NONE = -9
ZLO = 5


def trap_weights(xs, ys):
    """w(p) = wx(i) wy(j), flat: hx inside, 0.5 hx on both end rows, likewise wy"""
    return (line_model.weights1(ys)[:, None] * line_model.weights1(xs)[None, :]).reshape(-1)


def keysum_numpy(keys, terms, nkeys):
    """The keyed sums of terms (n, or (n, m)) over the keys 1 .. nkeys (a key outside them is summed nowhere), (nkeys,)
    or (nkeys, m): the terms of a key in ascending index are its ranks; lane l of 64 adds the ranks l, l + 64, ... in
    that order from 0.0, then v[l] = v[l] + v[l + d] for l < d, d = 32 .. 1."""
    keys = np.asarray(keys).reshape(-1)
    T = np.asarray(terms, dtype=np.float64)
    flat = T.ndim == 1
    T = T.reshape(len(keys), -1)
    use = np.nonzero((keys >= 1) & (keys <= nkeys))[0]
    order = use[np.argsort(keys[use], kind="stable")]
    k = keys[order] - 1
    count = np.bincount(k, minlength=nkeys)
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    rank = np.arange(len(order)) - first[k]
    depth = int((count.max() + 63) // 64) if len(order) else 1
    pad = np.zeros((nkeys, 64, depth, T.shape[1]))
    have = np.zeros((nkeys, 64, depth), dtype=bool)
    pad[k, rank % 64, rank // 64] = T[order]
    have[k, rank % 64, rank // 64] = True
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.zeros((nkeys, 64, T.shape[1]))
        for q in range(depth):                      # (a lane adds nothing where it has no rank: not even a zero)
            v = np.where(have[:, :, q, None], v + pad[:, :, q], v)
        d = 32
        while d >= 1:
            v[:, :d] = v[:, :d] + v[:, d:2 * d]
            d //= 2
    out = v[:, 0]
    return out[:, 0] if flat else out


def partition_numpy(xs, ys, bz, thr):
    """dict(label (nsy,nsx) int32, ptr, root_of (flat; -1: not in), nin, K, root, sign, npix, flux, sx, sy) of the
    magnetogram bz (nsy,nsx)"""
    ny, nx = bz.shape
    n = nx * ny
    with np.errstate(invalid="ignore"):
        a = np.abs(bz)
        inn = a > thr
        pos = bz > 0.0
    idx = np.arange(n).reshape(ny, nx)
    best = np.full((ny, nx), -1.0)
    at = idx.copy()
    for dj in (-1, 0, 1):                           # ascending candidate index, strict >: ties stay with the smallest
        for di in (-1, 0, 1):
            js, je = max(0, -dj), min(ny, ny - dj)
            is_, ie = max(0, -di), min(nx, nx - di)
            tgt = (slice(js, je), slice(is_, ie))
            src = (slice(js + dj, je + dj), slice(is_ + di, ie + di))
            ok = inn[src] & (pos[src] == pos[tgt])
            with np.errstate(invalid="ignore"):
                take = ok & (a[src] > best[tgt])
            best[tgt] = np.where(take, a[src], best[tgt])
            at[tgt] = np.where(take, idx[src], at[tgt])
    ptr = np.where(inn, at, -1).reshape(-1)
    root_of = ptr.copy()
    live = root_of >= 0
    while True:                                     # to the fixed point, however many rounds that takes
        nxt = root_of.copy()
        nxt[live] = root_of[root_of[live]]
        if np.array_equal(nxt, root_of):
            break
        root_of = nxt
    roots = np.nonzero(root_of == np.arange(n))[0]
    K = len(roots)
    number = np.zeros(n, dtype=np.int64)
    number[roots] = np.arange(1, K + 1)
    label = np.where(live, number[np.maximum(root_of, 0)], 0).astype(np.int32)
    w = trap_weights(xs, ys)
    bf = bz.reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        f = bf * w
        X = np.tile(np.asarray(xs, dtype=np.float64), ny)
        Y = np.repeat(np.asarray(ys, dtype=np.float64), nx)
        sums = keysum_numpy(label, np.stack([f, f * X, f * Y], axis=1), K)
    return dict(label=label.reshape(ny, nx), ptr=ptr, root_of=root_of, nin=int(live.sum()), K=K,
                root=roots.astype(np.int64), sign=np.where(bf[roots] > 0.0, 1, -1).astype(np.int32),
                npix=np.bincount(label[label > 0] - 1, minlength=K).astype(np.int64),
                flux=sums[:, 0], sx=sums[:, 1], sy=sums[:, 2])


def connect_numpy(mesh, b, label, K, step, max_steps):
    """dict(dest, ends, length, status (per pixel, flat), ntraced, pa, pc, nlines, pflux) of the field b (3,nz,ny,nx)
    with the label map (ny,nx) of its lower face"""
    x, y, z = mesh
    nx, ny = len(x), len(y)
    n = nx * ny
    lo, h, hi, _n = line_model.box(mesh)
    lab = np.asarray(label).reshape(-1).astype(np.int64)
    a = np.where((lab >= 1) & (lab <= K), lab, 0)
    bzn = b[2, 0].reshape(-1)
    seeds = np.stack([np.tile(x, ny), np.repeat(y, nx), np.full(n, z[0])], axis=1)
    with np.errstate(invalid="ignore"):
        inside = np.all((seeds >= lo) & (seeds <= hi), axis=1)
        up, down = bzn > 0.0, bzn < 0.0
    run = (a != 0) & (up | down) & inside
    ends, length = seeds.copy(), np.zeros(n)
    status = np.full(n, line_model.OUTSIDE, dtype=np.int32)
    for sel, sgn in ((run & up, 1.0), (run & down, -1.0)):
        at = np.nonzero(sel)[0]
        if len(at) == 0:
            continue
        e, l, _i, s, _n2 = line_model.trace_numpy(mesh, b, None, seeds[at], step, max_steps, sgn)
        ends[at], length[at], status[at] = e, l, s
    dest = np.full(n, CONNECT_NONE, dtype=np.int32)
    i2 = np.clip(np.floor((ends[:, 0] - lo[0]) / h[0] + 0.5).astype(np.int64), 0, nx - 1)
    j2 = np.clip(np.floor((ends[:, 1] - lo[1]) / h[1] + 0.5).astype(np.int64), 0, ny - 1)
    c = np.where(status == ZLO, a[j2 * nx + i2], -status.astype(np.int64))
    dest[run] = c[run]
    base = K + 9
    key = np.where(run, a * base + (c + 8), 0)
    uniq, inverse = np.unique(key[run], return_inverse=True)
    dense = np.zeros(n, dtype=np.int64)
    dense[run] = inverse + 1
    term = np.abs(bzn) * trap_weights(x, y)
    return dict(dest=dest, ends=ends, length=length, status=status, ntraced=int(run.sum()),
                pa=(uniq // base).astype(np.int32), pc=(uniq % base - 8).astype(np.int32),
                nlines=np.bincount(inverse, minlength=len(uniq)).astype(np.int64),
                pflux=keysum_numpy(dense, term, len(uniq)))
