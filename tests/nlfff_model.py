"""CPU model of the history row of a Grad-Rubin pass, with the device's own summation order.

TEST INFRASTRUCTURE - plain numpy.  ndsmk_nlfff_metrics (csrc/field.hip) is nlfff_part_k + nlfff_final_k:

  per point     bb = (bx bx + by by) + bz bz; J = curl_h B with ddq's sums (csrc/diffq.hpp: 0.0 + v c1 + v c2 (+ v c3),
                the coefficients -1.5 / h, 2 / h, -0.5 / h on the lower plane, 1.5 / h, -2 / h, 0.5 / h on the upper,
                -0.5 / h, 0.5 / h inside); w = w_x (w_y w_z), trapezoid weights;
                v0 += w bb;  where sqrt(bb) > 0:  v1 += w (sqrt((cx cx + cy cy) + cz cz) / sqrt(bb)),
                v2 += w sqrt((jx jx + jy jy) + jz jz);  v3 += 1 where status == ZLO;  v4 = fmax(v4, |B - Bold|)
  nlfff_part_k  nb = min(ny nz, MAX_BLOCKS) blocks of BLOCK threads.  Block b walks the rows r = j + ny k = b, b + nb,
                ..., thread t the points i = t, t + BLOCK, ... of each: one accumulator per thread and value, from 0.0,
                across rows in that order.  Then the halving tree over the BLOCK threads: for o = BLOCK / 2 .. 1,
                sh[t] = sh[t] + sh[t + o] (fmax for v4) for t < o.
  nlfff_final_k one block: thread t folds the partials of the blocks t, t + BLOCK, ... in that order from 0.0, then the
                same tree.
  the row       [v4, 0.5 v0, v1 / v2 (0 unless v2 > 0), v3]

Every step is deterministic and the library is built without contraction, so the device's row can be asserted bit for
bit against history_row_model (tests/test_gpu_nlfff_edges.py); tests/test_nlfff_model.py ties the model to exact sums
that share none of its partition.  Arrays are numpy C order (3, nz, ny, nx) / (nz, ny, nx)."""
import numpy as np

from alpha_model import ZLO

BLOCK = 256           # kHelBlock of field.hip
MAX_BLOCKS = 2048     # kHelMaxBlocks


def spacing(mesh):
    """dq as the library forms it: q[1] - q[0] per axis"""
    return [float(q[1]) - float(q[0]) for q in mesh]


def trap_w(n, h):
    w = np.full(n, h)
    w[0] = w[-1] = 0.5 * h
    return w


def ddq(v, axis, h):
    """d/dq of v (nz, ny, nx) along the mesh axis (0: x), ddq's products and the order it adds them in"""
    v = np.moveaxis(v, 2 - axis, 0)
    d = np.empty_like(v)
    d[1:-1] = (0.0 + v[:-2] * (-0.5 / h)) + v[2:] * (0.5 / h)
    d[0] = ((0.0 + v[0] * (-1.5 / h)) + v[1] * (2.0 / h)) + v[2] * (-0.5 / h)
    d[-1] = ((0.0 + v[-1] * (1.5 / h)) + v[-2] * (-2.0 / h)) + v[-3] * (0.5 / h)
    return np.moveaxis(d, 0, 2 - axis)


def point_terms(mesh, b_new, b_old, status):
    """what every point adds, each (ny nz, nx) - a row of the kernel per row of the array: the energy term w bb, the
    two current terms and the mask of the points that add them (|B| > 0), the ZLO indicator, max_c |B_c - Bold_c|"""
    b_new = np.asarray(b_new, dtype=np.float64)
    b_old = np.asarray(b_old, dtype=np.float64)
    nz, ny, nx = b_new.shape[1:]
    dq = spacing(mesh)
    wx, wy, wz = (trap_w(n, h) for n, h in zip((nx, ny, nz), dq))
    wyz = wy[None, :] * wz[:, None]
    w = wx[None, None, :] * wyz[:, :, None]
    bx, by, bz = b_new
    bb = (bx * bx + by * by) + bz * bz
    jx = ddq(bz, 1, dq[1]) - ddq(by, 2, dq[2])
    jy = ddq(bx, 2, dq[2]) - ddq(bz, 0, dq[0])
    jz = ddq(by, 0, dq[0]) - ddq(bx, 1, dq[1])
    bm = np.sqrt(bb)
    ok = bm > 0.0
    cx, cy, cz = jy * bz - jz * by, jz * bx - jx * bz, jx * by - jy * bx
    sine = w * (np.sqrt((cx * cx + cy * cy) + cz * cz) / np.where(ok, bm, 1.0))
    cur = w * np.sqrt((jx * jx + jy * jy) + jz * jz)
    em = np.abs(bx - b_old[0])
    em = np.fmax(em, np.abs(by - b_old[1]))
    em = np.fmax(em, np.abs(bz - b_old[2]))
    rows = (nz * ny, nx)
    return dict(energy=(w * bb).reshape(rows), sine=sine.reshape(rows), current=cur.reshape(rows), ok=ok.reshape(rows),
                zlo=(np.asarray(status).reshape(rows) == ZLO).astype(np.float64), change=em.reshape(rows))


def blocks(nrows):
    return min(nrows, MAX_BLOCKS)


def _tree(acc, op):
    """sh[.., 0] after the halving tree along the last axis (BLOCK entries)"""
    sh = acc.copy()
    o = BLOCK // 2
    while o > 0:
        sh[..., :o] = op(sh[..., :o], sh[..., o:2 * o])
        o //= 2
    return sh[..., 0]


def _fold(terms, mask, op):
    """one value from the terms (nrows, nx) of the points in `mask`, in the kernels' order"""
    nrows, nx = terms.shape
    nb = blocks(nrows)
    mrows, mpts = -(-nrows // nb), -(-nx // BLOCK)
    t = np.zeros((mrows * nb, mpts * BLOCK))
    m = np.zeros(t.shape, dtype=bool)
    t[:nrows, :nx] = terms
    m[:nrows, :nx] = mask
    acc = np.zeros((nb, BLOCK))
    for r in range(mrows):                               # block b's rows b, b + nb, ...
        for q in range(mpts):                            # thread t's points t, t + BLOCK, ... of that row
            rows, cols = slice(r * nb, (r + 1) * nb), slice(q * BLOCK, (q + 1) * BLOCK)
            acc = np.where(m[rows, cols], op(acc, t[rows, cols]), acc)
    part = _tree(acc, op)                                # nlfff_part_k: one partial per block
    mfin = -(-nb // BLOCK)
    p = np.zeros(mfin * BLOCK)
    p[:nb] = part
    live = np.arange(mfin * BLOCK) < nb
    acc = np.zeros(BLOCK)
    for q in range(mfin):                                # nlfff_final_k: thread t's partials t, t + BLOCK, ...
        cols = slice(q * BLOCK, (q + 1) * BLOCK)
        acc = np.where(live[cols], op(acc, p[cols]), acc)
    return float(_tree(acc, op))


def kernel_sum(terms, mask=None):
    return _fold(terms, np.ones(terms.shape, dtype=bool) if mask is None else mask, np.add)


def kernel_max(terms):
    return _fold(terms, np.ones(terms.shape, dtype=bool), np.fmax)


def chain_length(nx, nrows):
    """the longest chain of additions a term passes through: the points of one thread, the 8 levels of the block's
    tree, the partials of one thread of the final fold, its 8 levels"""
    nb = blocks(nrows)
    return -(-nrows // nb) * -(-nx // BLOCK) + 8 + -(-nb // BLOCK) + 8


def history_row_model(mesh, b_new, b_old, status):
    """hist[k] of ndsm_hip_vecpot_nlfff for B^{k+1} = b_new, B^k = b_old and the pass's status, bit for bit"""
    p = point_terms(mesh, b_new, b_old, status)
    v0 = kernel_sum(p["energy"])
    v1 = kernel_sum(p["sine"], p["ok"])
    v2 = kernel_sum(p["current"], p["ok"])
    v3 = kernel_sum(p["zlo"])
    v4 = kernel_max(p["change"])
    return np.array([v4, 0.5 * v0, v1 / v2 if v2 > 0.0 else 0.0, v3])
