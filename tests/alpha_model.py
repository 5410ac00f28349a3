"""What the alpha-map and Grad-Rubin tests share (test_alpha_model.py, test_gpu_alpha_map.py, test_gpu_nlfff.py): the
numpy restatement of ndsm_hip_vecpot_alpha_map (include/ndsm_hip.h) on top of line_model.trace_numpy, which the device
matches bit for bit, and the flux tube with a compact current that the accuracy tests use."""
import numpy as np

from line_model import box, grids, trace_numpy

ZLO = 5


def node_seeds(mesh):
    """the seed of every node, x fastest: r_d = lo_d + float(i_d) * h_d, as the kernel forms it"""
    lo, h, _hi, n = box(mesh)
    q = [lo[d] + np.arange(int(n[d])).astype(np.float64) * h[d] for d in range(3)]
    Z, Y, X = np.meshgrid(q[2], q[1], q[0], indexing="ij")
    return np.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], axis=1)


def bilinear(mesh, alpha0, ends):
    """the bilinear interpolant of alpha0 (ny,nx) at the (x, y) of ends (m,3): line_cell's cell and unclamped
    fractions on two axes, c0 = v00 + fx (v10 - v00), c1 = v01 + fx (v11 - v01), c0 + fy (c1 - c0)"""
    lo, h, _hi, n = box(mesh)
    nx = int(n[0])
    u = (ends[:, :2] - lo[:2]) / h[:2]
    c = np.minimum(np.maximum(np.floor(u), 0.0), n[:2] - 2.0)
    f = u - c
    ci = c.astype(np.int64)
    base = ci[:, 0] + nx * ci[:, 1]
    a = np.ascontiguousarray(alpha0, dtype=np.float64).reshape(-1)
    v00, v10, v01, v11 = a[base], a[base + 1], a[base + nx], a[base + nx + 1]
    c0 = v00 + f[:, 0] * (v10 - v00)
    c1 = v01 + f[:, 0] * (v11 - v01)
    return c0 + f[:, 1] * (c1 - c0)


def alpha_of_ends(mesh, alpha0, ends, status):
    """alpha per line from its end and status: the interpolant where the line ended on the lower face, else +0.0"""
    out = np.zeros(len(ends))
    hit = status == ZLO
    out[hit] = bilinear(mesh, alpha0, ends[hit])
    return out


def alpha_map_numpy(mesh, b, alpha0, polarity, step, max_steps):
    """(alpha, status), each (nz,ny,nx): the node seeds traced with sgn = -polarity, then the bilinear rule"""
    _lo, _h, _hi, n = box(mesh)
    shape = (int(n[2]), int(n[1]), int(n[0]))
    ends, _len, _int, status, _ns = trace_numpy(mesh, b, None, node_seeds(mesh), step, max_steps, -float(polarity))
    return alpha_of_ends(mesh, alpha0, ends, status).reshape(shape), status.reshape(shape)


def default_max_steps(mesh, step):
    return int(np.ceil(4.0 * sum(len(q) for q in mesh) / step))


# ---------------------------------------------------------------------------------------------------------------------
# the flux tube with a compact current
# ---------------------------------------------------------------------------------------------------------------------
def tube_mesh(n, nz=9, height=0.25):
    """the unit square with n points per side and a z-short box: only x and y are refined with n"""
    return [np.linspace(0.0, 1.0, n), np.linspace(0.0, 1.0, n), np.linspace(0.0, height, nz)]


def flux_tube(mesh, qa=1.0, b0=1.0):
    """A straight flux tube along z through the centre of the box, radius a = 0.3 of the shorter horizontal extent,
    twist q a = qa.  Inside r <= a it is the Gold-Hoyle tube, B_z = B0 / (1 + q^2 r^2), B_phi = B0 q r / (1 + q^2 r^2),
    alpha = 2 q / (1 + q^2 r^2); outside B_z = B_z(a) and B_phi = B_phi(a) a / r, a potential field: continuous,
    force-free everywhere, alpha = 0 outside.  Returns (b (3,nz,ny,nx), alpha (nz,ny,nx), r (nz,ny,nx), a)."""
    lo, _h, hi, _n = box(mesh)
    X, Y, _Z = grids(mesh)
    xc, yc = 0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1])
    a = 0.3 * min(hi[0] - lo[0], hi[1] - lo[1])
    q = qa / a
    dx, dy = X - xc, Y - yc
    r2 = dx * dx + dy * dy
    r = np.sqrt(r2)
    inside = r <= a
    den = 1.0 + q * q * np.where(inside, r2, a * a)
    bz = b0 / den
    # B_phi / r: B0 q / (1 + q^2 r^2) inside, B_phi(a) a / r^2 outside
    w = np.where(inside, b0 * q / den, (b0 * q * a / den) * a / np.where(inside, 1.0, r2))
    b = np.stack([-w * dy, w * dx, bz])
    alpha = np.where(inside, 2.0 * q / den, 0.0)
    return b, alpha, r, a
