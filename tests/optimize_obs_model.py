"""CPU model of the optimization-method solver with a measurement term and a freed lower face, with the device's own
expressions and summation order.

TEST INFRASTRUCTURE - plain numpy, built on optimize_model and nlfff_model.  ndsm_hip_vecpot_optimize_obs
(csrc/optimize_obs.hip, vecpot_optimize_obs) is ndsm_hip_vecpot_optimize (optimize_model's docstring) with

  obs_omega_k   a third sum: every node of the k = 0 plane - whatever |B| is - adds
                W2 ((wm_x (dx dx) + wm_y (dy dy)) + wm_z (dz dz)),  d = B(k = 0) - Bobs,  W2 = w_x w_y (no z factor;
                without a wm array the three factors are not applied), in the same row walk, tree and fold: the
                threads of the rows with k > 0 add nothing to it.
  obs_final_k   L_m = that sum, L = (L_f + L_d) + nu L_m; the decision and the stop flag as before.
  obs_force_k   interior nodes: T = B + dt F~ as before.  The five other faces and the rim of the lower face (i = 0,
                nx - 1 or j = 0, ny - 1): T = B.  The other nodes of the k = 0 plane, with free = 1:  T = B + dt H,
                  H = (F~ + c G) - c (nu (wm (B - Bobs)))   per component,  c = 2.0 / h_z,
                F~ optimize_model.force's expressions evaluated at the face node (ddq's rows there: centred in x and y,
                the three-point one-sided row in z, for curl_h P, grad_h s and grad_h w alike),
                G = w (-P_y, P_x, -s) at the node (without a weight array the factor w is not applied; without a wm
                array neither is wm).  With free = 0 the whole plane is copied.
  vecpot_optimize_obs  the driver of optimize_model.run; a history row is [tries, L, L_f, L_d, L_m, dt, accepted].

Every step is deterministic and the library is built without contraction, so the device's field, history and info can
be asserted bit for bit against run() (tests/test_gpu_optimize_obs.py); tests/test_optimize_obs_model.py checks H
against the derivative of the model's own functional.  Arrays are numpy C order: fields (3, nz, ny, nx), w (nz, ny, nx),
Bobs and wm (3, ny, nx)."""
import numpy as np

import optimize_model as M
from nlfff_model import ddq, kernel_sum, spacing, trap_w

VARIANTS = ("full", "g_only", "g_sign", "g_no_w", "g_no_s", "g_half", "no_nu", "half_nu")


def plane_weights(mesh, shape):
    """W2 = w_x w_y, (ny, nx)"""
    nz, ny, nx = shape
    dq = spacing(mesh)
    wx, wy = trap_w(nx, dq[0]), trap_w(ny, dq[1])
    return wx[None, :] * wy[:, None]


def measure_terms(mesh, b, bobs, wm=None):
    """what every node adds to L_m (nz, ny, nx) and the mask of the nodes that add: the k = 0 plane"""
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = b[:, 0] - bobs
        if wm is None:
            t = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        else:
            t = (wm[0] * (d[0] * d[0]) + wm[1] * (d[1] * d[1])) + wm[2] * (d[2] * d[2])
        t = plane_weights(mesh, b.shape[1:]) * t
    lm = np.zeros(b.shape[1:])
    lm[0] = t
    on = np.zeros(b.shape[1:], dtype=bool)
    on[0] = True
    return lm, on


def functional(mesh, b, bobs, wm=None, nu=0.0, w=None, terms=None):
    """(L, L_f, L_d, L_m) of b in the kernels' summation order"""
    p = M.point_terms(mesh, b, w) if terms is None else terms
    _, lf, ld = M.functional(mesh, b, w, p)
    nz, ny, nx = p["ok"].shape
    lm, on = measure_terms(mesh, b, bobs, wm)
    lm = kernel_sum(lm.reshape(nz * ny, nx), on.reshape(nz * ny, nx))
    with np.errstate(all="ignore"):
        return (lf + ld) + nu * lm, lf, ld, lm


def force_everywhere(mesh, b, w=None, terms=None):
    """optimize_model.force's F~ without its face mask: every node, with ddq's one-sided rows on the end planes"""
    b = np.asarray(b, dtype=np.float64)
    dq = spacing(mesh)
    p = M.point_terms(mesh, b, w) if terms is None else terms
    o, j, d = p["omega"], p["j"], p["d"]
    with np.errstate(all="ignore"):
        pp = M.cross(o, b)
        s = (o[0] * b[0] + o[1] * b[1]) + o[2] * b[2]
        cp = M.curl(pp, dq)
        q = M.cross(o, j)
        gs = [ddq(s, a, dq[a]) for a in range(3)]
        oo = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]
        f = [(((cp[a] - q[a]) - gs[a]) + o[a] * d) + oo * b[a] for a in range(3)]
        if w is not None:
            gw = [ddq(w, a, dq[a]) for a in range(3)]
            r = M.cross(pp, gw)
            f = [(w * f[a] - r[a]) - s * gw[a] for a in range(3)]
    return np.array(f), pp, s


def forces(mesh, b, bobs, wm=None, nu=0.0, w=None, terms=None, variant="full"):
    """(F~ (3, nz, ny, nx): the interior nodes, 0 on the faces;  H (3, ny, nx): the nodes of the k = 0 plane off its
    rim, 0 on the rim).  variant (tests of the formula only): "g_only" drops F~ from H, "g_sign" turns G round,
    "g_no_w" drops its w, "g_no_s" the s of its z component, "g_half" takes 1 / h_z for 2 / h_z on G, "no_nu" drops
    the measurement term, "half_nu" halves it"""
    assert variant in VARIANTS, variant
    b = np.asarray(b, dtype=np.float64)
    dq = spacing(mesh)
    f, pp, s = force_everywhere(mesh, b, w, terms)
    ft = np.zeros_like(b)
    ft[:, 1:-1, 1:-1, 1:-1] = f[:, 1:-1, 1:-1, 1:-1]
    c = 2.0 / dq[2]
    with np.errstate(all="ignore"):
        g = [-pp[1][0], pp[0][0], -s[0]]
        if variant == "g_no_s":
            g[2] = 0.0 * g[2]
        if w is not None and variant != "g_no_w":
            g = [w[0] * g[a] for a in range(3)]
        if variant == "g_sign":
            g = [-g[a] for a in range(3)]
        d = b[:, 0] - bobs
        m = d if wm is None else wm * d
        cg = 1.0 / dq[2] if variant == "g_half" else c
        knu = {"no_nu": 0.0, "half_nu": 0.5 * nu}.get(variant, nu)
        face = 0.0 * f[:, 0] if variant == "g_only" else f[:, 0]
        hh = [(face[a] + cg * g[a]) - c * (knu * m[a]) for a in range(3)]
    h = np.zeros(b[:, 0].shape)
    h[:, 1:-1, 1:-1] = np.array(hh)[:, 1:-1, 1:-1]
    return ft, h


def trial(b, dt, ft, h, free):
    """T = B + dt F~ inside, T = B + dt H on the freed nodes of the lower face, the bits of B everywhere else"""
    t = np.array(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        t[:, 1:-1, 1:-1, 1:-1] = (b + dt * ft)[:, 1:-1, 1:-1, 1:-1]
        if free:
            t[:, 0, 1:-1, 1:-1] = (b[:, 0] + dt * h)[:, 1:-1, 1:-1]
    return t


def run(mesh, b0, bobs=None, wm=None, nu=0.0, free=1, w=None, niter_max=10000, check=50, tol=1e-4, dt0=None,
        dt_min=None, hist_rows=None):
    """(B, hist, info, accepted L values) of the driver, bit for bit; defaults as VecPot.optimize_obs"""
    assert free in (0, 1) and nu >= 0.0
    b = np.array(b0, dtype=np.float64)
    bobs = b[:, 0].copy() if bobs is None else np.asarray(bobs, dtype=np.float64)
    if w is not None:
        w = np.asarray(w, dtype=np.float64)
    if wm is not None:
        wm = np.asarray(wm, dtype=np.float64)
    if dt0 is None:
        dt0 = 0.1 * min(spacing(mesh)) ** 2
    if dt_min is None:
        dt_min = 1e-6 * dt0
    if hist_rows is None:
        hist_rows = -(-niter_max // check) + 2
    dt = float(dt0)
    terms = M.point_terms(mesh, b, w)
    L, Lf, Ld, Lm = functional(mesh, b, bobs, wm, nu, w, terms)
    tries = accepted = 0
    trace = [L]
    hist = np.zeros((hist_rows, 7))
    hist[0] = [tries, L, Lf, Ld, Lm, dt, accepted]
    rows = 1
    stop = 2 if dt < dt_min else 0
    flag = stop == 2
    lprev = L
    done = 0
    while stop == 0 and done < niter_max:
        n = min(check, niter_max - done)
        for _ in range(n):
            if flag:
                break
            ft, h = forces(mesh, b, bobs, wm, nu, w, terms)
            t = trial(b, dt, ft, h, free)
            tt = M.point_terms(mesh, t, w)
            lt = functional(mesh, t, bobs, wm, nu, w, tt)
            tries += 1
            if lt[0] < L:
                b, terms = t, tt
                L, Lf, Ld, Lm = lt
                accepted += 1
                dt = dt * 1.01
                trace.append(L)
            else:
                dt = dt * 0.5
            flag = dt < dt_min
        done += n
        rows = min(rows + 1, hist_rows)
        hist[rows - 1] = [tries, L, Lf, Ld, Lm, dt, accepted]
        if flag:
            stop = 2
        elif n == check:
            if lprev - L <= tol * lprev:
                stop = 1
            lprev = L
    return b, hist[:rows].copy(), (rows, tries, stop), trace
