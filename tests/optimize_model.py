"""CPU model of the optimization-method force-free solver, with the device's own expressions and summation order.

TEST INFRASTRUCTURE - plain numpy.  ndsm_hip_vecpot_optimize (csrc/optimize.hip, vecpot_optimize) is

  opt_omega_k   per node, faces included: J = curl_h B and D = (d_x B_x + d_y B_y) + d_z B_z with ddq's sums
                (nlfff_model.ddq), bb = (bx bx + by by) + bz bz, C = J x B; where bb > 0:
                Omega = (C - D B) / bb,  v0 += Ww (((cx cx + cy cy) + cz cz) / bb),  v1 += Ww (D D),
                Ww = (w_x (w_y w_z)) w (trapezoid weights; without a weight array the last factor is not applied);
                elsewhere Omega = 0 and nothing is added.  The sums: nlfff_model.kernel_sum's partition.
  opt_final_k   L_f = v0, L_d = v1, L = L_f + L_d; a try is accepted when L_T < L (dt *= 1.01), else rejected
                (dt *= 0.5); dt < dt_min raises the stop flag.
  opt_force_k   on interior nodes, P = Omega x B and s = (ox bx + oy by) + oz bz at the neighbours:
                F = (((curl_h P - Omega x J) - grad_h s) + Omega D) + |Omega|^2 B per component, with a weight array
                F~ = (w F - P x grad_h w) - s grad_h w, T = B + dt F~; T = B on the six faces.
  vecpot_optimize  row 0 = the start; then check tries at a time (the last interval may be shorter), one history row
                after each, [tries, L, L_f, L_d, dt, accepted]; stop 2 when the flag is up, else - after a whole
                interval - stop 1 when L_prev - L <= tol L_prev; stop 0 after niter_max tries.

Every step is deterministic and the library is built without contraction, so the device's field, history and info can
be asserted bit for bit against run() (tests/test_gpu_optimize.py); tests/test_optimize_model.py checks the model's
force against the derivative of its own functional.  Arrays are numpy C order (3, nz, ny, nx) / (nz, ny, nx)."""
import numpy as np

from nlfff_model import ddq, kernel_sum, spacing, trap_w


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def curl(v, dq):
    """curl_k's expressions"""
    return [ddq(v[2], 1, dq[1]) - ddq(v[1], 2, dq[2]),
            ddq(v[0], 2, dq[2]) - ddq(v[2], 0, dq[0]),
            ddq(v[1], 0, dq[0]) - ddq(v[0], 1, dq[1])]


def weights(mesh, shape):
    """W = w_x (w_y w_z), (nz, ny, nx)"""
    nz, ny, nx = shape
    dq = spacing(mesh)
    wx, wy, wz = (trap_w(n, h) for n, h in zip((nx, ny, nz), dq))
    wyz = wy[None, :] * wz[:, None]
    return wx[None, None, :] * wyz[:, :, None]


def point_terms(mesh, b, w=None):
    """Omega (3, nz, ny, nx), J, D, and what every node adds to L_f and L_d with the mask of the nodes that add"""
    b = np.asarray(b, dtype=np.float64)
    dq = spacing(mesh)
    bx, by, bz = b
    W = weights(mesh, b.shape[1:])
    if w is not None:
        W = W * w
    with np.errstate(all="ignore"):                   # (a step far too large overflows, on the device too)
        bb = (bx * bx + by * by) + bz * bz
        j = curl(b, dq)
        d = (ddq(bx, 0, dq[0]) + ddq(by, 1, dq[1])) + ddq(bz, 2, dq[2])
        c = cross(j, b)
        ok = bb > 0.0
        den = np.where(ok, bb, 1.0)
        omega = np.array([np.where(ok, (c[q] - d * b[q]) / den, 0.0) for q in range(3)])
        lf = W * (((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) / den)
        ld = W * (d * d)
    return dict(omega=omega, j=j, d=d, lf=lf, ld=ld, ok=ok)


def functional(mesh, b, w=None, terms=None):
    """(L, L_f, L_d) of b in the kernels' summation order"""
    p = point_terms(mesh, b, w) if terms is None else terms
    nz, ny, nx = p["ok"].shape
    rows = (nz * ny, nx)
    lf = kernel_sum(p["lf"].reshape(rows), p["ok"].reshape(rows))
    ld = kernel_sum(p["ld"].reshape(rows), p["ok"].reshape(rows))
    return lf + ld, lf, ld


def force(mesh, b, w=None, terms=None, variant="full"):
    """F~ (3, nz, ny, nx) on the interior nodes, 0 on the faces.  variant (tests of the formula only): "no_pxgw" drops
    P x grad w, "no_sgw" drops s grad w, "wf" keeps w F alone"""
    b = np.asarray(b, dtype=np.float64)
    dq = spacing(mesh)
    p = point_terms(mesh, b, w) if terms is None else terms
    o, j, d = p["omega"], p["j"], p["d"]
    with np.errstate(all="ignore"):
        pp = cross(o, b)
        s = (o[0] * b[0] + o[1] * b[1]) + o[2] * b[2]
        cp = curl(pp, dq)
        q = cross(o, j)
        gs = [ddq(s, a, dq[a]) for a in range(3)]
        oo = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]
        f = [(((cp[a] - q[a]) - gs[a]) + o[a] * d) + oo * b[a] for a in range(3)]
        if w is not None:
            gw = [ddq(w, a, dq[a]) for a in range(3)]
            r = cross(pp, gw)
            if variant == "full":
                f = [(w * f[a] - r[a]) - s * gw[a] for a in range(3)]
            elif variant == "no_pxgw":
                f = [w * f[a] - s * gw[a] for a in range(3)]
            elif variant == "no_sgw":
                f = [w * f[a] - r[a] for a in range(3)]
            else:
                assert variant == "wf", variant
                f = [w * f[a] for a in range(3)]
    out = np.zeros_like(b)
    out[:, 1:-1, 1:-1, 1:-1] = np.array(f)[:, 1:-1, 1:-1, 1:-1]
    return out


def trial(b, dt, ft):
    """T = B + dt F~ inside, the bits of B on the faces"""
    t = np.array(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        t[:, 1:-1, 1:-1, 1:-1] = (b + dt * ft)[:, 1:-1, 1:-1, 1:-1]
    return t


def run(mesh, b0, w=None, niter_max=10000, check=50, tol=1e-4, dt0=None, dt_min=None, hist_rows=None):
    """(B, hist, info, accepted L values) of the driver, bit for bit; defaults as VecPot.optimize"""
    b = np.array(b0, dtype=np.float64)
    if w is not None:
        w = np.asarray(w, dtype=np.float64)
    if dt0 is None:
        dt0 = 0.1 * min(spacing(mesh)) ** 2
    if dt_min is None:
        dt_min = 1e-6 * dt0
    if hist_rows is None:
        hist_rows = -(-niter_max // check) + 2
    dt = float(dt0)
    terms = point_terms(mesh, b, w)
    L, Lf, Ld = functional(mesh, b, w, terms)
    tries = accepted = 0
    trace = [L]
    hist = np.zeros((hist_rows, 6))
    hist[0] = [tries, L, Lf, Ld, dt, accepted]
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
            t = trial(b, dt, force(mesh, b, w, terms))
            tt = point_terms(mesh, t, w)
            lt = functional(mesh, t, w, tt)
            tries += 1
            if lt[0] < L:
                b, terms = t, tt
                L, Lf, Ld = lt
                accepted += 1
                dt = dt * 1.01
                trace.append(L)
            else:
                dt = dt * 0.5
            flag = dt < dt_min
        done += n
        rows = min(rows + 1, hist_rows)
        hist[rows - 1] = [tries, L, Lf, Ld, dt, accepted]
        if flag:
            stop = 2
        elif n == check:
            if lprev - L <= tol * lprev:
                stop = 1
            lprev = L
    return b, hist[:rows].copy(), (rows, tries, stop), trace


# ---- the fields of the tests -------------------------------------------------------------------------------------

def abc_field(mesh, alpha=2.0, coef=(1.0, 0.7, 0.4)):
    """the ABC field: curl B = alpha B, div B = 0"""
    x, y, z = (np.asarray(q, dtype=np.float64) for q in mesh)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    a, b, c = coef
    return np.array([a * np.sin(alpha * Z) + c * np.cos(alpha * Y),
                     b * np.sin(alpha * X) + a * np.cos(alpha * Z),
                     c * np.sin(alpha * Y) + b * np.cos(alpha * X)])


def bump(mesh, power=2):
    """a smooth function that vanishes on the six faces (with its first derivative for power = 2), 1 at the centre"""
    u = [(np.asarray(q, dtype=np.float64) - q[0]) / (q[-1] - q[0]) for q in mesh]
    Z, Y, X = np.meshgrid(u[2], u[1], u[0], indexing="ij")
    return (np.sin(np.pi * X) * np.sin(np.pi * Y) * np.sin(np.pi * Z)) ** power


def perturbed_abc(mesh, amp=0.3):
    """(the exact force-free field, the same with an interior bump of that height on B_x and half of it on B_z)"""
    exact = abc_field(mesh)
    b = exact.copy()
    g = bump(mesh)
    b[0] += amp * g
    b[2] -= 0.5 * amp * g
    return exact, b


def box(n, ny=None):
    """n x (ny or n) x ((n - 1) / 2 + 1) nodes on [0, 2] x [0, 2] x [0, 1]"""
    return (np.linspace(0.0, 2.0, n), np.linspace(0.0, 2.0, ny or n), np.linspace(0.0, 1.0, (n - 1) // 2 + 1))
