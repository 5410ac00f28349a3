"""CPU model of the magnetogram preprocessing, with the device's own expressions and summation order.

TEST INFRASTRUCTURE - plain numpy.  ndsm_hip_vecpot_preprocess (csrc/preprocess.hip, vecpot_preprocess) is

  pre_sums_k    per node of the plane: w = w_x w_y (trapezoid weights), x = (i - 0.5 (nx - 1)) hx, y likewise,
                e = (bz bz - bx bx) - by by, bb = (bx bx + by by) + bz bz, d = B - Bo,
                Lambda_c = ((v[i-1] + v[i+1]) - 2 v) rx + ((v[j-1] + v[j+1]) - 2 v) ry on interior nodes, rx = 1 / (hx hx),
                0 on the edge nodes; the eleven terms
                w (bx bz), w (by bz), w e, w (x e), w (y e), w ((y bx) bz - (x by) bz), w (dx dx + dy dy), w (dz dz),
                (lx lx + ly ly) + lz lz, w bb, w (sqrt(x x + y y) bb)
                summed in nlfff_model.kernel_sum's partition over ny rows of nx points.
  pre_final_k   S9 = hh v9; L1 = ((S1 S1 + S2 S2) + S3 S3) / (E E), L2 likewise with M, L3h = S7 / E, L3z = S8 / E,
                L4 = ((hh hh) S9) / E, L = (((mu1 L1 + mu2 L2) + mu3h L3h) + mu3z L3z) + mu4 L4; a try is accepted when
                L_T < L (dt *= 1.01), else rejected (dt *= 0.5); dt < dt_min raises the stop flag.
  pre_update_k  at every node, with the sums of the current field: T = B - (dt (E / hh)) G,
                G_c = w ((a f1_c + b f2_c) + c3 d_c) + c4 (stencil of Lambda_c, Lambda 0 outside the plane)
  vecpot_preprocess  E = S10, M = S11 of the observation; row 0 = the start; then check tries at a time (the last
                interval may be shorter), one history row after each; stop 2 when the flag is up, else - after a whole
                interval - stop 1 when L_prev - L <= tol L_prev; stop 0 after niter_max tries.

Every step is deterministic and the library is built without contraction, so the device's field, history and info can
be asserted bit for bit against run() (tests/test_gpu_preprocess.py); tests/test_preprocess_model.py checks the model's
gradient against the derivative of its own functional.  Arrays are numpy C order (3, ny, nx)."""
import numpy as np

from nlfff_model import kernel_sum, spacing, trap_w

MU = (1.0, 1.0, 1e-3, 1e-2, 1e-2)
ROW = 17


def plane(mesh):
    """(hx, hy), W (ny, nx), x (nx), y (ny) of the lower face"""
    hx, hy = spacing(mesh)[:2]
    nx, ny = len(mesh[0]), len(mesh[1])
    w = trap_w(nx, hx)[None, :] * trap_w(ny, hy)[:, None]
    x = (np.arange(nx, dtype=np.float64) - 0.5 * float(nx - 1)) * hx
    y = (np.arange(ny, dtype=np.float64) - 0.5 * float(ny - 1)) * hy
    return (hx, hy), w, x, y


def stencil(v, hx, hy, zero_outside):
    """the 5-point stencil on v (ny, nx): on the interior nodes, 0 on the edge (zero_outside False), or at every node
    with v taken as 0 outside the plane"""
    rx, ry = 1.0 / (hx * hx), 1.0 / (hy * hy)
    p = np.zeros((v.shape[0] + 2, v.shape[1] + 2))
    p[1:-1, 1:-1] = v
    full = ((p[1:-1, :-2] + p[1:-1, 2:]) - 2.0 * v) * rx + ((p[:-2, 1:-1] + p[2:, 1:-1]) - 2.0 * v) * ry
    if zero_outside:
        return full
    out = np.zeros_like(v)
    out[1:-1, 1:-1] = full[1:-1, 1:-1]
    return out


def laplacians(mesh, b):
    hx, hy = spacing(mesh)[:2]
    with np.errstate(all="ignore"):
        return np.array([stencil(b[c], hx, hy, False) for c in range(3)])


def sums(mesh, b, obs, lam=None):
    """S1 .. S11 (S9 with its factor hh) of b in the kernels' summation order, and Lambda"""
    (hx, hy), w, x, y = plane(mesh)
    X, Y = x[None, :], y[:, None]
    bx, by, bz = b
    with np.errstate(all="ignore"):                   # (a step far too large overflows, on the device too)
        if lam is None:
            lam = laplacians(mesh, b)
        e = (bz * bz - bx * bx) - by * by
        bb = (bx * bx + by * by) + bz * bz
        dx, dy, dz = bx - obs[0], by - obs[1], bz - obs[2]
        terms = [w * (bx * bz), w * (by * bz), w * e, w * (X * e), w * (Y * e),
                 w * ((Y * bx) * bz - (X * by) * bz), w * (dx * dx + dy * dy), w * (dz * dz),
                 (lam[0] * lam[0] + lam[1] * lam[1]) + lam[2] * lam[2], w * bb, w * (np.sqrt(X * X + Y * Y) * bb)]
        s = [kernel_sum(t) for t in terms]
        s[8] = (hx * hy) * s[8]
    return s, lam


def functional(mesh, s, mu, E, M):
    """(L, L1, L2, L3h, L3z, L4) from the sums"""
    hx, hy = spacing(mesh)[:2]
    hh = hx * hy
    with np.errstate(all="ignore"):
        l1 = np.float64((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]) / np.float64(E * E)
        l2 = np.float64((s[3] * s[3] + s[4] * s[4]) + s[5] * s[5]) / np.float64(M * M)
        l3h, l3z = np.float64(s[6]) / np.float64(E), np.float64(s[7]) / np.float64(E)
        l4 = np.float64((hh * hh) * s[8]) / np.float64(E)
        l = (((mu[0] * l1 + mu[1] * l2) + mu[2] * l3h) + mu[3] * l3z) + mu[4] * l4
    return tuple(float(v) for v in (l, l1, l2, l3h, l3z, l4))


def norms(mesh, obs):
    """E = S10 and M = S11 of the observation"""
    s, _ = sums(mesh, obs, obs)
    return s[9], s[10]


def value(mesh, b, obs, mu, E=None, M=None):
    """L of b alone"""
    if E is None:
        E, M = norms(mesh, obs)
    return functional(mesh, sums(mesh, b, obs)[0], mu, E, M)[0]


def gradient(mesh, b, obs, mu, s, lam, E, M, variant="full"):
    """G = dL/dB (3, ny, nx) at every node.  variant (tests of the formula only): "no_s6" drops the S6 terms,
    "flip_gy_x" flips the sign of the x-factor of G_y, "plain_laplacian" takes the stencil of B's Laplacian computed
    without zeroed edges in place of the transposed stencil of Lambda"""
    (hx, hy), w, x, y = plane(mesh)
    X, Y = x[None, :], y[:, None]
    hh = hx * hy
    bx, by, bz = b
    s1, s2, s3, s4, s5, s6 = (np.float64(v) for v in s[:6])
    E, M = np.float64(E), np.float64(M)
    with np.errstate(all="ignore"):
        a, bq = (2.0 * mu[0]) / (E * E), (2.0 * mu[1]) / (M * M)
        c3h, c3z = (2.0 * mu[2]) / E, (2.0 * mu[3]) / E
        c4 = ((2.0 * mu[4]) * ((hh * hh) * hh)) / E
        dx, dy, dz = bx - obs[0], by - obs[1], bz - obs[2]
        if variant == "plain_laplacian":
            t = [stencil(stencil(b[c], hx, hy, True), hx, hy, True) for c in range(3)]
        else:
            t = [stencil(lam[c], hx, hy, True) for c in range(3)]
        k6 = 0.0 if variant == "no_s6" else 1.0
        sg = -1.0 if variant == "flip_gy_x" else 1.0
        f1x = s1 * bz - (2.0 * s3) * bx
        f1y = s2 * bz - (2.0 * s3) * by
        f1z = (s1 * bx + s2 * by) + (2.0 * s3) * bz
        if variant == "full":
            f2x = ((((-2.0) * s4) * X) * bx - ((2.0 * s5) * Y) * bx) + (s6 * Y) * bz
            f2y = ((((-2.0) * s4) * X) * by - ((2.0 * s5) * Y) * by) - (s6 * X) * bz
            f2z = (((2.0 * s4) * X) * bz + ((2.0 * s5) * Y) * bz) + s6 * (Y * bx - X * by)
        else:
            f2x = ((((-2.0) * s4) * X) * bx - ((2.0 * s5) * Y) * bx) + k6 * ((s6 * Y) * bz)
            f2y = (sg * ((((-2.0) * s4) * X) * by) - ((2.0 * s5) * Y) * by) - sg * k6 * ((s6 * X) * bz)
            f2z = (((2.0 * s4) * X) * bz + ((2.0 * s5) * Y) * bz) + k6 * (s6 * (Y * bx - X * by))
        gx = w * ((a * f1x + bq * f2x) + c3h * dx) + c4 * t[0]
        gy = w * ((a * f1y + bq * f2y) + c3h * dy) + c4 * t[1]
        gz = w * ((a * f1z + bq * f2z) + c3z * dz) + c4 * t[2]
    return np.array([gx, gy, gz])


def trial(mesh, b, dt, g, E):
    hx, hy = spacing(mesh)[:2]
    with np.errstate(all="ignore"):
        step = np.float64(dt) * (np.float64(E) / (hx * hy))
        return b - step * g


def row_of(tries, f, dt, accepted, s):
    return [tries] + list(f) + [dt, accepted] + list(s[:6]) + [s[9], s[10]]


def run(mesh, b0, obs=None, mu=MU, niter_max=10000, check=50, tol=1e-4, dt0=None, dt_min=None, hist_rows=None):
    """(B, hist, info, accepted L values) of the driver, bit for bit; defaults as VecPot.preprocess"""
    b = np.array(b0, dtype=np.float64)
    obs = b.copy() if obs is None else np.array(obs, dtype=np.float64)
    mu = [float(v) for v in mu]
    if dt0 is None:
        dt0 = 0.01
    if dt_min is None:
        dt_min = 1e-6 * dt0
    if hist_rows is None:
        hist_rows = -(-niter_max // check) + 2
    dt = float(dt0)
    E, M = norms(mesh, obs)
    if not (E > 0.0 and M > 0.0):
        raise ValueError("the observation needs E > 0 and M > 0")
    s, lam = sums(mesh, b, obs)
    f = functional(mesh, s, mu, E, M)
    tries = accepted = 0
    trace = [f[0]]
    hist = np.zeros((hist_rows, ROW))
    hist[0] = row_of(tries, f, dt, accepted, s)
    rows = 1
    stop = 2 if dt < dt_min else 0
    flag = stop == 2
    lprev = f[0]
    done = 0
    while stop == 0 and done < niter_max:
        n = min(check, niter_max - done)
        for _ in range(n):
            if flag:
                break
            t = trial(mesh, b, dt, gradient(mesh, b, obs, mu, s, lam, E, M), E)
            st, lt = sums(mesh, t, obs)
            ft = functional(mesh, st, mu, E, M)
            tries += 1
            if ft[0] < f[0]:
                b, s, lam, f = t, st, lt, ft
                accepted += 1
                dt = dt * 1.01
                trace.append(f[0])
            else:
                dt = dt * 0.5
            flag = dt < dt_min
        done += n
        rows = min(rows + 1, hist_rows)
        hist[rows - 1] = row_of(tries, f, dt, accepted, s)
        if flag:
            stop = 2
        elif n == check:
            if lprev - f[0] <= tol * lprev:
                stop = 1
            lprev = f[0]
    return b, hist[:rows].copy(), (rows, tries, stop), trace


def balance(hist):
    """(eps_force, eps_torque) per history row"""
    h = np.asarray(hist, dtype=np.float64)
    a = np.abs(h[..., 9:15])
    return (a[..., 0] + a[..., 1] + a[..., 2]) / h[..., 15], (a[..., 3] + a[..., 4] + a[..., 5]) / h[..., 16]


# ---- the field of the tests --------------------------------------------------------------------------------------

def test_magnetogram(mesh, seed=27, noise=0.05):
    """(3, ny, nx): two submerged charges, scaled to max |component| = 1, seeded noise, then a shear that breaks the
    force balance: Bx += 0.2 Bz, By -= 0.1 Bz"""
    x, y = (np.asarray(q, dtype=np.float64) for q in mesh[:2])
    lx = x[-1] - x[0]
    xc, yc = x - 0.5 * (x[0] + x[-1]), y - 0.5 * (y[0] + y[-1])
    Y, X = np.meshgrid(yc, xc, indexing="ij")
    b = np.zeros((3,) + X.shape)
    for q, sx, sy, depth in ((1.0, -0.2 * lx, 0.03 * lx, 0.15 * lx), (-1.0, 0.2 * lx, -0.05 * lx, 0.18 * lx)):
        rx, ry, rz = X - sx, Y - sy, depth
        r3 = (rx * rx + ry * ry + rz * rz) ** 1.5
        b[0] += q * rx / r3
        b[1] += q * ry / r3
        b[2] += q * rz / r3
    b /= np.abs(b).max()
    b += noise * np.random.default_rng(seed).standard_normal(b.shape)
    b[0] += 0.2 * b[2]
    b[1] -= 0.1 * b[2]
    return b


test_magnetogram.__test__ = False      # (a field, not a test)
