"""CPU model of the 2-D solver's kernels, with the device's own summation orders.

TEST INFRASTRUCTURE - plain numpy; vcycle2d / solve2d also take the `port` oracle for the residual and the transfers.

relax_impl (csrc/smooth.hip) sends a 2-D level to one of three smoothers by its point count n = nx * ny:

  n <= SMALL_2D (4096)                     rbgs2_small   u and rhs in LDS
  SMALL_2D < n <= MEDIUM_2D (19456)        rbgs2_medium  u in LDS, a thread's first 8 points per colour in registers
  n > MEDIUM_2D, or variant 1 (the         rbgs2_color twice + launch_mean_shift (csrc/reduce.hip)
    host-driven coarsest-grid loop)

The sweep is the same expression everywhere (ndsm_poisson.f90:603-617, mirrored neighbours, (i + j) parity colours,
the even colour first) and is the oracle's relax_nd bit for bit.  What differs is the ORDER in which the mean of an
all-Neumann level - subtracted after every sweep - and the mean metric of the coarsest-grid solve are summed:

  wg_sum(v, 1024)    rbgs2_small, rbgs2_medium and the sweeps of tail.hip: thread t of 1024 adds v[t], v[t + 1024], ...
                     from 0.0, a shfl_down tree per 64-lane wave, the 16 wave partials added in index order from 0.0
  wg_sum(v, 256)     solve_exact_k (csrc/coarse.hip) and tail.hip's coarsest-grid solve: 256 threads, the four wave
                     partials folded as ((s0 + s1) + s2) + s3
  two_stage_sum(v)   sum_stage1 + mean_shift_k and diff_stage1 + diff_stage2 (reduce.hip): min(ceil(n / 256), 2048)
                     blocks of 256 grid-stride threads, a tree per wave, four wave partials added from the first;
                     then the block partials folded by 256 strided threads with the same tree

The oracle adds in index order.  All four orders are deterministic, so an all-Neumann result of the device can be
asserted bit for bit against this model (tests/test_gpu_2d.py), and test_model2d.py ties the model to the oracle.

Arrays are numpy C order (ny, nx) - (nz, ny, nx) for sweep3d; `bcs` is 2 * ndim letters, lower faces then upper.
"""
import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
SMALL_2D = 4096       # rbgs2_small's LDS arrays
MEDIUM_2D = 19456     # kMed2D of smooth.hip
EXACT_DEVICE = 2048   # kMaxPts of coarse.hip: above it ndsmk_solve_exact loops on the host
RED_BLOCK = 256       # kRedBlock of reduce.hip
RED_MAX_BLOCKS = 2048


def all_neumann(bcs):
    return set(bcs) == {"N"}


# ---------------------------------------------------------------------------------------------------------------------
# the sums
# ---------------------------------------------------------------------------------------------------------------------
def _strided(v, threads):
    """per-thread partial sums: thread t adds v[t], v[t + threads], ... in that order, starting from 0.0
    (zero padding is exact: a sum that started at +0.0 is never -0.0, and x + 0.0 == x otherwise)"""
    v = np.asarray(v, dtype=np.float64).ravel()
    rows = max(1, -(-v.size // threads))
    p = np.zeros(rows * threads)
    p[:v.size] = v
    acc = np.zeros(threads)
    for row in p.reshape(rows, threads):
        acc = acc + row
    return acc


def _wave_tree(acc):
    """lane 0 of every 64-lane wave after `for o in 32..1: v += shfl_down(v, o)`; all lanes read before any writes"""
    w = acc.reshape(-1, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        w[:, :64 - o] = w[:, :64 - o] + w[:, o:]
    return w[:, 0]


def wg_sum(v, threads=1024):
    """sum of v in the order of a single workgroup of `threads` threads (1024: rbgs2_small / rbgs2_medium / tail.hip's
    mean_shift, the wave partials added to 0.0 in index order; 256: solve_exact_k's block_sum, ((s0 + s1) + s2) + s3)"""
    assert threads % 64 == 0
    part = _wave_tree(_strided(v, threads))
    if threads == 256:
        return float(((part[0] + part[1]) + part[2]) + part[3])
    tot = 0.0
    for s in part:
        tot = tot + float(s)
    return tot


def two_stage_sum(v):
    """sum of v in the order of reduce.hip's two-stage reductions"""
    v = np.asarray(v, dtype=np.float64).ravel()
    nb = max(1, min(-(-v.size // RED_BLOCK), RED_MAX_BLOCKS))
    waves = _wave_tree(_strided(v, nb * RED_BLOCK)).reshape(nb, RED_BLOCK // 64)      # thread b * 256 + t of the grid
    part = waves[:, 0]
    for w in range(1, RED_BLOCK // 64):
        part = part + waves[:, w]
    fold = _wave_tree(_strided(part, RED_BLOCK))
    s = fold[0]
    for w in range(1, RED_BLOCK // 64):
        s = s + fold[w]
    return float(s)


def serial_sum(v):
    """the oracle's order: one accumulator, index order"""
    return float(np.add.accumulate(np.asarray(v, dtype=np.float64).ravel())[-1])


def mean_order(n, variant=0):
    """the sum that forms the mean of an all-Neumann 2-D level of n points in ndsmk_relax(..., variant)"""
    return wg_sum if (variant == 0 and n <= MEDIUM_2D) else two_stage_sum


UNIT = 2.0 ** -53     # unit roundoff of float64


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of k chained roundings"""
    return k * UNIT / (1.0 - k * UNIT)


def neumann_bound(v, n):
    """Bound on |model - oracle| after one all-Neumann sweep.  Both start from the same swept field v (the sweep is
    bit-identical) and differ only in the order in which sum(v) is added up.
      * A sum of n numbers that starts from 0.0, in ANY order, is off by at most gamma_{n-1} sum|v| (n - 1 rounded
        additions on the longest chain; Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), so two
        orders differ by at most 2 gamma_{n-1} sum|v| and the two means by that over n: 2 gamma_{n-1} mean|v|.
      * The division by n and the subtraction v - m each round once more.  The subtraction's rounding is at most
        2^-53 |v - m| per side; the tree orders' own chains are far shorter than n - 1 (at most 19 + 6 + 16 additions),
        which leaves the first term more than enough room for the second side and for the division's 2^-53 |m|.
    Hence |du| <= 2 gamma_{n-1} mean|u| + 2^-53 max|u|, taken on the result."""
    return 2.0 * gamma(n - 1) * float(np.abs(v).mean()) + UNIT * float(np.abs(v).max())



# ---------------------------------------------------------------------------------------------------------------------
# the sweeps
# ---------------------------------------------------------------------------------------------------------------------
def _mirror(n):
    """stencil_stride (ndsm_poisson.f90:633-658): both neighbours collapse onto the inner one at a boundary"""
    i = np.arange(n)
    lo = np.where(i == 0, 1, np.where(i == n - 1, n - 2, i - 1))
    hi = np.where(i == 0, 1, np.where(i == n - 1, n - 2, i + 1))
    return lo, hi


def _updated(shape, bcs):
    """points a sweep updates: everything but the Dirichlet faces; shape (.., ny, nx), bcs lower x, y(, z) then upper"""
    nd = len(shape)
    m = np.ones(shape, dtype=bool)
    for d in range(nd):
        ax = nd - 1 - d
        idx = np.arange(shape[ax]).reshape([-1 if a == ax else 1 for a in range(nd)])
        if bcs[d] == "D":
            m = m & (idx != 0)
        if bcs[nd + d] == "D":
            m = m & (idx != shape[ax] - 1)
    return m


def weights2d(mesh):
    """w_d = 1 / (dq_d dq_d) and w1 = 1 / (0 + 2 w_x + 2 w_y), in the oracle's order (ndsm_poisson.f90:483-489)"""
    wx, wy = (1.0 / ((float(q[1]) - float(q[0])) * (float(q[1]) - float(q[0]))) for q in mesh[:2])
    w0 = 0.0
    w0 = w0 + 2.0 * wx
    w0 = w0 + 2.0 * wy
    return wx, wy, 1.0 / w0


def sweep2d(u, rhs, mesh, bcs):
    """the two colour passes of one sweep, without the mean (rhs None: zero)"""
    u = np.array(u, dtype=np.float64)
    ny, nx = u.shape
    rhs = np.zeros_like(u) if rhs is None else np.asarray(rhs, dtype=np.float64)
    wx, wy, w1 = weights2d(mesh)
    xl, xh = _mirror(nx)
    yl, yh = _mirror(ny)
    j, i = np.ogrid[:ny, :nx]
    colour = (i + j) & 1
    upd = _updated(u.shape, bcs)
    for par in (0, 1):
        un = np.zeros_like(u)
        un = un + u[:, xl] * wx + u[:, xh] * wx
        un = un + u[yl, :] * wy + u[yh, :] * wy
        u = np.where(upd & (colour == par), (un - rhs) * w1, u)
    return u


def sweep3d(u, rhs, mesh, bcs):
    """one sweep of red_black_gauss_3D without the mean (ndsm_optimized.f90:106-139) - for the 3-D coarsest-grid cases"""
    u = np.array(u, dtype=np.float64)
    nz, ny, nx = u.shape
    rhs = np.zeros_like(u) if rhs is None else np.asarray(rhs, dtype=np.float64)
    hx, hy, hz = (float(q[1]) - float(q[0]) for q in mesh[:3])
    wx, wy, wz = 1.0 / (hx * hx), 1.0 / (hy * hy), 1.0 / (hz * hz)
    w1 = 1.0 / (2 * (wx + wy + wz))

    def nb(n):     # only the out-of-range neighbour is mirrored here
        i = np.arange(n)
        return np.where(i - 1 < 0, 1, i - 1), np.where(i + 1 > n - 1, n - 2, i + 1)

    (xl, xh), (yl, yh), (zl, zh) = nb(nx), nb(ny), nb(nz)
    k, j, i = np.ogrid[:nz, :ny, :nx]
    colour = (i + j + k) & 1
    upd = _updated(u.shape, bcs)
    first = 1 if bcs[0] == "D" else 0
    for p in (0, 1):
        new = w1 * ((u[:, :, xh] + u[:, :, xl]) * wx + (u[:, yh, :] + u[:, yl, :]) * wy + (u[zh] + u[zl]) * wz - rhs)
        u = np.where(upd & (colour == ((first + p) & 1)), new, u)
    return u


def shift_mean(u, total):
    return u - total / float(u.size)


def relax2d(u, rhs, mesh, bcs, nsweeps=1, variant=0, order=None):
    """ndsmk_relax on a 2-D level: nsweeps sweeps, on all-Neumann sets each followed by u - sum / float(n) with the sum
    in the order of the level's size class and variant (`order` overrides it: serial_sum gives the oracle)"""
    u = np.array(u, dtype=np.float64)
    order = order or mean_order(u.size, variant)
    for _ in range(nsweeps):
        u = sweep2d(u, rhs, mesh, bcs)
        if all_neumann(bcs):
            u = shift_mean(u, order(u))
    return u


# ---------------------------------------------------------------------------------------------------------------------
# the coarsest-grid solve
# ---------------------------------------------------------------------------------------------------------------------
def exact_loop(u, sweep, alln, ex_tol, use_max, nmax, order=None):
    """solve_exact (ndsm_multigrid_core.f90:728-800) around `sweep` (one sweep without the mean): u_sav = 0; the test
    du <= ex_tol comes first, then the sweep (+ mean shift), then du = max or mean of |u_sav - u|.  Up to EXACT_DEVICE
    points the sums are solve_exact_k's, above it the host loop's (variant-1 sweeps and ndsmk_diff_metrics).
    (`order` overrides both: serial_sum gives the oracle.)  Returns u, the sweep count, the converged flag and the
    list of du."""
    u = np.array(u, dtype=np.float64)
    n = u.size
    tot = order or ((lambda v: wg_sum(v, 256)) if n <= EXACT_DEVICE else two_stage_sum)
    sav, du, dus, conv = np.zeros_like(u), DBL_MAX, [], False
    for _ in range(nmax):
        if du <= ex_tol:
            conv = True
            break
        u = sweep(u)
        if alln:
            u = shift_mean(u, tot(u))
        d = np.abs(sav - u)
        du = float(d.max()) if use_max else tot(d) / float(n)
        dus.append(du)
        sav = u.copy()
    return u, len(dus), conv, dus


def exact2d(u, rhs, mesh, bcs, ex_tol=1e-13, use_max=True, nmax=10000, order=None):
    return exact_loop(u, lambda v: sweep2d(v, rhs, mesh, bcs), all_neumann(bcs), ex_tol, use_max, nmax, order)


def exact3d(u, rhs, mesh, bcs, ex_tol=1e-13, use_max=True, nmax=10000, order=None):
    return exact_loop(u, lambda v: sweep3d(v, rhs, mesh, bcs), all_neumann(bcs), ex_tol, use_max, nmax, order)


# ---------------------------------------------------------------------------------------------------------------------
# the V-cycle and the solve
# ---------------------------------------------------------------------------------------------------------------------
def vcycle2d(port, u, rhs, mesh, bcs, ms=5, ex_tol=1e-13, du_max=True, nmax_exact=10000, ngrids=None, order=None):
    """one V-cycle (ndsm_oracle.c: fine_to_coarse, solve_exact, coarse_to_fine) of the hierarchy rooted at u's shape.
    Returns (levels, sweeps, unconverged): levels[l - 1] = (u, rhs) of level l as the device leaves them, the
    coarsest-grid sweep count and 0 / 1 for a coarsest-grid solve that ran out of sweeps.
    The sums do not depend on whether levels run inside tail.hip's single launch: its sweeps sum as rbgs2_small (and
    rbgs2_medium: the same order) and its coarsest-grid solve as solve_exact_k, which its gate holds to EXACT_DEVICE.
    (`order` overrides every sum: serial_sum gives the oracle.)"""
    u = np.array(u, dtype=np.float64)
    ns = list(u.shape[::-1])
    shapes, meshes = port.hierarchy(ns, mesh, ngrids)
    ng = len(shapes)
    U, R = {1: u}, {1: np.zeros_like(u) if rhs is None else np.asarray(rhs, dtype=np.float64)}
    for l in range(1, ng):                                          # fine_to_coarse
        U[l] = relax2d(U[l], R[l], meshes[l - 1], bcs, ms, 0, order)
        R[l + 1] = port.restrict(port.residual_nd(U[l], R[l], meshes[l - 1], bcs), ns, mesh, l, ngrids)
        U[l + 1] = np.zeros_like(R[l + 1])
    U[ng], sweeps, conv, _dus = exact2d(U[ng], R[ng], meshes[ng - 1], bcs, ex_tol, du_max, nmax_exact, order)
    for lc in range(ng, 1, -1):                                     # coarse_to_fine
        U[lc] = relax2d(U[lc], R[lc], meshes[lc - 1], bcs, ms, 0, order)
        U[lc - 1] = U[lc - 1] + port.interp(U[lc], ns, mesh, lc - 1, ngrids)
        U[lc - 1] = relax2d(U[lc - 1], R[lc - 1], meshes[lc - 2], bcs, ms, 0, order)
    return [(U[l], R[l]) for l in range(1, ng + 1)], sweeps, 0 if conv else 1


def solve2d(port, u, rhs, mesh, bcs, ms=5, ex_tol=1e-13, du_max=True, nmax_exact=10000, vc_tol=1e-10, nmax=1024,
            ngrids=None, order=None):
    """solve_bvp: V-cycles until du < vc_tol (strict), the first du against the caller's array; the level-1 metric is
    ndsmk_diff_metrics (max, or two_stage_sum / n; `order` overrides every sum).  Returns (ierr, u, du_last, hist, ncycles, sweeps, unconverged)."""
    u = np.array(u, dtype=np.float64)
    du, hist, ierr, sweeps, unconv = DBL_MAX, [], 1, 0, 0
    for _ in range(nmax):
        prev = u
        levels, sw, un = vcycle2d(port, u, rhs, mesh, bcs, ms, ex_tol, du_max, nmax_exact, ngrids, order)
        u = levels[0][0]
        sweeps, unconv = sweeps + sw, unconv + un
        d = np.abs(u - prev)
        du = float(d.max()) if du_max else (order or two_stage_sum)(d) / float(u.size)
        hist.append(du)
        if du < vc_tol:
            ierr = 0
            break
    return ierr, u, du, hist, len(hist), sweeps, unconv


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_2d.py (kept here so that test_model2d.py can check the model on them without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
SHAPES_2D = (
    [64, 64],      # 4096 points: the last rbgs2_small level
    [8, 512],      # 4096, thin
    [64, 65],      # 4160: the first rbgs2_medium level
    [8, 513],      # 4104, thin
    [128, 128],    # 16384: a DDDD colour is under 8192 points, an NNNN colour exactly 8192 (registers only)
    [129, 127],    # 16383, odd nx
    [139, 139],    # 19321: 9730 points per colour, rbgs2_medium's trailing loop runs
    [152, 128],    # 19456 = kMed2D: the last rbgs2_medium level
    [8, 2432],     # 19456, thin: j up to 2431 in the packed coordinate
    [141, 138],    # 19458: the first level of rbgs2_color + launch_mean_shift
    [300, 260],    # 78000: levels of 19500 / 4875 / 1184 / ... points cross every class on the way down
    [9, 500],      # 4500, thin, two-level hierarchy
)
ANISO_2D = ([129, 127], [139, 139], [300, 260])
BCS_2D = ("NNNN", "DNND", "NDDN", "DDDD", "NNND")
VCYCLE_SHAPES = ([300, 260], [139, 139], [141, 138], [64, 65], [9, 500])

# coarsest-grid solves: (root shape, ngrids, solved level); the solved level is the root's last
EXACT_ROOTS = (
    ([90, 80], 2, 2),          # [45, 40]: 1800 points, solve_exact_k
    ([64, 128], 2, 2),         # [32, 64]: 2048 points, solve_exact_k's limit
    ([150, 140], 2, 2),        # [75, 70]: 5250 points, the host loop
    ([24, 22, 26], 2, 2),      # [12, 11, 13]: 1716 points, solve_exact_k's 3-D branch
    ([40, 36, 34], 2, 2),      # [20, 18, 17]: 6120 points, the host loop over rbgs3_color
)
EXACT_BCS = {2: ("DNND", "NNNN", "DDDD"), 3: ("NDDNDD", "NNNNNN", "DDNDDN")}
# (ex_tol, max metric?, nmax_exact): the last two run out of sweeps
EXACT_OPTIONS = ((1e-2, True, 10000), (1e-2, False, 10000), (1e-3, True, 12), (0.0, False, 5))
# coarsest-grid options of the V-cycle and solve cases: the 4 x 4 coarsest grids converge within the cap, the 4 x 250
# one of [9, 500] runs out of sweeps in every cycle (the unconverged counter)
VCYCLE_KW = dict(ex_tol=1e-13, nmax_exact=60)
