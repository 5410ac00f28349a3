"""Seeded input generators shared by the tests and tests/golden/make_golden.py.

The golden files hold only the reference's OUTPUTS; the matching inputs are
re-created here from fixed seeds (numpy default_rng,
seeds 2112 / 2113, U(-1,1)).
"""
import itertools

import numpy as np

# BC letter sets of the three vector-potential components, lower x,y,z then
# upper x,y,z (ndsm_vector_potential.f90:655,671,687)
BCS3 = ("NDDNDD", "DNDDND", "DDNDDN")

KERNEL_SHAPES_3D = ([22, 22, 22], [33, 22, 27])   # Fortran order [nx, ny, nz]
KERNEL_SHAPES_2D = ([27, 36], [22, 22])


def rand_field(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape)


def uniform_mesh(nshape):
    """x = linspace(0,1,nx); y,z = arange(n)*dx  (tests/integration_test/integration_test1.py:124-127)."""
    x = np.linspace(0.0, 1.0, int(nshape[0]))
    dx = x[1] - x[0]
    return [x] + [np.arange(int(n)) * dx for n in nshape[1:]]


# spacing of each axis relative to h_x = 1/(nx-1), and the first mesh point of each axis: neither ratio is 1 or a
# power of two, and all stay close enough to 1 for point Gauss-Seidel multigrid to converge within the defaults
ANISO_RATIOS = (1.0, 0.73, 1.37)
ANISO_ORIGINS = (0.25, -0.4, 1.1)
ANISO_SHAPES_3D = ([33, 22, 27], [24, 30, 20])
ANISO_SHAPE_2D = [27, 36]
ANISO_PIPELINE_SHAPE = [20, 17, 23]
BCS_ANISO = BCS3 + ("DDDDDD", "NDNDND")


def aniso_mesh(nshape):
    """a distinct spacing on every axis and no origin at 0: q_d = o_d + arange(n_d) * r_d h_x with h_x = 1/(nx-1)
    (ANISO_RATIOS, ANISO_ORIGINS); a 2-D shape takes the first two axes"""
    h = 1.0 / (int(nshape[0]) - 1)
    return [o + np.arange(int(n)) * (r * h) for n, r, o in zip(nshape, ANISO_RATIOS, ANISO_ORIGINS)]


def analytic_field(mesh):
    """analytic_case's current-free field and its potential at the points of `mesh` ([x, y, z], any spacings and
    origins).  Returns A, b shaped (3, nz, ny, nx)."""
    Z, Y, X = np.meshgrid(mesh[2], mesh[1], mesh[0], indexing="ij")
    wn = np.pi
    l = np.sqrt(2 * wn ** 2)
    b = np.zeros((3,) + X.shape)
    A = np.zeros((3,) + X.shape)
    b[0] = +l * np.sin(wn * X) * np.cos(wn * Y) * np.exp(-l * Z)
    b[1] = +l * np.cos(wn * X) * np.sin(wn * Y) * np.exp(-l * Z)
    b[2] = +2 * wn * np.cos(wn * X) * np.cos(wn * Y) * np.exp(-l * Z)
    A[0] = -np.cos(wn * X) * np.sin(wn * Y) * np.exp(-l * Z)
    A[1] = +np.sin(wn * X) * np.cos(wn * Y) * np.exp(-l * Z)
    return A, b


def aniso_pipeline_cases():
    """(name, x, y, z, b) of the anisotropic pipeline fixtures: the analytic field on aniso_mesh, and the same field
    plus seeded noise that unbalances the face fluxes"""
    x, y, z = aniso_mesh(ANISO_PIPELINE_SHAPE)
    _A, b = analytic_field([x, y, z])
    yield "analytic", x, y, z, b
    noise = np.random.default_rng(2114).uniform(-1.0, 1.0, b.shape)
    yield "unbalanced", x, y, z, b + 0.2 * np.abs(b).max() * noise


def manufactured_poisson(mesh, bcs):
    """u* = prod_d (cos|sin)(pi q_d / L_d): cos on the Neumann axis, sin on
    Dirichlet axes; rhs = laplace(u*).  Returned in numpy order (nz, ny, nx)."""
    nd = len(mesh)
    grids = np.meshgrid(*mesh[::-1], indexing="ij")[::-1]  # X, Y, Z each (nz,ny,nx)
    u = np.ones_like(grids[0])
    lam = 0.0
    for d in range(nd):
        L = mesh[d][-1] - mesh[d][0]
        k = np.pi / L
        if bcs[d] == "N":
            assert bcs[nd + d] == "N"
            u = u * np.cos(k * (grids[d] - mesh[d][0]))
        else:
            u = u * np.sin(k * (grids[d] - mesh[d][0]))
        lam += k * k
    return u, -lam * u


def analytic_case(n):
    """Current-free test field of tests/integration_test/integration_test1.py:57-99
    (k = pi, l = sqrt(2) pi) on x = linspace(0,1,nx), equal spacing in y, z.
    `n` is an int (cube) or Fortran-order [nx, ny, nz].  Returns x, y, z, A, b
    with A, b shaped (3, nz, ny, nx)."""
    ns = [n, n, n] if np.isscalar(n) else list(n)
    x, y, z = uniform_mesh(ns)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    wn = np.pi
    l = np.sqrt(2 * wn ** 2)
    b = np.zeros((3,) + X.shape)
    A = np.zeros((3,) + X.shape)
    b[0] = +l * np.sin(wn * X) * np.cos(wn * Y) * np.exp(-l * Z)
    b[1] = +l * np.cos(wn * X) * np.sin(wn * Y) * np.exp(-l * Z)
    b[2] = +2 * wn * np.cos(wn * X) * np.cos(wn * Y) * np.exp(-l * Z)
    A[0] = -np.cos(wn * X) * np.sin(wn * Y) * np.exp(-l * Z)
    A[1] = +np.sin(wn * X) * np.cos(wn * Y) * np.exp(-l * Z)
    return x, y, z, A, b


# BC sets of test_oracle.py::test_live_reference_random: the three components' plus the all-Neumann,
# all-Dirichlet and mixed corners
BCS_RANDOM = BCS3 + ("NNNNNN", "DDDDDD", "NDNDND")


def random_reference_cases():
    """(ns, mesh, u, rhs) of test_oracle.py::test_live_reference_random: two odd-sized boxes, fields drawn in
    this order from one default_rng(12345)."""
    rng = np.random.default_rng(12345)
    for ns in ([17, 23, 19], [40, 24, 32]):
        shp = tuple(ns[::-1])
        u, rhs = rng.uniform(-1, 1, shp), rng.uniform(-1, 1, shp)
        yield ns, uniform_mesh(ns), u, rhs


def aniso_case(nshape):
    """(mesh, u, rhs) of the anisotropic per-operator fixtures: aniso_mesh and the seeds of the uniform-mesh ones"""
    shp = tuple(int(n) for n in nshape[::-1])
    return aniso_mesh(nshape), rand_field(shp, 2112), rand_field(shp, 2113)


def quirk_case(n=24):
    """analytic field with B.n = 0 on the top face: its 2-D solve (the LAST one) converges at once,
    the 3-D solves cannot within 2 V-cycles"""
    x, y, z, A1, b1 = analytic_case(n)
    b = b1.copy()
    b[2, -1, :, :] = 0.0
    return x, y, z, b


def digest(a):
    """sha256 of an array's float64 bytes (C order, little-endian): equal digests <=> bit-identical arrays"""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).hexdigest()


# ---- edge values of the solver options (tests/golden/reference_options.json, test_oracle.py, test_gpu_options.py) ----
OPTION_PIPELINE_SHAPE = [24, 20, 18]
OPTION_MS = (0, 1, 6, 7, 11)            # 2 ms post-smoothing sweeps: 0, 2, 12, 14, 22
OPTION_NCYC = (0, 1, 3)
OPTION_NEX = (0, 1, 10000)
OPTION_SCALAR_3D = [17, 23, 19]
OPTION_SCALAR_2D = [27, 36]
HUGE = float(np.finfo(np.float64).max)  # du_last of a solve that ran no V-cycle (Fortran HUGE)


def noisy_case(ns):
    """analytic_case plus seeded noise, so that all three component solves iterate: x, y, z, b"""
    x, y, z, _A1, b1 = analytic_case(ns)
    return x, y, z, b1 + 0.05 * np.random.default_rng(5).standard_normal(b1.shape)


def option_matrix():
    """the full product (ms, ncycles, nmaxex, mean) of the edge values: 90 tuples"""
    return [(ms, nc, nex, mean) for ms in OPTION_MS for nc in OPTION_NCYC for nex in OPTION_NEX
            for mean in (False, True)]


def pipeline_option_cases():
    """keyword sets of vector_potential for the option matrix on noisy_case: the product, then zero tolerances and
    loose ones with the mean metric (93)"""
    kws = [dict(ms=ms, ncycles_max=nc, niterex_max=nex, mean=mean) for ms, nc, nex, mean in option_matrix()]
    kws.append(dict(ms=5, ncycles_max=3, vc_tol=0.0))
    kws.append(dict(ncycles_max=40, niterex_max=50, ex_tol=0.0, mean=True))
    kws.append(dict(ms=2, ncycles_max=5, niterex_max=2, vc_tol=1e-3, ex_tol=1e-2, mean=True))
    return kws


def negative_option_cases():
    """keyword sets with negative (and one NaN) option values: the reference takes a negative count as 0"""
    return [dict(ms=-1, ncycles_max=3), dict(ncycles_max=-2), dict(niterex_max=-3, ncycles_max=3),
            dict(vc_tol=-1.0, ncycles_max=3), dict(ex_tol=-1.0, ncycles_max=3, niterex_max=50),
            dict(vc_tol=float("nan"), ncycles_max=3),
            dict(ms=-1, ncycles_max=-2, niterex_max=-3, vc_tol=-1.0, ex_tol=-1.0)]


def zero_field_cases():
    """keyword sets for an all-zero field: du = 0 < vc_tol is strict, so vc_tol = 0 never converges"""
    return [dict(vc_tol=0.0, ncycles_max=3), dict(vc_tol=1e-10, ncycles_max=3)]


def scalar_option_problems():
    """(name, ns, mesh, bcs, u, rhs) of the scalar-solve option matrix: 17x23x19 and 27x36 (2-D), uniform and
    aniso_mesh, the three component sets plus all-Neumann (rhs made compatible by subtracting its mean)"""
    for ns, bcsets in ((OPTION_SCALAR_3D, BCS3 + ("NNNNNN",)), (OPTION_SCALAR_2D, ("NNNN", "DNND"))):
        shp = tuple(ns[::-1])
        u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
        for mname, meshf in (("uniform", uniform_mesh), ("aniso", aniso_mesh)):
            for bcs in bcsets:
                r = rhs - rhs.mean() if set(bcs) == {"N"} else rhs
                yield "%s_%s_%s" % ("x".join(str(n) for n in ns), mname, bcs), ns, meshf(ns), bcs, u, r


def scalar_kw(ms, nc, nex, mean):
    """option_matrix tuple -> keywords of Oracle.solve_bvp"""
    return dict(ms=ms, nmax=nc, nmax_exact=nex, du_max=not mean)


# ---- every boundary letter set (tests/golden/reference_bc_matrix.json, test_oracle_bc_matrix.py, test_gpu_bc_matrix.py) ----
ALL_BCS_3D = tuple("".join(p) for p in itertools.product("DN", repeat=6))   # 64, "DDDDDD" first, "NNNNNN" last
ALL_BCS_2D = tuple("".join(p) for p in itertools.product("DN", repeat=4))   # 16
# (shape, mesh function name) of the matrix: odd nx on aniso_mesh, even nx on uniform_mesh; inputs rand_field 2112 / 2113
BC_MATRIX_3D = (([17, 12, 9], "aniso"), ([18, 17, 17], "uniform"))
BC_MATRIX_2D = (([27, 36], "aniso"), ([22, 22], "uniform"))
BC_MATRIX_SEEDS = (2112, 2113)          # u, rhs

_AXIS_PAIRS = ("DD", "DN", "ND", "NN")  # (lower, upper) letters of one axis, coded 0 ... 3


def bc_orthogonal_array():
    """16 of the 64 sets, a strength-2 orthogonal array: x, y in 0 ... 3 and z = (x + y) mod 4, so that every pair of
    axes sees all 16 combinations of (lower, upper) letters.  Holds DDDDDD; NNNNNN is not a member (x = y = 3, z = 2)."""
    out = []
    for x in range(4):
        for y in range(4):
            p = (_AXIS_PAIRS[x], _AXIS_PAIRS[y], _AXIS_PAIRS[(x + y) % 4])
            out.append("".join(q[0] for q in p) + "".join(q[1] for q in p))
    return tuple(out)


def bc_matrix_case(ns, mesh_name):
    """(mesh, u, rhs) of one shape of the boundary-set matrix"""
    shp = tuple(int(n) for n in ns[::-1])
    mesh = aniso_mesh(ns) if mesh_name == "aniso" else uniform_mesh(ns)
    return mesh, rand_field(shp, BC_MATRIX_SEEDS[0]), rand_field(shp, BC_MATRIX_SEEDS[1])


def digest16(a):
    """the first 16 hex digits of digest(a): 64 bits tell bit-identical arrays apart and keep the fixtures small"""
    return digest(a)[:16]
