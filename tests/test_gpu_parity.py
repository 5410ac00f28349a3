"""GPU parity tests (run with -m gpu on an MI355X).

Everything goes through the C ABI of libndsm_hip.so (include/ndsm_hip.h):
either the reference's own entry point `ndsm_vector_solve` via
ndsm_amd.vector_potential, or the additive solver-handle API.  The checker is
the oracle (oracle/ndsm_oracle.c, pinned to the reference by test_oracle.py)
and the committed golden vectors produced by the reference itself.

Tolerances (fp64):
  * 3-D smoother, residual, restriction, prolongation, V-cycle, du history:
    BIT-IDENTICAL.  The kernels keep the reference's operand order and are
    compiled with -ffp-contract=off; max|.| is order independent.
  * anything containing the all-Neumann mean shift (2-D face solves, hence the
    full pipeline): the reference's own summation order is unspecified (OpenMP
    reduction), so |dA| <= 1e-12 max|A| and |dB| <= 1e-12 max|A| * 4/h, the
    bound SURVEY 8c derives from the reference's own thread-count spread.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from golden_inputs import (BCS3, KERNEL_SHAPES_2D, KERNEL_SHAPES_3D, analytic_case, aniso_mesh, manufactured_poisson,
                           rand_field, uniform_mesh)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def _tag(ns):
    return "x".join(str(n) for n in ns)


def _meshes(uniform, aniso=(), ids=_tag):
    """(ns, mesh function) cases: the shapes on uniform_mesh under the ids they always had, and the `aniso` shapes on
    golden_inputs.aniso_mesh (a spacing of its own on every axis, no origin at 0) under 'aniso-' ids"""
    return ([pytest.param(ns, uniform_mesh, id=ids(ns)) for ns in uniform] +
            [pytest.param(ns, aniso_mesh, id="aniso-" + ids(ns)) for ns in aniso])


def _pad_r(solver, arr):
    """place a level-l array at the start of the level-1 sized residual scratch"""
    full = np.zeros(solver._npshape(1))
    full.ravel()[:arr.size] = arr.ravel()
    return full


SHAPES_3D = KERNEL_SHAPES_3D + ([17, 23, 19], [40, 24, 32], [64, 64, 64])
ANISO_3D = ([33, 22, 27], [17, 23, 19], [40, 24, 32])       # odd and even nx


@pytest.mark.parametrize("ns,meshf", _meshes(SHAPES_3D, ANISO_3D))
def test_kernels3d_bitwise(hip, port, ns, meshf):
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    for bcs in BCS3 + ("DDDDDD", "NDNDND"):
        S = hip.MGSolver(ns, mesh, bcs)
        shapes, _ = port.hierarchy(ns, mesh)
        assert [tuple(int(v) for v in s) for s in shapes] == S.shapes
        # smoother: 1 and 3 sweeps
        S.upload(1, hip.BUF_U, u)
        S.upload(1, hip.BUF_RHS, rhs)
        S.op(hip.OP_RELAX_COLOR, 1, 1)
        want = port.relax3d(u, rhs, mesh, bcs)
        assert np.array_equal(S.download(1, hip.BUF_U), want), f"relax {bcs}"
        S.op(hip.OP_RELAX_COLOR, 1, 2)
        want = port.relax3d(port.relax3d(want, rhs, mesh, bcs), rhs, mesh, bcs)
        assert np.array_equal(S.download(1, hip.BUF_U), want), f"relax x3 {bcs}"
        # default variant (fused where available) must give the same bits
        S.upload(1, hip.BUF_U, u)
        S.op(hip.OP_RELAX, 1, 3)
        assert np.array_equal(S.download(1, hip.BUF_U), want), f"relax default x3 {bcs}"
        # residual
        S.upload(1, hip.BUF_U, u)
        S.op(hip.OP_RESIDUAL, 1)
        assert np.array_equal(S.download(1, hip.BUF_R), port.residual3d(u, rhs, mesh, bcs)), f"residual {bcs}"
        # one V-cycle
        S.upload(1, hip.BUF_U, u)
        S.vcycle(1)
        assert np.array_equal(S.download(1, hip.BUF_U), port.vcycle(u, rhs, mesh, bcs)), f"vcycle {bcs}"
        S.close()


@pytest.mark.parametrize("ns,meshf", _meshes(SHAPES_3D, ANISO_3D))
def test_transfer3d_bitwise(hip, port, ns, meshf):
    mesh = meshf(ns)
    S = hip.MGSolver(ns, mesh, "NDDNDD")
    shapes, _ = port.hierarchy(ns, mesh)
    for lvl in range(1, len(shapes)):
        f = rand_field(tuple(int(v) for v in shapes[lvl - 1][::-1]), 3000 + lvl)
        c = rand_field(tuple(int(v) for v in shapes[lvl][::-1]), 4000 + lvl)
        S.upload(1, hip.BUF_R, _pad_r(S, f))
        S.upload(lvl + 1, hip.BUF_U, c)                      # must be zeroed by restrict
        S.op(hip.OP_RESTRICT, lvl)
        assert np.array_equal(S.download(lvl + 1, hip.BUF_RHS), port.restrict(f, ns, mesh, lvl)), f"restrict {lvl}"
        assert not S.download(lvl + 1, hip.BUF_U).any()
        S.upload(lvl + 1, hip.BUF_U, c)
        S.upload(lvl, hip.BUF_U, np.zeros_like(f))
        S.op(hip.OP_PROLONG, lvl)
        assert np.array_equal(S.download(lvl, hip.BUF_U), port.interp(c, ns, mesh, lvl)), f"interp {lvl}"
        S.upload(lvl, hip.BUF_U, f)                          # u += P c on a non-zero u
        S.op(hip.OP_PROLONG, lvl)
        assert np.array_equal(S.download(lvl, hip.BUF_U), f + port.interp(c, ns, mesh, lvl))
    S.close()


# the restriction each shape of test_large_level_kernels_bitwise takes by itself: 0 the gather kernel (under 6 Mi points),
# 10 / 8 the streamed one's DMA / register-staged form (odd nx); all five take the tiled prolongation
LARGE_LEVEL_FORMS = {(128, 128, 128): 0, (200, 100, 120): 0, (256, 192, 160): 10, (129, 128, 130): 0, (257, 161, 158): 8}


@pytest.mark.parametrize("ns,meshf", _meshes(([128, 128, 128], [200, 100, 120], [256, 192, 160], [129, 128, 130], [257, 161, 158]),
                                             ([200, 100, 120], [257, 161, 158])))
def test_large_level_kernels_bitwise(hip, port, ns, meshf):
    """the kernels that only serve large levels against the oracle, level 1 -> 2, at their own sizes: the temporally
    blocked fused smoother (odd nx: its ghost-column variant) and the LDS-tiled prolongation (from 2 Mi points) at all
    five shapes; the LDS-streamed restriction (from 6 Mi points) at 256x192x160 - its DMA form - and 257x161x158 - odd
    nx: its register-staged, scheduled form.  128^3, 200x100x120 and 129x128x130 have 2.1-2.4 Mi points: their
    restriction is the gather kernel.  Which form runs is asserted from ndsm_hip_debug_transfer_form, not assumed; the
    streamed forms at their edges are test_gpu_transfer_matrix.py's."""
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    bcs = "DNDDND"
    S = hip.MGSolver(ns, mesh, bcs)
    form, kc, nkc, tiled = S.transfer_form(1)
    assert (form, tiled) == (LARGE_LEVEL_FORMS[tuple(ns)], 1), (ns, form, tiled)
    assert (kc >= 1 and nkc == -(-(ns[2] // 2) // kc)) if form else (kc, nkc) == (0, 0)
    shapes, _ = port.hierarchy(ns, mesh)
    c = rand_field(tuple(int(v) for v in shapes[1][::-1]), 4001)
    S.upload(1, hip.BUF_U, u)
    S.upload(1, hip.BUF_RHS, rhs)
    S.op(hip.OP_RELAX_FUSED, 1, 5)                     # 2 + 2 + 1 sweeps
    want = u
    for _ in range(5):
        want = port.relax3d(want, rhs, mesh, bcs)
    assert np.array_equal(S.download(1, hip.BUF_U), want)
    r = port.residual3d(want, rhs, mesh, bcs)
    S.op(hip.OP_RESIDUAL, 1)
    assert np.array_equal(S.download(1, hip.BUF_R), r)
    S.op(hip.OP_RESTRICT, 1)
    rc = port.restrict(r, ns, mesh, 1)
    assert np.array_equal(S.download(2, hip.BUF_RHS), rc)
    assert not S.download(2, hip.BUF_U).any()
    S.upload(2, hip.BUF_U, c)
    S.op(hip.OP_PROLONG, 1)
    assert np.array_equal(S.download(1, hip.BUF_U), want + port.interp(c, ns, mesh, 1))
    # Laplace fast path: rhs declared zero -> kernels never read it; same bits as rhs = 0 uploaded
    zero = np.zeros(shp)
    S.upload(1, hip.BUF_U, u)
    S.zero_rhs()
    S.op(hip.OP_RELAX_FUSED, 1, 5)
    S.op(hip.OP_RESIDUAL, 1)
    want0 = u
    for _ in range(5):
        want0 = port.relax3d(want0, zero, mesh, bcs)
    assert np.array_equal(S.download(1, hip.BUF_U), want0)
    assert np.array_equal(S.download(1, hip.BUF_R), port.residual3d(want0, zero, mesh, bcs))
    S.upload(1, hip.BUF_U, u)
    S.op(hip.OP_RELAX_COLOR, 1, 2)
    assert np.array_equal(S.download(1, hip.BUF_U), port.relax3d(port.relax3d(u, zero, mesh, bcs), zero, mesh, bcs))
    S.close()


@pytest.mark.parametrize("ns,meshf", _meshes(([22, 22, 22], [40, 24, 32], [33, 22, 27], [64, 64, 64], [200, 100, 70],
                                              [199, 101, 70], [256, 192, 160]), ([200, 100, 70], [199, 101, 70])))
def test_sweep_plus_residual_launch_bitwise(hip, ns, meshf):
    """the pipeline stage that evaluates r = rhs - L u behind the last sweep (op 9, forced) returns the
    bits of sweeps-then-residual.hip (which test_kernels3d_bitwise pins to the oracle): every BC set,
    odd/even sweep counts, general and declared-zero rhs"""
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    for bcs in ("NDDNDD", "DNDDND", "DDNDDN", "NNNNND", "DDDDDD"):
        S = hip.MGSolver(ns, mesh, bcs)
        for laplace in (False, True):
            if laplace:
                S.zero_rhs()
            else:
                S.upload(1, hip.BUF_RHS, rhs)
            for nsw in (1, 2, 5):
                S.upload(1, hip.BUF_U, u)
                S.op(hip.OP_RELAX_COLOR, 1, nsw)
                S.op(hip.OP_RESIDUAL, 1)
                uw, rw = S.download(1, hip.BUF_U), S.download(1, hip.BUF_R)
                S.upload(1, hip.BUF_U, u)
                S.upload(1, hip.BUF_R, np.full(shp, np.nan))
                S.op(hip.OP_RELAX_RES_FUSED, 1, nsw)
                assert np.array_equal(S.download(1, hip.BUF_U), uw), (bcs, laplace, nsw)
                assert np.array_equal(S.download(1, hip.BUF_R), rw), (bcs, laplace, nsw)
        S.close()


@pytest.mark.parametrize("ns", KERNEL_SHAPES_3D, ids=_tag)
def test_kernels3d_golden(hip, golden_dir, ns):
    """same kernels against the reference's own outputs (no oracle involved)"""
    g = np.load(os.path.join(golden_dir, f"kernels3d_{_tag(ns)}.npz"))
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    for bcs in BCS3:
        S = hip.MGSolver(ns, mesh, bcs)
        S.upload(1, hip.BUF_RHS, rhs)
        S.upload(1, hip.BUF_U, u)
        S.op(hip.OP_RELAX, 1, 1)
        assert np.array_equal(S.download(1, hip.BUF_U), g[f"relax_{bcs}"])
        S.upload(1, hip.BUF_U, u)
        S.op(hip.OP_RESIDUAL, 1)
        assert np.array_equal(S.download(1, hip.BUF_R), g[f"residual_{bcs}"])
        S.upload(1, hip.BUF_U, u)
        S.vcycle(1)
        assert np.array_equal(S.download(1, hip.BUF_U), g[f"vcycle_{bcs}"])
        S.close()


@pytest.mark.parametrize("ns", ([22, 22, 22], [33, 22, 27], [64, 64, 64]), ids=_tag)
@pytest.mark.parametrize("bcs", BCS3)
def test_solve3d_history_golden(hip, golden_dir, ns, bcs):
    h = json.load(open(os.path.join(golden_dir, "solve3d_history.json")))[f"{_tag(ns)}_{bcs}"]
    mesh = uniform_mesh(ns)
    us, rhs = manufactured_poisson(mesh, bcs)
    ierr, u, du, hist, nc = hip.poisson_solve(np.zeros_like(us), rhs, mesh, bcs, hist_len=64)
    assert ierr == 0 and nc == h["ncycles"]
    assert list(hist) == h["du"]
    assert du == h["du"][-1]
    if ns[0] <= 33:
        assert np.array_equal(u, np.load(os.path.join(golden_dir, f"solve3d_{_tag(ns)}_{bcs}.npy")))
    else:
        p = np.load(os.path.join(golden_dir, f"solve3d_{_tag(ns)}_{bcs}_planes.npz"))
        assert np.array_equal(u[ns[2] // 2], p["kz"])
        assert np.array_equal(u[:, ns[1] // 2], p["jy"])
        assert np.array_equal(u[:, :, ns[0] // 2], p["ix"])


@pytest.mark.parametrize("ns,meshf", _meshes(KERNEL_SHAPES_2D + ([64, 48],), ([27, 36],)))
def test_kernels2d(hip, port, ns, meshf):
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    rhs0 = rhs - rhs.mean()
    for bcs in ("NNNN", "DNND", "DDDD"):
        S = hip.MGSolver(ns, mesh, bcs)
        S.upload(1, hip.BUF_U, u)
        S.upload(1, hip.BUF_RHS, rhs)
        S.op(hip.OP_RELAX, 1, 1)
        got, want = S.download(1, hip.BUF_U), port.relax_nd(u, rhs, mesh, bcs)
        if bcs == "NNNN":
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)
        else:
            assert np.array_equal(got, want)
        S.upload(1, hip.BUF_U, u)
        S.op(hip.OP_RESIDUAL, 1)
        assert np.array_equal(S.download(1, hip.BUF_R), port.residual_nd(u, rhs, mesh, bcs))
        S.close()
    # transfers are shared with 3-D: exact
    S = hip.MGSolver(ns, mesh, "NNNN")
    shapes, _ = port.hierarchy(ns, mesh)
    for lvl in range(1, len(shapes)):
        f = rand_field(tuple(int(v) for v in shapes[lvl - 1][::-1]), 3000 + lvl)
        c = rand_field(tuple(int(v) for v in shapes[lvl][::-1]), 4000 + lvl)
        S.upload(1, hip.BUF_R, _pad_r(S, f))
        S.op(hip.OP_RESTRICT, lvl)
        assert np.array_equal(S.download(lvl + 1, hip.BUF_RHS), port.restrict(f, ns, mesh, lvl))
        S.upload(lvl + 1, hip.BUF_U, c)
        S.upload(lvl, hip.BUF_U, np.zeros_like(f))
        S.op(hip.OP_PROLONG, lvl)
        assert np.array_equal(S.download(lvl, hip.BUF_U), port.interp(c, ns, mesh, lvl))
    S.close()
    # full all-Neumann solve
    ierr, us, du, hist, nc = hip.poisson_solve(np.zeros(shp), rhs0, mesh, "NNNN")
    ierr2, us2, du2, hist2, nc2, sw = port.solve_bvp(np.zeros(shp), rhs0, mesh, "NNNN", hist_len=64)
    assert ierr == ierr2 == 0 and nc == nc2
    np.testing.assert_allclose(us, us2, rtol=0, atol=1e-13)


# tests/integration_test/results_test1.txt:6-14 (dx, Ea_max, Ea_avg, Eb_max, Eb_avg): the reference's published
# run of its nine resolutions (22 x scale, integration_test1.py:105-120), and results_test2.txt:6-14: the same
# with the MEAN difference as the convergence metric (integration_test2.py:130, `mean=True`) - rows that stop a
# cycle earlier or later differ from table 1 in the last printed digit or two
RESULTS_TEST1 = {
    22: ("4.76190e-02", "1.86048e-03", "2.67773e-04", "7.65805e-02", "6.53421e-03"),
    44: ("2.32558e-02", "4.44560e-04", "6.18187e-05", "1.95261e-02", "1.35063e-03"),
    66: ("1.53846e-02", "1.94618e-04", "2.67419e-05", "8.72558e-03", "5.57752e-04"),
    77: ("1.31579e-02", "1.42398e-04", "1.95035e-05", "6.42133e-03", "4.00818e-04"),
    88: ("1.14943e-02", "1.08647e-04", "1.48417e-05", "4.92049e-03", "3.01727e-04"),
    99: ("1.02041e-02", "8.56395e-05", "1.16779e-05", "3.89144e-03", "2.35234e-04"),
    160: ("6.28931e-03", "3.25317e-05", "4.41144e-06", "1.49319e-03", "8.63559e-05"),
    176: ("5.71429e-03", "2.68552e-05", "3.63900e-06", "1.23446e-03", "7.09164e-05"),
    220: ("4.56621e-03", "1.71483e-05", "2.31968e-06", "7.90579e-04", "4.48076e-05"),
}
RESULTS_TEST2 = dict(RESULTS_TEST1)
RESULTS_TEST2.update({
    99: ("1.02041e-02", "8.56396e-05", "1.16779e-05", "3.89144e-03", "2.35234e-04"),
    160: ("6.28931e-03", "3.25317e-05", "4.41138e-06", "1.49319e-03", "8.63560e-05"),
    176: ("5.71429e-03", "2.68552e-05", "3.63899e-06", "1.23446e-03", "7.09164e-05"),
    220: ("4.56621e-03", "1.71485e-05", "2.31965e-06", "7.90579e-04", "4.48076e-05"),
})
_ROWS_MEASURED = {}


@pytest.mark.parametrize("mean", (False, True), ids=("max_metric_table1", "mean_metric_table2"))
@pytest.mark.parametrize("n", sorted(RESULTS_TEST1))
def test_pipeline_known_answer_rows(hip, n, mean):
    """The reference's own published rows - all nine resolutions of both of its integration tests (max and mean
    form of the convergence metric) - through the reference's own entry point and the drop-in Python loader:
    every entry to all printed digits"""
    import ndsm_amd
    x, y, z, A1, b1 = analytic_case(n)
    ierr, A, B = ndsm_amd.vector_potential(x, y, z, b1.copy(), mean=mean)
    assert ierr == 0
    eA = np.linalg.norm(A1 - A, axis=0)
    eB = np.linalg.norm(b1 - B, axis=0)
    vals = (x[1] - x[0], eA.max(), eA.mean(), eB.max(), eB.mean())
    if not mean:
        _ROWS_MEASURED[n] = vals
    got = tuple("{:.5e}".format(v) for v in vals)
    assert got == (RESULTS_TEST2 if mean else RESULTS_TEST1)[n]


def test_bz_formed_behind_the_az_solve_bitwise(hip):
    """B_z = d(A_y)/dx - d(A_x)/dy is formed (and sent home) as soon as A_x and A_y are final, behind the A_z solve;
    against the single curl at the end (NDSM_HIP_NO_EARLY_BZ=1): the same A and B, bit for bit - on a field whose
    three components all take several cycles, odd and even shapes"""
    import ndsm_amd
    keep = os.environ.get("NDSM_HIP_NO_EARLY_BZ")
    try:
        for ns in ([96, 80, 72], [33, 22, 27]):
            x, y, z, _A1, b = analytic_case(ns)
            b = b + 0.2 * np.random.default_rng(4).standard_normal(b.shape)
            os.environ.pop("NDSM_HIP_NO_EARLY_BZ", None)
            i1, A, B = ndsm_amd.vector_potential(x, y, z, b)
            os.environ["NDSM_HIP_NO_EARLY_BZ"] = "1"
            i2, A2, B2 = ndsm_amd.vector_potential(x, y, z, b)
            assert i1 == i2 and np.array_equal(A, A2) and np.array_equal(B, B2), ns
    finally:
        if keep is None:
            os.environ.pop("NDSM_HIP_NO_EARLY_BZ", None)
        else:
            os.environ["NDSM_HIP_NO_EARLY_BZ"] = keep


@pytest.mark.parametrize("ns", ([4, 4, 4], [4, 5, 7], [6, 4, 9], [7, 7, 4]), ids=_tag)
def test_pipeline_smallest_grids(hip, port, ns):
    """the smallest grids the reference's algorithm is defined on (every dimension >= 4: one or two levels, 2-D
    faces of 4 x 4 points) against the oracle, at the pipeline's stated tolerance"""
    import ndsm_amd
    x, y, z, _A1, b = analytic_case(ns)
    ierr, A, B = ndsm_amd.vector_potential(x, y, z, b.copy())
    ierr2, A2, B2, _io, _ro = port.vector_potential(x, y, z, b)
    assert ierr == ierr2
    sc = np.abs(A2).max()
    h = x[1] - x[0]
    assert np.abs(A - A2).max() <= 1e-11 * sc and np.abs(B - B2).max() <= 1e-11 * sc * 4 / h


@pytest.mark.parametrize("ns", ([3, 8, 8], [2, 9, 9], [2, 2, 2]), ids=_tag)
def test_pipeline_grid_too_small_is_an_error_code(hip, ns):
    """below four points in a dimension the reference's level count FLOOR(LOG(nmin/4)/LOG(2)) + 1 is not positive
    and the reference itself stops or crashes (seen with oracle/_ref); here: return code 9002, A untouched, a text"""
    import ndsm_amd
    x, y, z, _A1, b = analytic_case(ns)
    ierr, A, _B = ndsm_amd.vector_potential(x, y, z, b.copy())
    assert ierr == 9002 and not A.any()
    assert "at least 4 points" in hip.last_error(hip.load_library())


def test_2d_neumann_solve_error_scaling(hip):
    """the reference's unit_test_2D_solve property (tests/unit_tests/unit_test_2D_solve.f90:63-242; stale there -
    it no longer compiles - so re-stated, not run): the 2-D all-Neumann Poisson problem laplace(u) = a (2x - Lx)
    + b (2y - Ly) on its 27 x 36 base mesh scaled up, zero initial guess, ms = 5, tolerance 1e-12; the solution
    with its mean removed is a x^2 (x/3 - Lx/2) + b y^2 (y/3 - Ly/2) minus its mean.  Every solve converges and
    the max / mean errors fall as h^2"""
    a1, b1 = 0.3745401188473625, 0.9507143064099162
    rows = []
    for scale in (1.0, 1.5, 2.0, 4.0, 5.5, 10.0):
        nx, ny = int(np.ceil(27 * scale)), int(np.ceil(36 * scale))
        dq = 1.0 / (nx - 1)
        x, y = np.arange(nx) * dq, np.arange(ny) * dq
        Lx, Ly = 1.0, y.max() - y.min()
        rhs = a1 * (2 * x[None, :] - Lx) + b1 * (2 * y[:, None] - Ly)
        ue = a1 * x[None, :] ** 2 * (x[None, :] / 3 - Lx / 2) + b1 * y[:, None] ** 2 * (y[:, None] / 3 - Ly / 2)
        ue = ue - ue.mean()
        S = hip.MGSolver([nx, ny], [x, y], "NNNN", ms=5, ex_tol=1e-12)
        S.upload(1, hip.BUF_RHS, rhs)
        S.upload(1, hip.BUF_U, np.zeros_like(rhs))
        ierr, du, nc, _h = S.solve(vc_tol=1e-12, nmax=256)
        u = S.download(1, hip.BUF_U)
        S.close()
        assert ierr == 0 and nc < 64, (scale, ierr, nc, du)
        rows.append((dq, np.abs(u - ue).max(), np.abs(u - ue).mean()))
    rows = np.array(rows)
    for k, name in ((1, "Emax"), (2, "Eavg")):
        gamma = np.polyfit(np.log(rows[:, 0]), np.log(rows[:, k]), 1)[0]
        assert 1.9 < gamma < 2.1, (name, gamma, rows)


def test_pipeline_error_scaling(hip):
    """the property the reference's integration test reports (integration_test1.py:157-160, utests.py:32-65): the
    errors against the analytic field fall as a power law in the mesh spacing - second order for A, first to
    second for B = curl A (one-sided differences on the boundary)"""
    import ndsm_amd
    sizes = [22, 44, 66, 88, 160, 220]
    rows = []
    for n in sizes:
        if n not in _ROWS_MEASURED:
            x, y, z, A1, b1 = analytic_case(n)
            ierr, A, B = ndsm_amd.vector_potential(x, y, z, b1.copy())
            assert ierr == 0
            eA = np.linalg.norm(A1 - A, axis=0)
            eB = np.linalg.norm(b1 - B, axis=0)
            _ROWS_MEASURED[n] = (x[1] - x[0], eA.max(), eA.mean(), eB.max(), eB.mean())
        rows.append(_ROWS_MEASURED[n])
    rows = np.array(rows)
    want = np.array([[float(v) for v in RESULTS_TEST1[n]] for n in sizes])
    for k, (name, lo, hi) in enumerate((("Ea_max", 1.9, 2.1), ("Ea_avg", 1.9, 2.1), ("Eb_max", 1.8, 2.1), ("Eb_avg", 1.9, 2.3)), start=1):
        gamma = np.polyfit(np.log(rows[:, 0]), np.log(rows[:, k]), 1)[0]
        gamma_ref = np.polyfit(np.log(want[:, 0]), np.log(want[:, k]), 1)[0]
        assert lo < gamma < hi and abs(gamma - gamma_ref) < 1e-3, (name, gamma, gamma_ref)


@pytest.mark.parametrize("name,ns", (("pipeline_22", 22), ("pipeline_33x22x27", [33, 22, 27])))
def test_pipeline_golden(hip, golden_dir, name, ns):
    import ndsm_amd
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    x, y, z, A1, b1 = analytic_case(ns)
    ierr, A, B = ndsm_amd.vector_potential(x, y, z, b1.copy())
    assert ierr == 0
    scale = np.abs(g["A"]).max()
    h = x[1] - x[0]
    assert np.abs(A - g["A"]).max() <= 1e-12 * scale
    assert np.abs(B - g["B"]).max() <= 1e-12 * scale * 4 / h


def test_pipeline_vs_oracle_options(hip, port):
    """non-default options through the reference ABI: mean metric, ms, tolerances"""
    import ndsm_amd
    x, y, z, A1, b1 = analytic_case([24, 30, 20])
    for kw in (dict(mean=True), dict(ms=3, vc_tol=1e-8), dict(ncycles_max=2)):
        ierr, A, B = ndsm_amd.vector_potential(x, y, z, b1.copy(), **kw)
        ierr2, A2, B2, _, _ = port.vector_potential(x, y, z, b1, **kw)
        assert ierr == ierr2, kw
        scale = np.abs(A2).max()
        assert np.abs(A - A2).max() <= 1e-11 * scale, kw
        assert np.abs(B - B2).max() <= 1e-11 * scale * 4 / (x[1] - x[0]), kw


def test_roundtrip_properties_large(hip):
    """size-independent properties at a size the oracle is too slow for (256^3):
    (i) linearity of a V-cycle in (u, rhs); (ii) Dirichlet faces are never
    written; (iii) residual of the converged solve is at rounding level of
    vc_tol; (iv) adjointness <u_c, R r_f>_c = <P u_c, r_f>_f of the transfer pair
    (the reference's unit_test_galerkin property, tests/unit_tests/unit_test_galerkin.f90:56-189)."""
    ns = [256, 256, 256]
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    bcs = "NDDNDD"
    S = hip.MGSolver(ns, mesh, bcs)
    u1, f1 = rand_field(shp, 1), rand_field(shp, 2)
    u2, f2 = rand_field(shp, 3), rand_field(shp, 4)

    def vc(u, f):
        S.upload(1, hip.BUF_U, u)
        S.upload(1, hip.BUF_RHS, f)
        S.vcycle(1)
        return S.download(1, hip.BUF_U)

    a, b, c = vc(u1, f1), vc(u2, f2), vc(u1 + 2 * u2, f1 + 2 * f2)
    # NOTE: the coarsest solve has a data-dependent sweep count, so linearity holds to the
    # coarse tolerance (ex_tol = 1e-13 on the correction), not to rounding
    assert np.abs(c - (a + 2 * b)).max() < 1e-9 * np.abs(c).max()
    # (ii)
    assert np.array_equal(a[:, 0, :], u1[:, 0, :]) and np.array_equal(a[:, -1, :], u1[:, -1, :])
    assert np.array_equal(a[0], u1[0]) and np.array_equal(a[-1], u1[-1])
    # (iv) adjointness with the cell volumes as inner-product weights
    hf = mesh[0][1] - mesh[0][0]
    nc = S.shapes[1]
    hc = 1.0 / (nc[0] - 1)
    rf = rand_field(shp, 5)
    uc = rand_field(tuple(nc[::-1]), 6)
    S.upload(1, hip.BUF_R, rf)
    S.op(hip.OP_RESTRICT, 1)
    Rr = S.download(2, hip.BUF_RHS)
    S.upload(2, hip.BUF_U, uc)
    S.upload(1, hip.BUF_U, np.zeros(shp))
    S.op(hip.OP_PROLONG, 1)
    Pu = S.download(1, hip.BUF_U)
    lhs = float((uc * Rr).sum()) * hc ** 3
    rhs_ = float((Pu * rf).sum()) * hf ** 3
    assert abs(lhs - rhs_) <= 1e-12 * abs(lhs)
    S.close()
    # (iii)
    us, rhs = manufactured_poisson(mesh, bcs)
    ierr, u, du, hist, ncyc = hip.poisson_solve(np.zeros_like(us), rhs, mesh, bcs, hist_len=64)
    assert ierr == 0 and du < 1e-10 and ncyc <= 20
    assert np.abs(u - us).max() < 5e-5          # O(h^2) truncation error at h = 1/255
    assert all(hist[i + 1] < 0.5 * hist[i] for i in range(len(hist) - 1))


@pytest.mark.parametrize("ns,nranks,meshf", [pytest.param(ns, nr, uniform_mesh, id=f"{ns}-{nr}") for ns, nr in
                                             (([64, 64, 64], 2), ([64, 48, 96], 3), ([128, 128, 128], 4), ([128, 64, 160], 8))] +
                         [pytest.param([64, 48, 96], 3, aniso_mesh, id="aniso-[64, 48, 96]-3")])
def test_slab_world_bitwise(hip, ns, nranks, meshf):
    """z-slab decomposition (loop-back transport: all slabs on this GPU, neighbours reached by
    device copies; production swaps those copies for RCCL send/recv): sweeps, a V-cycle and a whole
    solve must return the SAME BITS as the single-domain solver."""
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    for bcs in BCS3:
        S = hip.MGSolver(ns, mesh, bcs)
        W = hip.World(ns, mesh, bcs, nranks)
        assert W.nlocal == nranks and W.slabs[0]["z0"] == 0 and W.slabs[-1]["z1"] == ns[2]
        S.upload(1, hip.BUF_U, u)
        S.upload(1, hip.BUF_RHS, rhs)
        W.upload(hip.BUF_U, u)
        W.upload(hip.BUF_RHS, rhs)
        S.op(hip.OP_RELAX, 1, 3)
        W.relax(3)
        assert np.array_equal(W.download(hip.BUF_U), S.download(1, hip.BUF_U)), f"sweeps {bcs}"
        S.upload(1, hip.BUF_U, u)
        W.upload(hip.BUF_U, u)
        S.vcycle(2)
        W.vcycle(2)
        assert np.array_equal(W.download(hip.BUF_U), S.download(1, hip.BUF_U)), f"vcycle {bcs}"
        S.close()
        W.close()
    bcs = "NDDNDD"
    us, rhs = manufactured_poisson(mesh, bcs)
    ierr, uref, du, hist, nc = hip.poisson_solve(np.zeros_like(us), rhs, mesh, bcs, hist_len=64)
    W = hip.World(ns, mesh, bcs, nranks)
    W.upload(hip.BUF_U, np.zeros_like(us))
    W.upload(hip.BUF_RHS, rhs)
    ierr2, du2, nc2, hist2 = W.solve(hist_len=64)
    assert (ierr2, nc2, du2) == (ierr, nc, du) and list(hist2) == list(hist)
    assert np.array_equal(W.download(hip.BUF_U), uref)
    W.close()


def test_reference_quirks(hip, port):
    """Q3' (returned ierr = flag of the last 2-D face solve; the 3-D flags are additive in iopt[8])
    and Q2 (the Az solve always smooths with ms = 5) through the reference entry point."""
    import ctypes
    import ndsm_amd
    x, y, z, A1, b1 = analytic_case(24)
    b = b1.copy()
    b[2, -1, :, :] = 0.0                       # B.n = 0 on the top face: its chi solve converges at once
    ierr, A, B = ndsm_amd.vector_potential(x, y, z, b, ncycles_max=2)
    ierr_o, A_o, B_o, io_o, _ = port.vector_potential(x, y, z, b, ncycles_max=2)
    assert ierr == ierr_o == 0
    assert np.abs(A - A_o).max() <= 1e-11 * np.abs(A_o).max()
    # additive slot: which 3-D solves missed vc_tol
    L = ndsm_amd.load_library()
    ns = np.array(b.shape[::-1], dtype=np.intc)
    io = np.zeros(16, dtype=np.intc)
    ro = np.zeros(16)
    io[0], io[1], io[6], io[7] = 5, 2, 1, 10000
    ro[0], ro[1] = 1e-10, 1e-13
    Aq, Bq = np.zeros(b.size), b.ravel().copy()
    f = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    rc = L.ndsm_vector_solve(ctypes.c_size_t(b.size), ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                             io.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), f(ro), f(x), f(y), f(z), f(Aq), f(Bq))
    assert rc == 0 and io[3] == 0 and (io[L.get_iopt_fail3d()] & 0b011) == 0b011 and ro[L.get_ropt_tim()] > 0
    # Q2: ms = 3 for Ax, Ay but 5 for Az -> identical to the oracle (which hard-codes the same)
    ierr, A, B = ndsm_amd.vector_potential(x, y, z, b1.copy(), ms=3)
    ierr_o, A_o, B_o, _, _ = port.vector_potential(x, y, z, b1, ms=3)
    assert ierr == ierr_o and np.abs(A - A_o).max() <= 1e-11 * np.abs(A_o).max()


@pytest.mark.gpu
@pytest.mark.parametrize("ns,meshf", _meshes(([64, 64, 64], [128, 96, 80], [256, 256, 256]), ([128, 96, 80],)))
def test_mixed_precision_solve(hip, ns, meshf):
    """BASELINE config[4] mode: fp64 residual + fp32 correction V-cycle on level 1 (csrc/mixed.hip).
    In exact arithmetic it is the reference's iteration, so: the same number of V-cycles to the same
    vc_tol, du history equal to fp32 rounding, and a final solution within a few vc_tol (the
    stopping rule's own resolution; absolute, as vc_tol is) of the all-fp64 solve."""
    mesh = meshf(ns)
    for bcs in ("NDDNDD", "DNDDND", "DDDDDD"):
        us, rhs = manufactured_poisson(mesh, bcs) if bcs == "NDDNDD" else (None, rand_field(tuple(ns[::-1]), 77) * 10.0)
        u0 = np.zeros(tuple(ns[::-1]))
        if us is not None:
            u0[:, 0, :], u0[:, -1, :], u0[0], u0[-1] = us[:, 0, :], us[:, -1, :], us[0], us[-1]
        S = hip.MGSolver(ns, mesh, bcs)
        S.upload(1, hip.BUF_RHS, rhs)
        S.upload(1, hip.BUF_U, u0)
        ie64, du64, nc64, h64 = S.solve(vc_tol=1e-11, nmax=64, hist_len=64)
        u64 = S.download(1, hip.BUF_U)
        assert S.set_precision(2), "fp32 kernels should cover this level"
        S.upload(1, hip.BUF_U, u0)
        ie32, du32, nc32, h32 = S.solve(vc_tol=1e-11, nmax=64, hist_len=64)
        u32 = S.download(1, hip.BUF_U)
        S.close()
        assert ie64 == 0 and ie32 == 0, (bcs, ie64, ie32)
        assert abs(nc32 - nc64) <= 1, (bcs, nc32, nc64)
        n = min(nc32, nc64) - 1
        assert np.allclose(h32[:n], h64[:n], rtol=1e-3, atol=0), (bcs, h32[:n], h64[:n])
        assert np.abs(u32 - u64).max() <= 5e-11, (bcs, np.abs(u32 - u64).max(), np.abs(u64).max())


@pytest.mark.gpu
@pytest.mark.parametrize("ns,ms,meshf", [pytest.param(ns, ms, uniform_mesh, id=f"{ns}-{ms}") for ns, ms in
                                        (([256, 192, 160], 5), ([192, 192, 192], 4), ([256, 256, 256], 1), ([257, 161, 158], 5),
                                         ([193, 190, 131], 2))] +
                         [pytest.param([257, 161, 158], 5, aniso_mesh, id="aniso-[257, 161, 158]-5")])
def test_fused_metric_bitwise(hip, ns, ms, meshf):
    """mg_solve on a large level 1 keeps the start-of-cycle iterate in place (three rotating buffers)
    and lets the launch of the cycle's last sweep evaluate update_u's max|u_new - u_old|
    (ndsm_multigrid_core.f90:1077-1122): same du history, same cycle count and same solution bits as
    the separate metric pass (NDSM_HIP_NO_TRACK), for ms odd, even and 1, general and declared-zero rhs."""
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    u0, rhs = rand_field(shp, 11), rand_field(shp, 12) * 50.0
    for bcs in ("NDDNDD", "DDNDDN"):
        for laplace in (False, True):
            out = []
            for notrack in (True, False):
                if notrack:
                    os.environ["NDSM_HIP_NO_TRACK"] = "1"
                else:
                    os.environ.pop("NDSM_HIP_NO_TRACK", None)
                S = hip.MGSolver(ns, mesh, bcs, ms=ms)
                if laplace:
                    S.zero_rhs()
                else:
                    S.upload(1, hip.BUF_RHS, rhs)
                S.upload(1, hip.BUF_U, u0)
                ie, du, nc, h = S.solve(vc_tol=1e-9, nmax=6, hist_len=16)
                out.append((ie, du, nc, list(h), S.download(1, hip.BUF_U)))
                S.close()
            os.environ.pop("NDSM_HIP_NO_TRACK", None)
            a, b = out
            assert a[:4] == b[:4], (bcs, laplace, a[:4], b[:4])
            assert np.array_equal(a[4], b[4]), (bcs, laplace)


@pytest.mark.gpu
@pytest.mark.parametrize("ns,meshf", _meshes(([161, 120, 115], [160, 121, 115]), ([161, 120, 115],)))
def test_tracked_solve_vs_oracle(hip, port, ns, meshf):
    """a level 1 just large enough for every large-level path at once (fused smoother incl. its odd-nx
    ghost-column variant, sweep+residual, streamed restriction, prolongation and metric folded into the
    smoother launches) - three solve-loop cycles against the oracle: du history and solution bits"""
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    u0, rhs = rand_field(shp, 21), rand_field(shp, 22) * 10.0
    for bcs, lap in (("NDDNDD", True), ("DNDDDN", False)):
        r = np.zeros(shp) if lap else rhs
        ie2, u2, du2, h2, nc2, _sw = port.solve_bvp(u0.copy(), r, mesh, bcs, ms=5, nmax=3, hist_len=8)
        S = hip.MGSolver(ns, mesh, bcs, ms=5)
        if lap:
            S.zero_rhs()
        else:
            S.upload(1, hip.BUF_RHS, rhs)
        S.upload(1, hip.BUF_U, u0)
        ie, du, nc, h = S.solve(vc_tol=1e-10, nmax=3, hist_len=8)
        got = S.download(1, hip.BUF_U)
        S.close()
        assert nc == nc2 == 3 and list(h) == list(h2[:3]), (bcs, list(h), list(h2[:3]))
        assert np.array_equal(got, u2), bcs


@pytest.mark.gpu
def test_pipeline_mixed_precision_and_large_paths(hip):
    """The whole ndsm_vector_solve pipeline at a size where every large-level path is live (fused
    two-sweep smoother, sweep+residual launch, streamed restriction, tiled prolongation, kept-iterate
    metric): known-answer errors fall as h^2 against the analytic field (the reference's own
    acceptance test, tests/integration_test/integration_test1.py), and the additive mixed-precision
    option (get_iopt_prec) reproduces the fp64 pipeline to the solve tolerance."""
    import ndsm_amd
    n = 192
    x, y, z, A1, b1 = analytic_case(n)
    ierr, A, B = ndsm_amd.vector_potential(x, y, z, b1.copy())
    assert ierr == 0
    ea = np.linalg.norm(A1 - A, axis=0)
    eb = np.linalg.norm(b1 - B, axis=0)
    h = x[1] - x[0]
    # results_test1.txt rows (22..220) scale as Ea_max ~ 0.9 h^2, Eb_max ~ 37 h^2
    assert ea.max() < 2.0 * h * h and eb.max() < 60.0 * h * h, (ea.max() / h ** 2, eb.max() / h ** 2)
    ierr2, A2, B2 = ndsm_amd.vector_potential(x, y, z, b1.copy(), mixed_precision=True)
    assert ierr2 == 0
    assert np.abs(A2 - A).max() <= 1e-9 * np.abs(A).max(), np.abs(A2 - A).max()
    assert np.abs(B2 - B).max() <= 1e-9 * np.abs(A).max() * 4 / h, np.abs(B2 - B).max()


@pytest.mark.gpu
def test_slab_world_laplace_variant(hip):
    """World.zero_rhs: the z-slab path with the rhs declared zero (kernels never read it) returns the
    bits of the single-domain solver with a zero rhs uploaded"""
    ns, nranks = [64, 64, 96], 3
    mesh = uniform_mesh(ns)
    u = rand_field(tuple(ns[::-1]), 5)
    S = hip.MGSolver(ns, mesh, "DNDDND")
    W = hip.World(ns, mesh, "DNDDND", nranks)
    S.upload(1, hip.BUF_U, u)
    S.upload(1, hip.BUF_RHS, np.zeros_like(u))
    W.upload(hip.BUF_U, u)
    W.zero_rhs()
    S.vcycle(2)
    W.vcycle(2)
    assert np.array_equal(W.download(hip.BUF_U), S.download(1, hip.BUF_U))
    S.close()
    W.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ns,nranks,levels,meshf", [pytest.param(ns, nr, lv, uniform_mesh, id=f"{ns}-{nr}-{lv}") for ns, nr, lv in
                                                    (([64, 64, 256], 4, 2), ([128, 64, 256], 2, 3), ([64, 64, 384], 8, 2))] +
                         [pytest.param([64, 64, 256], 4, 2, aniso_mesh, id="aniso-[64, 64, 256]-4-2")])
def test_slab_world_distributed_coarse_levels(hip, ns, nranks, levels, meshf):
    """several distributed levels (NDSM_HIP_DIST_LEVELS; by default chosen by size): every rank
    restricts straight into its own slab of the next level's rhs and prolongs from it, only the first
    non-distributed level travels to rank 0.  Loop-back world vs the single-domain solver: V-cycles and
    a whole solve, bit for bit."""
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    os.environ["NDSM_HIP_DIST_LEVELS"] = str(levels)
    try:
        for bcs in ("NDDNDD", "DDNDDN"):
            S = hip.MGSolver(ns, mesh, bcs)
            W = hip.World(ns, mesh, bcs, nranks)
            assert W.dist_levels == levels, W.dist_levels
            for X in (S,):
                X.upload(1, hip.BUF_U, u)
                X.upload(1, hip.BUF_RHS, rhs)
            W.upload(hip.BUF_U, u)
            W.upload(hip.BUF_RHS, rhs)
            S.vcycle(2)
            W.vcycle(2)
            assert np.array_equal(W.download(hip.BUF_U), S.download(1, hip.BUF_U)), f"vcycle {bcs}"
            ie1, du1, nc1, h1 = S.solve(hist_len=64)
            ie2, du2, nc2, h2 = W.solve(hist_len=64)
            assert (ie1, nc1) == (ie2, nc2) and np.array_equal(h1, h2), (bcs, nc1, nc2)
            assert np.array_equal(W.download(hip.BUF_U), S.download(1, hip.BUF_U)), f"solve {bcs}"
            S.close()
            W.close()
    finally:
        os.environ.pop("NDSM_HIP_DIST_LEVELS", None)


@pytest.mark.gpu
def test_interpolation_reproduces_trilinear_functions(hip):
    """the reference's unit_test_interp property (tests/unit_tests/unit_test_interp.f90:42-181): the
    interpolation is exact (to rounding) for functions that are linear in every coordinate - here
    through both prolongation kernels (tiled for the large level pair, gather for a small one) on the
    non-nested meshes, including the last fine points that lie on the coarse mesh's end."""
    for ns in ([200, 100, 70], [64, 40, 24]):
        mesh = uniform_mesh(ns)
        S = hip.MGSolver(ns, mesh, "DDDDDD")
        nc = S.shapes[1]
        rng = np.random.default_rng(7)
        c = rng.uniform(-1, 1, 8)
        f = lambda X, Y, Z: (c[0] + c[1] * X + c[2] * Y + c[3] * Z + c[4] * X * Y + c[5] * Y * Z + c[6] * X * Z  # noqa: E731
                             + c[7] * X * Y * Z)
        cm = [np.linspace(m[0], m[-1], n) for m, n in zip(mesh, nc)]
        Zc, Yc, Xc = np.meshgrid(cm[2], cm[1], cm[0], indexing="ij")
        Zf, Yf, Xf = np.meshgrid(mesh[2], mesh[1], mesh[0], indexing="ij")
        S.upload(2, hip.BUF_U, f(Xc, Yc, Zc))
        S.upload(1, hip.BUF_U, np.zeros(tuple(ns[::-1])))
        S.op(hip.OP_PROLONG, 1)
        got = S.download(1, hip.BUF_U)
        want = f(Xf, Yf, Zf)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), np.abs(got - want).max()
        S.close()


@pytest.mark.gpu
def test_full_size_config3_properties(hip):
    """BASELINE config[2] size (512^3): three solve-loop cycles of the Ax Laplace problem with every
    large-level path live (two-sweep launches, sweep+residual, correction folded into the first
    post-smoothing launch, metric in the last) against the same cycles with the separate
    prolongation / metric passes (NDSM_HIP_NO_TRACK): same du history and same bits; the Dirichlet
    faces are never written; du falls monotonically at the V-cycle's rate."""
    import bench
    n = 512
    mesh, u0 = bench.boundary_problem(n)
    out = []
    for notrack in (False, True):
        if notrack:
            os.environ["NDSM_HIP_NO_TRACK"] = "1"
        else:
            os.environ.pop("NDSM_HIP_NO_TRACK", None)
        try:
            S = hip.MGSolver([n, n, n], mesh, "NDDNDD")
            S.zero_rhs()
            S.upload(1, hip.BUF_U, u0)
            ie, du, nc, h = S.solve(vc_tol=0.0, nmax=3, hist_len=8)
            out.append((list(h), S.download(1, hip.BUF_U)))
            S.close()
        finally:
            os.environ.pop("NDSM_HIP_NO_TRACK", None)
    (h1, a), (h2, b) = out
    assert h1 == h2 and len(h1) == 3
    assert np.array_equal(a, b)
    assert h1[1] < 0.3 * h1[0] and h1[2] < 0.3 * h1[1], h1
    assert np.array_equal(a[:, 0, :], u0[:, 0, :]) and np.array_equal(a[:, -1, :], u0[:, -1, :])
    assert np.array_equal(a[0], u0[0]) and np.array_equal(a[-1], u0[-1])


@pytest.mark.gpu
def test_out_of_memory_is_a_clean_error(hip):
    """a hierarchy that cannot fit in HBM (2048^3: 64 GiB per level-1 array) fails with a device error
    code >= 9001 ... (the reference would abort the process in ALLOCATE); nothing leaks into the
    next call: a small solve right after it still returns the oracle's bits"""
    n = 2048
    mesh = [np.linspace(0, 1, n)] * 3
    with pytest.raises(hip.NdsmHipError):
        hip.MGSolver([n, n, n], mesh, "NDDNDD")
    ns = [22, 22, 22]
    m = uniform_mesh(ns)
    u, rhs = rand_field((22, 22, 22), 1), rand_field((22, 22, 22), 2)
    S = hip.MGSolver(ns, m, "NDDNDD")
    S.upload(1, hip.BUF_U, u)
    S.upload(1, hip.BUF_RHS, rhs)
    S.vcycle(1)
    a = S.download(1, hip.BUF_U)
    S.upload(1, hip.BUF_U, u)
    S.vcycle(1)
    assert np.array_equal(a, S.download(1, hip.BUF_U))
    S.close()


@pytest.mark.gpu
def test_argument_errors_are_reported_not_fatal(hip):
    """bad arguments come back as error codes / exceptions (the reference STOPs the process on its
    internal asserts, ndsm_root.f90:317-455): unknown BC letter, a dimension below the 4 points one
    grid needs, an op on a level that does not exist, a forced fused sweep on a shape it cannot take"""
    ns = [24, 24, 24]
    m = uniform_mesh(ns)
    with pytest.raises(hip.NdsmHipError):
        hip.MGSolver(ns, m, "NDDNDX")
    with pytest.raises(hip.NdsmHipError):
        hip.MGSolver([24, 3, 24], uniform_mesh([24, 3, 24]), "NDDNDD")
    S = hip.MGSolver(ns, m, "NDDNDD")
    with pytest.raises(hip.NdsmHipError):
        S.op(hip.OP_RELAX, S.ngrids + 1, 1)
    S.close()
    S = hip.MGSolver([12, 24, 24], uniform_mesh([12, 24, 24]), "NDDNDD")     # rows shorter than the fused tile's minimum
    with pytest.raises(hip.NdsmHipError):
        S.op(hip.OP_RELAX_FUSED, 1, 1)
    S.upload(1, hip.BUF_U, rand_field((24, 24, 12), 3))
    S.op(hip.OP_RELAX, 1, 1)                                                 # the two-pass kernel takes it
    S.close()
    # the reference's only input check: fewer than two points -> ierr = 1, nothing else touched
    import ndsm_amd
    x = np.linspace(0, 1, 1)
    b = np.zeros((3, 1, 1, 1))
    ierr, A, B = ndsm_amd.vector_potential(x, x, x, b)
    assert ierr == 1


@pytest.mark.gpu
def test_random_shapes_solve_vs_oracle(hip, port):
    """seeded random small shapes (8..71 per dimension, odd and even), random D/N face letters, random
    ms: four solve-loop cycles on the device against the oracle - solution bits, du history, cycle count
    (scripts/fuzz_shapes.py runs the same with more cases)"""
    rng = np.random.default_rng(20260101)
    for c in range(16):
        ns = [int(rng.integers(8, 72)) for _ in range(3)]
        bcs = "".join(rng.choice(["D", "N"]) for _ in range(6))
        if bcs == "NNNNNN":
            bcs = "NNNNND"
        ms = int(rng.integers(1, 6))
        mesh = uniform_mesh(ns)
        shp = tuple(ns[::-1])
        u, rhs = rand_field(shp, 100 + c), rand_field(shp, 200 + c)
        ierr2, u2, du2, h2, nc2, sw = port.solve_bvp(u.copy(), rhs, mesh, bcs, ms=ms, nmax=4, hist_len=8)
        S = hip.MGSolver(ns, mesh, bcs, ms=ms)
        S.upload(1, hip.BUF_U, u)
        S.upload(1, hip.BUF_RHS, rhs)
        ierr, du, nc, h = S.solve(vc_tol=1e-10, nmax=4, hist_len=8)
        got = S.download(1, hip.BUF_U)
        S.close()
        assert nc == nc2 and list(h) == list(h2[:len(h)]), (ns, bcs, ms)
        assert np.array_equal(got, u2), (ns, bcs, ms)


@pytest.mark.gpu
def test_random_shapes_fused_launches(hip):
    """seeded random level shapes (ragged against every tile size), random face letters, 1..5 sweeps, with
    and without a right-hand side: the forced fused launches (and the sweep+residual launch) return the
    bits of the two-pass kernels + residual.hip (scripts/fuzz_fused.py)"""
    rng = np.random.default_rng(20260102)
    for c in range(30):
        ns = [int(rng.integers(16, 300)), int(rng.integers(16, 200)), int(rng.integers(8, 120))]
        bcs = "".join(rng.choice(["D", "N"]) for _ in range(6))
        if bcs == "NNNNNN":
            bcs = "DNNNNN"
        nsw = int(rng.integers(1, 6))
        lap = bool(rng.integers(0, 2))
        mesh = uniform_mesh(ns)
        shp = tuple(ns[::-1])
        u, rhs = rand_field(shp, 100 + c), rand_field(shp, 200 + c)
        S = hip.MGSolver(ns, mesh, bcs)
        if lap:
            S.zero_rhs()
        else:
            S.upload(1, hip.BUF_RHS, rhs)
        S.upload(1, hip.BUF_U, u)
        S.op(hip.OP_RELAX_COLOR, 1, nsw)
        S.op(hip.OP_RESIDUAL, 1)
        a, ra = S.download(1, hip.BUF_U), S.download(1, hip.BUF_R)
        S.upload(1, hip.BUF_U, u)
        S.op(hip.OP_RELAX_FUSED, 1, nsw)
        assert np.array_equal(a, S.download(1, hip.BUF_U)), (ns, bcs, nsw, lap)
        S.upload(1, hip.BUF_U, u)
        S.upload(1, hip.BUF_R, np.full(shp, np.nan))
        S.op(hip.OP_RELAX_RES_FUSED, 1, nsw)
        assert np.array_equal(a, S.download(1, hip.BUF_U)), (ns, bcs, nsw, lap)
        assert np.array_equal(ra, S.download(1, hip.BUF_R)), (ns, bcs, nsw, lap)
        S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ns,nranks,levels", (([128, 64, 160], 2, 0), ([64, 64, 256], 4, 2), ([128, 96, 192], 3, 0),
                                             ([128, 64, 256], 2, 3)), ids=str)
def test_slab_world_mixed_precision_bitwise(hip, ns, nranks, levels):
    """mixed precision on z-slabs (ndsm_hip_world_set_precision; BASELINE config[4]): fp64 residual, fp32
    correction V-cycle with the level-1 halo exchange, restriction and prolongation in fp32 - the
    single-domain mixed mode cut along z.  Loop-back world vs the single-domain mixed solver: du history,
    cycle count and solution bits; and the mode really is on (its iterates differ from the fp64 ones)."""
    if levels:
        os.environ["NDSM_HIP_DIST_LEVELS"] = str(levels)
    try:
        mesh = uniform_mesh(ns)
        shp = tuple(ns[::-1])
        u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
        for bcs, lap in (("NDDNDD", True), ("DDNDDN", False)):
            S = hip.MGSolver(ns, mesh, bcs)
            W = hip.World(ns, mesh, bcs, nranks)
            W64 = hip.World(ns, mesh, bcs, nranks)
            assert S.set_precision(2) and W.set_precision(2)
            if levels:
                assert W.dist_levels == levels
            S.upload(1, hip.BUF_U, u)
            for X in (W, W64):
                X.upload(hip.BUF_U, u)
            if lap:
                for X in (S, W, W64):
                    X.zero_rhs()
            else:
                S.upload(1, hip.BUF_RHS, rhs)
                for X in (W, W64):
                    X.upload(hip.BUF_RHS, rhs)
            a = S.solve(vc_tol=1e-9, nmax=6, hist_len=8)
            b = W.solve(vc_tol=1e-9, nmax=6, hist_len=8)
            c = W64.solve(vc_tol=1e-9, nmax=6, hist_len=8)
            assert (a[0], a[2]) == (b[0], b[2]) and list(a[3]) == list(b[3]), (bcs, list(a[3]), list(b[3]))
            ub = W.download(hip.BUF_U)
            assert np.array_equal(S.download(1, hip.BUF_U), ub), bcs
            u64 = W64.download(hip.BUF_U)
            assert not np.array_equal(ub, u64) and np.abs(ub - u64).max() <= 1e-6 * np.abs(u64).max(), bcs
            assert list(b[3]) != list(c[3])
            for X in (S, W, W64):
                X.close()
    finally:
        os.environ.pop("NDSM_HIP_DIST_LEVELS", None)


@pytest.mark.gpu
def test_world_precision_and_distributed_entry_argument_handling(hip):
    """mixed precision is refused (0, fp64 stays, same bits) where a slab is out of the fp32 kernels' reach;
    the distributed pipeline entry with nranks = 1 is ndsm_vector_solve, bad ranks come back as codes"""
    import ndsm_amd
    ns = [33, 40, 64]                                  # odd nx, < 64 points per row: no fp32 kernels
    mesh = uniform_mesh(ns)
    u = rand_field(tuple(ns[::-1]), 5)
    W, W2 = hip.World(ns, mesh, "NDDNDD", 2), hip.World(ns, mesh, "NDDNDD", 2)
    assert W.set_precision(1) is False
    with pytest.raises(hip.NdsmHipError):
        W.set_precision(7)
    for X in (W, W2):
        X.upload(hip.BUF_U, u)
        X.zero_rhs()
    a, b = W.solve(nmax=3, hist_len=4), W2.solve(nmax=3, hist_len=4)
    assert list(a[3]) == list(b[3]) and np.array_equal(W.download(hip.BUF_U), W2.download(hip.BUF_U))
    W.close()
    W2.close()
    x, y, z, A1, b1 = analytic_case([24, 20, 28])
    ierr, A, B = ndsm_amd.vector_potential(x, y, z, b1.copy())
    ierr1, As, Bs = ndsm_amd.vector_potential_slab(x, y, z, b1, 0, 1)
    assert ierr == ierr1 and np.array_equal(A, As) and np.array_equal(B, Bs)
    with pytest.raises(hip.NdsmHipError):
        ndsm_amd.vector_potential_slab(x, y, z, b1, 3, 2)          # rank >= nranks
    with pytest.raises(hip.NdsmHipError):
        ndsm_amd.vector_potential_slab(x, y, z, b1[:, :14], 0, 2)  # no communicator in this process


@pytest.mark.gpu
def test_random_slab_worlds(hip):
    """seeded random shapes, 2..8 slabs, 1..3 distributed levels, exchange overlap on or off, random ms and
    face letters: three solve-loop cycles of the loop-back world return the single-domain solver's du
    history and bits (scripts/fuzz_world.py)"""
    rng = np.random.default_rng(20260103)
    done = 0
    try:
        while done < 12:
            nr = int(rng.integers(2, 9))
            ns = [int(rng.integers(16, 160)), int(rng.integers(16, 120)), int(rng.integers(16, 60)) * nr]
            lv = int(rng.integers(1, 4))
            bcs = "".join(rng.choice(["D", "N"]) for _ in range(6))
            if bcs == "NNNNNN":
                bcs = "DNNNNN"
            ms = int(rng.integers(1, 6))
            os.environ["NDSM_HIP_DIST_LEVELS"] = str(lv)
            os.environ["NDSM_HIP_OVERLAP"] = str(int(rng.integers(0, 2)))
            mesh = uniform_mesh(ns)
            shp = tuple(ns[::-1])
            u, rhs = rand_field(shp, 100 + done), rand_field(shp, 200 + done)
            try:
                W = hip.World(ns, mesh, bcs, nr, ms=ms)
            except hip.NdsmHipError:
                continue          # the shape cannot be cut that way
            S = hip.MGSolver(ns, mesh, bcs, ms=ms)
            S.upload(1, hip.BUF_U, u)
            S.upload(1, hip.BUF_RHS, rhs)
            W.upload(hip.BUF_U, u)
            W.upload(hip.BUF_RHS, rhs)
            r1 = S.solve(vc_tol=1e-10, nmax=3, hist_len=8)
            r2 = W.solve(vc_tol=1e-10, nmax=3, hist_len=8)
            assert r1[2] == r2[2] and list(r1[3]) == list(r2[3]), (ns, nr, lv, bcs, ms)
            assert np.array_equal(S.download(1, hip.BUF_U), W.download(hip.BUF_U)), (ns, nr, lv, bcs, ms)
            S.close()
            W.close()
            done += 1
    finally:
        os.environ.pop("NDSM_HIP_DIST_LEVELS", None)
        os.environ.pop("NDSM_HIP_OVERLAP", None)


@pytest.mark.gpu
def test_full_size_config4_loopback(hip):
    """BASELINE config[3] shape (1024 x 1024 x 512, 4 GiB per array) cut into 8 z-slabs - loop-back world,
    distributed levels by the default rule (two here), halo exchange behind the interior planes - against
    the single-domain solver: one V-cycle, bit for bit."""
    ns = [1024, 1024, 512]
    dx = 1.0 / (ns[0] - 1)
    mesh = [np.arange(n) * dx for n in ns]
    rng = np.random.default_rng(11)
    az, by, cx = rng.uniform(-1, 1, ns[2]), rng.uniform(-1, 1, ns[1]), rng.uniform(-1, 1, ns[0])
    u = az[:, None, None] * by[None, :, None] + cx[None, None, :]
    W = hip.World(ns, mesh, "NDDNDD", 8)
    assert W.dist_levels == 2
    W.upload(hip.BUF_U, u)
    W.zero_rhs()
    W.vcycle(1)
    b = W.download(hip.BUF_U)
    W.close()
    S = hip.MGSolver(ns, mesh, "NDDNDD")
    S.upload(1, hip.BUF_U, u)
    S.zero_rhs()
    S.vcycle(1)
    a = S.download(1, hip.BUF_U)
    S.close()
    assert np.array_equal(a, b)


@pytest.mark.gpu
def test_beyond_int32_points_loopback(hip):
    """2048 x 2048 x 520 = 2.18e9 points (> 2^31; 16 GiB per array - BASELINE config[4]'s plane size,
    half its depth; scripts/check_c5_size.py runs the full 2^32-point grid the same way): one V-cycle of
    the single-domain solver, whose linear indices leave 32-bit range, against the loop-back world of 8
    z-slabs, whose do not - bit for bit.  Needs ~50 GiB of host memory and ~100 GB of HBM."""
    with open("/proc/meminfo") as f:
        avail = [int(l.split()[1]) for l in f if l.startswith("MemAvailable")][0] / 2**20
    if avail < 80:
        pytest.skip(f"only {avail:.0f} GiB of host memory available")
    ns = [2048, 2048, 520]
    dx = 1.0 / (ns[0] - 1)
    mesh = [np.arange(n) * dx for n in ns]
    rng = np.random.default_rng(12)
    plane = rng.uniform(-1, 1, (ns[1], ns[0]))
    zf = np.cos(np.arange(ns[2]) * 0.37) + 0.01 * np.arange(ns[2])
    u = np.empty((ns[2], ns[1], ns[0]))
    for k in range(ns[2]):
        np.multiply(plane, zf[k], out=u[k])
        u[k, (k * 7) % ns[1]] += 0.5
    S = hip.MGSolver(ns, mesh, "DNDDND")
    S.upload(1, hip.BUF_U, u)
    S.zero_rhs()
    S.vcycle(1)
    a = S.download(1, hip.BUF_U)
    S.close()
    W = hip.World(ns, mesh, "DNDDND", 8)
    W.upload(hip.BUF_U, u)
    W.zero_rhs()
    W.vcycle(1)
    b = W.download(hip.BUF_U)
    W.close()
    assert np.isfinite(a).all() and np.array_equal(a, b)


@pytest.mark.gpu
def test_baseline_config0_three_level_cycle(hip, port):
    """BASELINE config[0]: 64^3 Poisson, 3-level V-cycle (additive option slot get_iopt_ngrids; the
    coarsest grid is then 16^3 = 4096 points, beyond the single-workgroup coarse kernel, so the
    host-driven exact-solve loop runs): whole solve against the oracle with the same level cap -
    solution bits, du history, V-cycle count, coarse sweep count."""
    ns = [64, 64, 64]
    mesh = uniform_mesh(ns)
    us, rhs = manufactured_poisson(mesh, "NDDNDD")
    ierr, u, du, hist, nc = hip.poisson_solve(np.zeros_like(us), rhs, mesh, "NDDNDD", ngrids=3, hist_len=64)
    ierr2, u2, du2, hist2, nc2, sw = port.solve_bvp(np.zeros_like(us), rhs, mesh, "NDDNDD", ngrids=3, hist_len=64)
    assert ierr == ierr2 == 0 and nc == nc2
    assert list(hist) == list(hist2[:nc2])
    assert np.array_equal(u, u2)


@pytest.mark.gpu
def test_baseline_config1_six_level_cycle(hip):
    """BASELINE config[1]: 256^3 Poisson fp64, 6-level V-cycle (coarsest 8^3): converges at the V-cycle's
    rate to the manufactured solution's O(h^2) error, and the level cap is honoured"""
    ns = [256, 256, 256]
    mesh = uniform_mesh(ns)
    us, rhs = manufactured_poisson(mesh, "NDDNDD")
    S = hip.MGSolver(ns, mesh, "NDDNDD", ngrids=6)
    assert S.ngrids == 6 and tuple(S.shapes[-1]) == (8, 8, 8)
    S.close()
    ierr, u, du, hist, nc = hip.poisson_solve(np.zeros_like(us), rhs, mesh, "NDDNDD", ngrids=6, hist_len=64)
    assert ierr == 0 and du < 1e-10 and nc <= 20
    assert np.abs(u - us).max() < 5e-5
    assert all(hist[i + 1] < 0.5 * hist[i] for i in range(len(hist) - 1))


@pytest.mark.gpu
def test_baseline_config2_full_pipeline_512(hip):
    """BASELINE config[2]: the 512^3 vector-potential solve (six 2-D face solves, three 3-D Laplace
    solves, flux balance, curl) through ndsm_vector_solve at full size: the reference's acceptance
    criterion - errors against the analytic field fall as h^2 (integration_test1.py:157-159; the
    published rows give Ea_max ~ 0.9 h^2, Eb_max ~ 37 h^2) - and B's normal component on the faces
    is reproduced"""
    import ndsm_amd
    n = 512
    x, y, z, A1, b1 = analytic_case(n)
    ierr, A, B = ndsm_amd.vector_potential(x, y, z, b1)
    assert ierr == 0
    h = x[1] - x[0]
    ea = np.sqrt(((A1 - A) ** 2).sum(axis=0)).max()
    eb = np.sqrt(((b1 - B) ** 2).sum(axis=0)).max()
    assert ea < 2.0 * h * h and eb < 60.0 * h * h, (ea / h ** 2, eb / h ** 2)
    assert np.abs(B[2, 0] - b1[2, 0]).max() < 60.0 * h * h        # Bz on the lower z face


# ---------------------------------------------------------------------------
# The tile configurations of the benchmarked grids (>= 64 M points: `big` in smooth_fused.hip's
# launch_fused_t - <2,136,30,1024> under its level-1 symbol, <1,132,31,1024> plain and with the metric)
# against an INDEPENDENT implementation: forced onto oracle-sized grids, and at 512^3 itself.
# ---------------------------------------------------------------------------
@pytest.fixture()
def big_tiles(hip):
    L = hip.load_library()
    L.ndsm_hip_debug_fused_cfg(0, 0, 0, 0, 1)
    yield
    L.ndsm_hip_debug_fused_cfg(0, 0, 0, 0, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", ([256, 192, 160], [200, 100, 120], [161, 120, 115]), ids=_tag)
def test_large_level_tiles_forced_vs_oracle(hip, port, big_tiles, ns):
    """the >= 64 M-point tile choices on grids the oracle handles in seconds: five sweeps (2 + 2 + 1: the
    level-1 two-sweep symbol and the big one-sweep tile), general and declared-zero rhs, then three
    solve-loop cycles (sweep + metric on the big one-sweep tile) - solution bits and du history"""
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    zero = np.zeros(shp)
    bcs = "NDDNDD"
    S = hip.MGSolver(ns, mesh, bcs)
    for lap in (False, True):
        S.upload(1, hip.BUF_U, u)
        if lap:
            S.zero_rhs()
        else:
            S.upload(1, hip.BUF_RHS, rhs)
        S.op(hip.OP_RELAX_FUSED, 1, 5)
        want = u
        for _ in range(5):
            want = port.relax3d(want, zero if lap else rhs, mesh, bcs)
        assert np.array_equal(S.download(1, hip.BUF_U), want), lap
        S.upload(1, hip.BUF_U, u)
        S.op(hip.OP_RELAX_FUSED, 1, 1)                    # the one-sweep tile alone
        assert np.array_equal(S.download(1, hip.BUF_U), port.relax3d(u, zero if lap else rhs, mesh, bcs)), lap
    S.close()
    for lap in (True, False):
        r = zero if lap else rhs * 10.0
        ie2, u2, du2, h2, nc2, _sw = port.solve_bvp(u.copy(), r, mesh, bcs, ms=5, nmax=3, hist_len=8)
        S = hip.MGSolver(ns, mesh, bcs, ms=5)
        if lap:
            S.zero_rhs()
        else:
            S.upload(1, hip.BUF_RHS, r)
        S.upload(1, hip.BUF_U, u)
        ie, du, nc, h = S.solve(vc_tol=1e-10, nmax=3, hist_len=8)
        got = S.download(1, hip.BUF_U)
        S.close()
        assert nc == nc2 == 3 and list(h) == list(h2[:3]), (lap, list(h), list(h2[:3]))
        assert np.array_equal(got, u2), lap


@pytest.mark.gpu
def test_benchmarked_512_kernels_vs_oracle(hip, port):
    """BASELINE config[2]'s grid itself (512^3 = 134 M points, where launch_fused_t takes the big tiles by
    its own rule): the launches bench.py times against the ORACLE - five fused sweeps with a general rhs
    (two-sweep level-1 launch x2 + big one-sweep tile), the residual, and - the timed step itself - one
    pass of the solve loop on the Ax Laplace problem (two-sweep Laplace launches, sweep + residual,
    streamed restriction, correction folded into the post-smoothing, sweep + metric on the big tile,
    levels 2-8): du and solution bits."""
    import bench
    n = 512
    ns = [n, n, n]
    shp = (n, n, n)
    bcs = "NDDNDD"
    mesh, u0 = bench.boundary_problem(n)
    rhs = rand_field(shp, 2113)
    u = rand_field(shp, 2112)
    S = hip.MGSolver(ns, mesh, bcs)
    S.upload(1, hip.BUF_U, u)
    S.upload(1, hip.BUF_RHS, rhs)
    S.op(hip.OP_RELAX_FUSED, 1, 5)
    S.op(hip.OP_RESIDUAL, 1)
    got, gotr = S.download(1, hip.BUF_U), S.download(1, hip.BUF_R)
    want = u
    for _ in range(5):
        want = port.relax3d(want, rhs, mesh, bcs, inplace=want is not u)
    assert np.array_equal(got, want)
    assert np.array_equal(gotr, port.residual3d(want, rhs, mesh, bcs))
    del got, gotr, want, u, rhs
    # the timed step: solve-loop pass on the Laplace problem
    S.upload(1, hip.BUF_U, u0)
    S.zero_rhs()
    ie, du, nc, h = S.solve(vc_tol=0.0, nmax=1, hist_len=4)
    got = S.download(1, hip.BUF_U)
    S.close()
    ie2, u2, du2, h2, nc2, _sw = port.solve_bvp(u0, np.zeros(shp), mesh, bcs, ms=5, vc_tol=0.0, nmax=1, hist_len=4)
    assert nc == nc2 == 1 and list(h) == list(h2[:1]), (list(h), list(h2))
    assert np.array_equal(got, u2)


@pytest.mark.gpu
def test_benchmarked_512_fused_vs_colour_kernels(hip):
    """512^3, second independent check that needs no CPU time: the fused launches (big tiles) against the
    thread-per-point colour passes + stand-alone residual and metric kernels (which the small-shape tests
    pin to the oracle and the reference's golden vectors), general and zero rhs, 1 / 2 / 5 sweeps"""
    n = 512
    ns = [n, n, n]
    shp = (n, n, n)
    mesh = uniform_mesh(ns)
    u, rhs = rand_field(shp, 5), rand_field(shp, 6)
    for bcs in ("NDDNDD", "DDNDDN"):
        S = hip.MGSolver(ns, mesh, bcs)
        for lap in (False, True):
            if lap:
                S.zero_rhs()
            else:
                S.upload(1, hip.BUF_RHS, rhs)
            for nsw in (1, 2, 5):
                S.upload(1, hip.BUF_U, u)
                S.op(hip.OP_RELAX_COLOR, 1, nsw)
                S.op(hip.OP_RESIDUAL, 1)
                uw, rw = S.download(1, hip.BUF_U), S.download(1, hip.BUF_R)
                S.upload(1, hip.BUF_U, u)
                S.op(hip.OP_RELAX_RES_FUSED, 1, nsw)
                assert np.array_equal(S.download(1, hip.BUF_U), uw), (bcs, lap, nsw)
                assert np.array_equal(S.download(1, hip.BUF_R), rw), (bcs, lap, nsw)
                S.upload(1, hip.BUF_U, u)
                S.op(hip.OP_RELAX_FUSED, 1, nsw)
                assert np.array_equal(S.download(1, hip.BUF_U), uw), (bcs, lap, nsw)
        S.close()


@pytest.mark.gpu
def test_baseline_config1_vs_oracle(hip, port):
    """BASELINE config[1] against the oracle, not only through properties: 256^3 Poisson, ngrids = 6 -
    the whole solve's du history, cycle count, coarse sweep count and solution bits"""
    ns = [256, 256, 256]
    mesh = uniform_mesh(ns)
    us, rhs = manufactured_poisson(mesh, "NDDNDD")
    ierr, u, du, hist, nc = hip.poisson_solve(np.zeros_like(us), rhs, mesh, "NDDNDD", ngrids=6, hist_len=64)
    ierr2, u2, du2, hist2, nc2, _sw = port.solve_bvp(np.zeros_like(us), rhs, mesh, "NDDNDD", ngrids=6, hist_len=64)
    assert ierr == ierr2 == 0 and nc == nc2
    assert list(hist) == list(hist2[:nc2])
    assert du == du2
    assert np.array_equal(u, u2)


@pytest.mark.gpu
def test_full_size_config4_loopback_poisson(hip):
    """BASELINE config[3] as written - a POISSON problem: 1024 x 1024 x 512 with a non-zero right-hand
    side (the general-rhs slab kernels, stand-alone prolongation), 8 z-slabs in loop-back against the
    single-domain solver: one V-cycle and the convergence metric, bit for bit."""
    ns = [1024, 1024, 512]
    dx = 1.0 / (ns[0] - 1)
    mesh = [np.arange(n) * dx for n in ns]
    rng = np.random.default_rng(13)
    az, by, cx = rng.uniform(-1, 1, ns[2]), rng.uniform(-1, 1, ns[1]), rng.uniform(-1, 1, ns[0])
    u = az[:, None, None] * by[None, :, None] + cx[None, None, :]
    rhs = (by[None, :, None] * cx[None, None, :]) * az[:, None, None] * 50.0 + 1.0
    W = hip.World(ns, mesh, "NDDNDD", 8)
    W.upload(hip.BUF_U, u)
    W.upload(hip.BUF_RHS, rhs)
    ie, du_w, nc, hw = W.solve(vc_tol=0.0, nmax=1, hist_len=2)
    b = W.download(hip.BUF_U)
    W.close()
    S = hip.MGSolver(ns, mesh, "NDDNDD")
    S.upload(1, hip.BUF_U, u)
    S.upload(1, hip.BUF_RHS, rhs)
    del u, rhs
    ie, du_s, nc, hs = S.solve(vc_tol=0.0, nmax=1, hist_len=2)
    a = S.download(1, hip.BUF_U)
    S.close()
    assert list(hw) == list(hs) and du_w == du_s
    assert np.array_equal(a, b)


# ---------------------------------------------------------------------------
# the face phase on the device, the persistent vector-potential context
# ---------------------------------------------------------------------------
def _vp_cases():
    x, y, z, _A1, b = analytic_case([40, 33, 36])
    bn = b + 0.3 * np.random.default_rng(5).uniform(-1, 1, b.shape)       # unbalanced fluxes
    return x, y, z, b, bn


@pytest.mark.gpu
def test_device_face_phase_equals_host_face_phase(hip):
    """B.n extraction / fluxes / right-hand sides / A_t / face writes as device kernels (faces.hip) against
    the host face phase (vecpot_faces, the code the distributed driver's rank 0 runs; selected with
    NDSM_HIP_HOST_FACES): the same bits in A and B - balanced and unbalanced boundary data, non-zero
    initial guess, both flux-balance orders"""
    import ndsm_amd
    x, y, z, b, bn = _vp_cases()
    a0 = np.random.default_rng(6).uniform(-1, 1, b.shape)
    V = ndsm_amd.VecPot(x, y, z)
    for field, guess, flx in ((b, None, False), (bn, None, False), (bn, a0, False), (bn, a0, True)):
        os.environ["NDSM_HIP_HOST_FACES"] = "1"
        try:
            i1, A1, B1 = V.solve(field, a_init=guess, flxcrl=flx)
        finally:
            os.environ.pop("NDSM_HIP_HOST_FACES", None)
        i2, A2, B2 = V.solve(field, a_init=guess, flxcrl=flx)
        i3, A3, B3 = V.solve(field, a_init=guess, flxcrl=flx, device=True)      # device-resident entry
        assert i1 == i2 == i3
        assert np.array_equal(A1, A2) and np.array_equal(B1, B2), (guess is not None, flx)
        assert np.array_equal(A2, A3) and np.array_equal(B2, B3), (guess is not None, flx)
    V.close()


@pytest.mark.gpu
def test_vecpot_context_reuse_and_cache(hip, port):
    """the persistent context: (a) a handle solves different boundary data one after the other and
    returns what fresh ndsm_vector_solve calls return; (b) ndsm_vector_solve's internal cache - same mesh
    again, another mesh, the first mesh again, NDSM_HIP_NO_CACHE - never changes a bit; (c) the oracle
    bound of the pipeline still holds"""
    import ndsm_amd
    x, y, z, b, bn = _vp_cases()
    x2, y2, z2, _A, b2 = analytic_case([24, 40, 28])
    os.environ["NDSM_HIP_NO_CACHE"] = "1"
    try:
        ref = [ndsm_amd.vector_potential(x, y, z, f.copy()) for f in (b, bn)]
        ref2 = ndsm_amd.vector_potential(x2, y2, z2, b2.copy())
    finally:
        os.environ.pop("NDSM_HIP_NO_CACHE", None)
    V = ndsm_amd.VecPot(x, y, z)
    for k in (0, 1, 0):
        ie, A, B = V.solve((b, bn)[k])
        assert ie == ref[k][0] and np.array_equal(A, ref[k][1]) and np.array_equal(B, ref[k][2]), k
    V.close()
    for k, (xx, yy, zz, ff, want) in enumerate(((x, y, z, b, ref[0]), (x, y, z, bn, ref[1]), (x2, y2, z2, b2, ref2),
                                                (x, y, z, b, ref[0]))):
        ie, A, B = ndsm_amd.vector_potential(xx, yy, zz, ff.copy())
        assert ie == want[0] and np.array_equal(A, want[1]) and np.array_equal(B, want[2]), k
    ierr2, A2, B2, _io, _ro = port.vector_potential(x, y, z, b)
    assert np.abs(ref[0][1] - A2).max() <= 1e-12 * np.abs(A2).max()
    h = x[1] - x[0]
    assert np.abs(ref[0][2] - B2).max() <= 1e-12 * np.abs(A2).max() * 4 / h


@pytest.mark.gpu
@pytest.mark.parametrize("ns,meshf", _meshes(([64, 64, 64], [33, 22, 27], [40, 24, 32], [100, 37, 51], [128, 128, 128],
                                              [144, 144, 72], [22, 22, 22], [40, 136, 72]), ([33, 22, 27],)))
def test_tail_cycle_bitwise(hip, ns, meshf):
    """the bottom of the V-cycle as ONE single-workgroup launch (tail.hip: every level of <= 6144 points
    resident in LDS - sweeps, residual, restriction, coarsest-grid solve, interpolation) against the same
    levels run kernel by kernel (switched through the development hook): V-cycles from random data, every
    level's u and rhs afterwards, the coarsest-grid sweep counters, the du history of a solve - bit for bit;
    max and mean form of the coarsest grid's stop test, ms = 1 ... 5, an unconverged coarsest solve"""
    L = hip.load_library()
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 7), rand_field(shp, 8)
    ran = 0

    def run(bcs, ms, du_max, nmax_exact):
        S = hip.MGSolver(ns, mesh, bcs, ms=ms, du_max=du_max, nmax_exact=nmax_exact)
        S.upload(1, hip.BUF_U, u)
        S.upload(1, hip.BUF_RHS, rhs)
        S.vcycle(2)
        lev = [(S.download(l, hip.BUF_U), S.download(l, hip.BUF_RHS)) for l in range(1, S.ngrids + 1)]
        info = S.info()
        ie, du, nc, h = S.solve(vc_tol=1e-9, nmax=6, hist_len=8)
        out = S.download(1, hip.BUF_U)
        sizes = [int(np.prod(sh)) for sh in S.shapes]
        S.close()
        return lev, info, (ie, du, nc, list(h)), out, sizes

    try:
        for bcs, ms, du_max, nmax_exact in (("NDDNDD", 5, True, 10000), ("DNDDND", 5, False, 10000), ("DDNDDN", 3, True, 10000),
                                            ("NNNNND", 1, False, 10000), ("DDDDDD", 2, True, 3), ("NDNDND", 4, True, 10000)):
            L.ndsm_hip_debug_tail(0)
            want = run(bcs, ms, du_max, nmax_exact)
            L.ndsm_hip_debug_tail(1)
            got = run(bcs, ms, du_max, nmax_exact)
            sizes = want[4]
            if len(sizes) >= 3 and sizes[-2] <= 6144:
                ran += 1                      # (at least the two coarsest levels qualify)
            for l, (a, b) in enumerate(zip(want[0], got[0]), start=1):
                assert np.array_equal(a[0], b[0]), (bcs, "u", l)
                assert np.array_equal(a[1], b[1]), (bcs, "rhs", l)
            assert want[1] == got[1], (bcs, want[1], got[1])
            assert want[2] == got[2], (bcs, want[2], got[2])
            assert np.array_equal(want[3], got[3]), bcs
            if nmax_exact == 3:
                assert want[1][1] > 0           # the coarsest solves did run out of sweeps
        assert ran > 0
    finally:
        L.ndsm_hip_debug_tail(1)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", ([64, 64], [128, 96], [40, 136], [33, 22], [512, 512], [70, 9]), ids=_tag)
def test_tail_cycle_bitwise_2d(hip, ns):
    """the same for the 2-D hierarchies of the face solves (five-point expressions; on all-Neumann problems the
    mean is subtracted after every sweep, summed in rbgs2_small's order, and inside the coarsest-grid solve in
    solve_exact_k's): V-cycles, every level, counters and a solve history with the single launch switched off
    and on - bit for bit"""
    L = hip.load_library()
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 17), rand_field(shp, 18)
    rhs = rhs - rhs.mean()

    def run(bcs, ms, du_max):
        S = hip.MGSolver(ns, mesh, bcs, ms=ms, du_max=du_max)
        S.upload(1, hip.BUF_U, u)
        S.upload(1, hip.BUF_RHS, rhs)
        S.vcycle(2)
        lev = [(S.download(l, hip.BUF_U), S.download(l, hip.BUF_RHS)) for l in range(1, S.ngrids + 1)]
        info = S.info()
        res = S.solve(vc_tol=1e-9, nmax=6, hist_len=8)
        out = S.download(1, hip.BUF_U)
        S.close()
        return lev, info, (res[0], res[1], res[2], list(res[3])), out

    try:
        for bcs, ms, du_max in (("NNNN", 5, True), ("NNNN", 2, False), ("NDDN", 5, True), ("DDDD", 3, False), ("DNND", 1, True)):
            L.ndsm_hip_debug_tail(0)
            want = run(bcs, ms, du_max)
            L.ndsm_hip_debug_tail(1)
            got = run(bcs, ms, du_max)
            for l, (a, b) in enumerate(zip(want[0], got[0]), start=1):
                assert np.array_equal(a[0], b[0]), (bcs, "u", l)
                assert np.array_equal(a[1], b[1]), (bcs, "rhs", l)
            assert want[1] == got[1], (bcs, want[1], got[1])
            assert want[2] == got[2], (bcs, want[2], got[2])
            assert np.array_equal(want[3], got[3]), bcs
    finally:
        L.ndsm_hip_debug_tail(1)


@pytest.mark.gpu
def test_face_solves_side_by_side_and_replayed_bitwise(hip):
    """the six 2-D face solves of ndsm_vector_solve: one after the other (NDSM_HIP_FACE_LANES=0), in lockstep on
    six streams with every launch enqueued (NDSM_HIP_NO_GRAPHS=1), and in lockstep with each solve's V-cycle +
    metric replayed as a recorded graph from its second round on (the default for faces of >= 32768 points) -
    the same A and B bit for bit; so is a repeated call (the recorded graphs are kept with the cached context)
    and a call after the options changed (ms, the coarsest-grid stop test: the graphs are recorded again)"""
    import ndsm_amd
    x, y, z, _A1, b1 = analytic_case([200, 200, 184])      # faces of 200 x 200 and 200 x 184 points

    def call(**kw):
        ierr, A, B = ndsm_amd.vector_potential(x, y, z, b1, **kw)
        assert ierr == 0
        return A, B

    keep = {k: os.environ.get(k) for k in ("NDSM_HIP_FACE_LANES", "NDSM_HIP_NO_GRAPHS")}
    try:
        os.environ["NDSM_HIP_FACE_LANES"] = "0"
        want = call()
        want3 = call(ms=3, mean=True)
        os.environ["NDSM_HIP_FACE_LANES"] = "1"
        os.environ["NDSM_HIP_NO_GRAPHS"] = "1"
        got = call()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        os.environ.pop("NDSM_HIP_NO_GRAPHS")
        for _ in range(2):                                   # records, then replays what the first call recorded
            got = call()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        got3 = call(ms=3, mean=True)                         # other sweeps per level, other stop test: recorded anew
        assert np.array_equal(got3[0], want3[0]) and np.array_equal(got3[1], want3[1])
        got = call()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        os.environ["NDSM_HIP_FAKE_GRAPH_FAILURE"] = "1"      # recording fails: the rounds are enqueued as usual
        got3 = call(ms=2)
        os.environ.pop("NDSM_HIP_FAKE_GRAPH_FAILURE")
        os.environ["NDSM_HIP_FACE_LANES"] = "0"
        want3 = call(ms=2)
        assert np.array_equal(got3[0], want3[0]) and np.array_equal(got3[1], want3[1])
    finally:
        os.environ.pop("NDSM_HIP_FAKE_GRAPH_FAILURE", None)
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.gpu
def test_baseline_config4_full_grid_mixed_component(hip):
    """BASELINE config[4]'s grid at FULL size - 2048 x 2048 x 1024 = 2^32 points, 32 GiB per fp64 array - and
    in its precision mode (fp32 smoother / fp64 residual): two solve-loop cycles of ONE component (Ay's
    boundary letters) in the mixed-precision mode, single domain against the 8-slab loop-back world - du
    history and solution bit for bit.  (The vector-potential driver around it needs A, B and a hierarchy at
    once, 3 x 32 + 3 x 32 + ~180 GiB: that is what the eight GPUs are for; on one GPU the per-component
    solve is the part that fits.)  Needs ~130 GiB of host memory and ~230 GiB of HBM."""
    with open("/proc/meminfo") as f:
        avail = [int(l.split()[1]) for l in f if l.startswith("MemAvailable")][0] / 2**20
    if avail < 160:
        pytest.skip(f"only {avail:.0f} GiB of host memory available")
    ns = [2048, 2048, 1024]
    dx = 1.0 / (ns[0] - 1)
    mesh = [np.arange(n) * dx for n in ns]
    rng = np.random.default_rng(14)
    plane = rng.uniform(-1, 1, (ns[1], ns[0]))
    zf = np.cos(np.arange(ns[2]) * 0.37) + 0.01 * np.arange(ns[2])
    u = np.empty((ns[2], ns[1], ns[0]))
    for k in range(ns[2]):
        np.multiply(plane, zf[k], out=u[k])
        u[k, (k * 7) % ns[1]] += 0.5
    try:
        S = hip.MGSolver(ns, mesh, "DNDDND")
    except hip.NdsmHipError as exc:
        pytest.skip(f"the single-domain hierarchy does not fit this GPU: {exc}")
    assert S.set_precision(1)
    S.upload(1, hip.BUF_U, u)
    S.zero_rhs()
    ie, du_s, nc, hs = S.solve(vc_tol=0.0, nmax=2, hist_len=4)
    a = S.download(1, hip.BUF_U)
    S.close()
    W = hip.World(ns, mesh, "DNDDND", 8)
    assert W.set_precision(1)
    W.upload(hip.BUF_U, u)
    del u
    W.zero_rhs()
    ie, du_w, nc, hw = W.solve(vc_tol=0.0, nmax=2, hist_len=4)
    b = W.download(hip.BUF_U)
    W.close()
    assert list(hs) == list(hw) and len(hs) == 2 and hs[1] < hs[0]
    assert np.isfinite(a).all() and np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", ([5, 4, 6], [17, 23, 19], [64, 20, 33]), ids=_tag)
def test_vecpot_paths_small_and_ragged_shapes(hip, port, ns):
    """the device face phase, the cached context and the small-HBM sequence (NDSM_HIP_LEAN: B takes the
    memory of the destroyed 3-D hierarchy) on tiny, odd and anisotropic boxes: all three return the bits
    of the host face phase, and the oracle's pipeline agrees within the stated bound"""
    import ndsm_amd
    x, y, z, _A1, b = analytic_case(ns)
    b = b + 0.1 * np.random.default_rng(3).uniform(-1, 1, b.shape)
    os.environ["NDSM_HIP_HOST_FACES"] = "1"
    os.environ["NDSM_HIP_NO_CACHE"] = "1"
    try:
        i0, A0, B0 = ndsm_amd.vector_potential(x, y, z, b.copy())
    finally:
        os.environ.pop("NDSM_HIP_HOST_FACES", None)
        os.environ.pop("NDSM_HIP_NO_CACHE", None)
    i1, A1, B1 = ndsm_amd.vector_potential(x, y, z, b.copy())
    os.environ["NDSM_HIP_LEAN"] = "1"
    try:
        i2, A2, B2 = ndsm_amd.vector_potential(x, y, z, b.copy())
        i3, A3, B3 = ndsm_amd.vector_potential(x, y, z, b.copy())
    finally:
        os.environ.pop("NDSM_HIP_LEAN", None)
    i4, A4, B4 = ndsm_amd.vector_potential(x, y, z, b.copy())
    for ie, A, B in ((i1, A1, B1), (i2, A2, B2), (i3, A3, B3), (i4, A4, B4)):
        assert ie == i0 and np.array_equal(A, A0) and np.array_equal(B, B0)
    ie, Ao, Bo, _io, _ro = port.vector_potential(x, y, z, b)
    assert ie == i0
    h = x[1] - x[0]
    assert np.abs(A0 - Ao).max() <= 1e-12 * max(np.abs(Ao).max(), 1e-300)
    assert np.abs(B0 - Bo).max() <= 1e-12 * max(np.abs(Ao).max(), 1e-300) * 4 / h


_RESTRICT_FORMS_CHILD = r"""
import hashlib, json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, ndsm_amd
from ndsm_amd import _lib
from golden_inputs import rand_field, uniform_mesh
L = ndsm_amd.load_library(); assert L.ndsm_hip_init(0) == 0
out = {}
for ns, bcs in (([200, 150, 220], "NDDNDD"), ([201, 150, 216], "DNNDDN"), ([320, 140, 150], "DDDDDD")):
    S = _lib.MGSolver(ns, uniform_mesh(ns), bcs)
    S.upload(1, _lib.BUF_R, rand_field(tuple(ns[::-1]), 77))
    S.upload(2, _lib.BUF_U, np.full(S._npshape(2), 3.0))
    S.op(_lib.OP_RESTRICT, 1)
    rc, uc = S.download(2, _lib.BUF_RHS), S.download(2, _lib.BUF_U)
    out["x".join(map(str, ns))] = [hashlib.sha256(rc.tobytes()).hexdigest(), bool(uc.any())]
    S.close()
print(json.dumps(out))
"""


@pytest.mark.gpu
def test_restriction_forms_agree():
    """the three forms of the streamed restriction (restrict_stream.hip: NDSM_RS_VARIANT = 10 fine planes by LDS-DMA +
    schedule + ordered accumulators, the default for fp64 levels with even nx; 8 register-staged with the schedule;
    5 register-staged with the table walk) and the gather kernel (NDSM_HIP_NO_STREAM_RESTRICT) on the same residual
    fields - even and odd nx, three BC sets: the same coarse right-hand side bit for bit, coarse u zeroed
    (nrestrict, ndsm_interp.f90:263-290; ndsm_multigrid_core.f90:557-558).  The variant is read once per process:
    one child per form."""
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for tag, env in (("gather", {"NDSM_HIP_NO_STREAM_RESTRICT": "1"}), ("dma", {"NDSM_RS_VARIANT": "10"}),
                     ("staged+schedule", {"NDSM_RS_VARIANT": "8"}), ("staged+walk", {"NDSM_RS_VARIANT": "5"})):
        e = dict(os.environ, **env)
        if tag != "gather":
            e.pop("NDSM_HIP_NO_STREAM_RESTRICT", None)
        r = subprocess.run([sys.executable, "-c", _RESTRICT_FORMS_CHILD, ROOT], env=e, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, (tag, r.stderr[-2000:])
        res[tag] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    for tag in ("dma", "staged+schedule", "staged+walk"):
        assert res[tag] == res["gather"], (tag, res[tag], res["gather"])
    assert not any(v[1] for v in res["gather"].values())


@pytest.mark.gpu
def test_correction_launch_with_one_tall_chunk(hip, port):
    """the launch that interpolates the coarse-grid correction while it loads (MODE 3) keeps the z tables of
    its chunk in LDS; a chunk taller than that table (a workgroup walking the whole of a tall grid, as on the
    2048 x 2048 x 1024 grid) reads them from global memory instead: forced here with one work item per tile
    on a 96 x 64 x 420 grid, two solve-loop cycles against the oracle"""
    L = hip.load_library()
    ns = [96, 64, 420]
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    u0 = rand_field(shp, 31)
    ie2, u2, du2, h2, nc2, _sw = port.solve_bvp(u0.copy(), np.zeros(shp), mesh, "NDDNDD", ms=5, nmax=2, hist_len=4)
    L.ndsm_hip_debug_fused_cfg(0, 0, 0, 1, -1)        # one work item per tile: a single chunk of 420 planes
    try:
        S = hip.MGSolver(ns, mesh, "NDDNDD", ms=5)
        S.zero_rhs()
        S.upload(1, hip.BUF_U, u0)
        ie, du, nc, h = S.solve(vc_tol=1e-10, nmax=2, hist_len=4)
        got = S.download(1, hip.BUF_U)
        S.close()
    finally:
        L.ndsm_hip_debug_fused_cfg(0, 0, 0, 0, -1)
    assert nc == nc2 == 2 and list(h) == list(h2[:2])
    assert np.array_equal(got, u2)


@pytest.mark.gpu
@pytest.mark.parametrize("ns,meshf", [pytest.param(ns, uniform_mesh, id=f"ns{i}") for i, ns in
                                     enumerate(([136, 130, 140], [131, 140, 134]))] +
                         [pytest.param([136, 130, 140], aniso_mesh, id="aniso-ns0")])
def test_correction_launch_with_rhs_vs_oracle(hip, port, ns, meshf):
    """a Poisson problem (right-hand side in HBM) takes its correction on the one-sweep launch that opens the
    post-smoothing (rbgs3_fused_k<.., S = 1, .., RHS0 = false, MODE = 3>): three solve-loop cycles, even and odd
    nx, several tiles and chunks, against the oracle - field, du history and cycle count
    (ndsm_multigrid_core.f90:593-684 coarse_to_fine followed by :672-675's sweeps)"""
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    u0 = rand_field(shp, 41)
    rhs = rand_field(shp, 42) * 50.0
    ie2, u2, du2, h2, nc2, _sw = port.solve_bvp(u0.copy(), rhs, mesh, "NDDNDD", ms=5, nmax=3, hist_len=4)
    S = hip.MGSolver(ns, mesh, "NDDNDD", ms=5)
    S.upload(1, hip.BUF_RHS, rhs)
    S.upload(1, hip.BUF_U, u0)
    ie, du, nc, h = S.solve(vc_tol=1e-30, nmax=3, hist_len=4)
    got = S.download(1, hip.BUF_U)
    S.close()
    assert nc == nc2 == 3 and list(h) == list(h2[:3])
    assert np.array_equal(got, u2)
