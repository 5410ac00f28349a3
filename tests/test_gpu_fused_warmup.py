"""The fused smoother's edge steps (run with -m gpu on an MI355X).

A workgroup of rbgs3_fused_k walks its z chunk [zs, ze) from NSTG planes below it and runs a stage only
where a stored plane depends on it: in the warm-up steps, the steps the group rounding adds at either end
and the steps whose stage planes lie outside the grid, stages are skipped one by one.  A skipped stage
would have produced a value no needed stage reads, so every result must keep its bits.  The shapes here
are small and flat enough for the edge steps to dominate: [32, 32, 42] is two tiles and six chunks of 7
planes (fewer planes than 2 * NST, chunk starts that are no multiple of the number of step copies).

Every comparison is np.array_equal: there are no tolerances.
"""
import numpy as np
import pytest

from golden_inputs import rand_field, uniform_mesh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


BCS = ("NDDNDD", "DDDDDD", "DDNDDN")      # the last: Neumann mirror faces on z, in the first and the last chunk
TILES = 2                                 # every shape below is one tile in x and two in y, for every fused kernel
CHUNKINGS = (0, TILES, 2 * TILES, 3 * TILES)   # work items: 0 = the planner's own choice


@pytest.mark.parametrize("ns", ([32, 32, 42], [48, 40, 37], [34, 32, 42], [33, 32, 42]), ids=lambda ns: "x".join(map(str, ns)))
def test_forced_fused_launches_vs_colour_passes(hip, ns):
    """forced fused launches (1, 2 and 2 + 2 + 1 sweeps; sweep + residual) return the bits of the colour
    passes (+ residual.hip), which test_kernels3d_bitwise pins to the oracle - general and declared-zero
    rhs, three boundary sets, the planner's chunking and one, two and three work items per tile"""
    L = hip.load_library()
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    for bcs in BCS:
        S = hip.MGSolver(ns, mesh, bcs)
        try:
            for laplace in (False, True):
                if laplace:
                    S.zero_rhs()
                else:
                    S.upload(1, hip.BUF_RHS, rhs)
                want = {}
                for nsw in (1, 2, 3, 5):
                    S.upload(1, hip.BUF_U, u)
                    S.op(hip.OP_RELAX_COLOR, 1, nsw)
                    S.op(hip.OP_RESIDUAL, 1)
                    want[nsw] = (S.download(1, hip.BUF_U), S.download(1, hip.BUF_R))
                for w in CHUNKINGS:
                    L.ndsm_hip_debug_fused_cfg(0, 0, 0, w, -1)
                    try:
                        for nsw in (1, 2, 5):
                            S.upload(1, hip.BUF_U, u)
                            S.op(hip.OP_RELAX_FUSED, 1, nsw)
                            assert np.array_equal(S.download(1, hip.BUF_U), want[nsw][0]), (bcs, laplace, w, nsw)
                        for nsw in (1, 3):
                            S.upload(1, hip.BUF_U, u)
                            S.upload(1, hip.BUF_R, np.full(shp, np.nan))
                            S.op(hip.OP_RELAX_RES_FUSED, 1, nsw)
                            assert np.array_equal(S.download(1, hip.BUF_U), want[nsw][0]), (bcs, laplace, w, nsw)
                            assert np.array_equal(S.download(1, hip.BUF_R), want[nsw][1]), (bcs, laplace, w, nsw)
                    finally:
                        L.ndsm_hip_debug_fused_cfg(0, 0, 0, 0, -1)
        finally:
            S.close()


@pytest.mark.parametrize("ms", (5, 4))
def test_tracked_solve_just_above_2m_points(hip, port, ms):
    """two solve-loop cycles on [161, 120, 115] (level 1 just large enough for the fused launches: the metric
    launch, the correction launch and, on level 2, the general-rhs launches) against the oracle - field, du
    history and cycle count, under the planner's chunking and with three work items per tile"""
    L = hip.load_library()
    ns = [161, 120, 115]
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    u0, rhs = rand_field(shp, 21), rand_field(shp, 22) * 10.0
    for bcs, lap in (("NDDNDD", True), ("DNDDDN", False)):
        r = np.zeros(shp) if lap else rhs
        ie2, u2, du2, h2, nc2, _sw = port.solve_bvp(u0.copy(), r, mesh, bcs, ms=ms, nmax=2, hist_len=8)
        for w in (0, 36):                 # 2 x 6 tiles of the two-sweep launch: three chunks of 39 planes
            L.ndsm_hip_debug_fused_cfg(0, 0, 0, w, -1)
            try:
                S = hip.MGSolver(ns, mesh, bcs, ms=ms)
                if lap:
                    S.zero_rhs()
                else:
                    S.upload(1, hip.BUF_RHS, rhs)
                S.upload(1, hip.BUF_U, u0)
                ie, du, nc, h = S.solve(vc_tol=1e-10, nmax=2, hist_len=8)
                got = S.download(1, hip.BUF_U)
                S.close()
            finally:
                L.ndsm_hip_debug_fused_cfg(0, 0, 0, 0, -1)
            assert nc == nc2 == 2 and list(h) == list(h2[:2]), (bcs, w, list(h), list(h2[:2]))
            assert np.array_equal(got, u2), (bcs, w)
