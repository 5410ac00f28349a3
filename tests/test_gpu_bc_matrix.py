"""Every multigrid kernel family under EVERY boundary letter set (run with -m gpu on an MI355X).

`MGSolver`, `poisson_solve` and `World` take any six letters (lower x, y, z, then upper x, y, z, each D or N): 64 sets
in 3-D, 16 in 2-D.  The hand-written kernels special-case each face - mirrored neighbours, the odd-nx ghost column, the
z range of the first and last chunk, mirror flags per point, single-wave paths chosen by the number of UPDATED points -
so a face can be wrong on one side of one axis only.  Three layers, each pinned to the one above it:

  1. test_oracle_bc_matrix.py (no GPU): the oracle port reproduces the reference under all 64 + 16 sets.
  2. here, "port ->": the colour passes, residual.hip, a V-cycle and a solve against the port, all sets, small shapes.
  3. here, "colour passes ->": every other launch that sweeps against the device's own colour passes (+ residual.hip)
     on the same solver - no oracle cost, so all 64 sets fit; the two large families run the 16 sets of
     golden_inputs.bc_orthogonal_array (every pair of axes sees all 16 combinations of its four letters).

Everything is np.array_equal.  The exceptions are the all-Neumann set AGAINST THE PORT, where the device adds the mean
as a tree and the port in a loop: sweeps take the bound derived in test_gpu_block_smoother.py (mean_sum_bound,
tol_s = 2 tol_(s-1) + 8 (g + 2^-53) V_s), 2-D sweeps the 1e-14 of test_kernels2d.  That bound covers sweeps only, so
the all-Neumann V-CYCLE and SOLVE are not held against the port but, bit for bit, against the same cycle put together
from the single operations on the device (sweeps + residual, restriction, coarsest-grid solve, interpolation), and
the solve against V-cycles one by one; its coarsest-grid solve is held against the port at five sweeps, with the bound.

Every family of layer 3 proves that it ran: it asks ndsm_hip_debug_relax_plan (plan_tools) for the plan of the very
request and asserts the pass kind and instantiation before it compares, and it counts the sets it visited.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import mixed_model as mm
import plan_tools
from golden_inputs import (ALL_BCS_2D, ALL_BCS_3D, BC_MATRIX_2D, BC_MATRIX_3D, aniso_mesh, bc_matrix_case,
                           bc_orthogonal_array, rand_field, uniform_mesh)
from test_gpu_block_smoother import mean_sum_bound
from test_relax_plan_zero_guess import zplan

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ARRAY16 = bc_orthogonal_array()
_PAIRS = ("DD", "DN", "ND", "NN")


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    yield _lib
    L.ndsm_hip_debug_fused_cfg(0, 0, 0, 0, -1)
    L.ndsm_hip_debug_tail(1)
    L.ndsm_hip_debug_zero_guess(1)


def _tag(ns):
    return "x".join(str(n) for n in ns)


def _nn(bcs):
    return set(bcs) == {"N"}


def _plan(ns, nsweeps, bcs, **kw):
    """the planner's answer for a relax call on a whole level of shape ns under the letters bcs"""
    nd = len(ns)
    lb = [int(bcs[d] == "D") for d in range(nd)] + [0] * (3 - nd)
    ub = [ns[d] - 1 - int(bcs[nd + d] == "D") for d in range(nd)] + [0] * (3 - nd)
    p = plan_tools.relax_plan(ns, nsweeps, lb=lb, ub=ub, all_neumann=_nn(bcs), **kw)
    assert p["err"] == 0, (ns, nsweeps, bcs, kw)
    assert sum(q["sweeps"] for q in p["passes"]) == nsweeps
    return p


def _solver(hip, ns, mesh, bcs, rhs, **kw):
    S = hip.MGSolver(ns, mesh, bcs, **kw)
    if rhs is None:
        S.zero_rhs()
    else:
        S.upload(1, hip.BUF_RHS, rhs)
    return S


def _colour(hip, S, u, counts, residual=False):
    """{n: u after n sweeps of the colour passes (, r = rhs - L u of residual.hip)} - the checker of layer 3"""
    want = {}
    for n in counts:
        S.upload(1, hip.BUF_U, u)
        S.op(hip.OP_RELAX_COLOR, 1, n)
        if residual:
            S.op(hip.OP_RESIDUAL, 1)
            want[n] = (S.download(1, hip.BUF_U), S.download(1, hip.BUF_R))
        else:
            want[n] = S.download(1, hip.BUF_U)
    return want


def test_the_set_lists():
    assert len(set(ALL_BCS_3D)) == 64 and len(set(ALL_BCS_2D)) == 16 and len(set(ARRAY16)) == 16
    assert set(ARRAY16) <= set(ALL_BCS_3D) and "NNNNNN" not in ARRAY16
    code = {b: tuple(_PAIRS.index(b[d] + b[3 + d]) for d in range(3)) for b in ARRAY16}
    for a, c in ((0, 1), (0, 2), (1, 2)):                 # strength 2: every pair of axes sees all 16 combinations
        assert len({(v[a], v[c]) for v in code.values()}) == 16


# ---------------------------------------------------------------------------------------------------------------------
# layer 2: port -> colour passes, residual, V-cycle, solve
# ---------------------------------------------------------------------------------------------------------------------
def _vcycle_by_ops(hip, S, ms):
    """one V-cycle from the single operations, level by level (ndsmh_mg.f90, vcycle_levels with the tail launch off)"""
    ng = S.ngrids
    for l in range(1, ng):
        S.op(hip.OP_RELAX_RES, l, ms)
        S.op(hip.OP_RESTRICT, l)
    S.op(hip.OP_EXACT, ng)
    S.op(hip.OP_RELAX, ng, ms)
    for l in range(ng, 1, -1):
        S.op(hip.OP_PROLONG, l - 1)
        S.op(hip.OP_RELAX, l - 1, ms if l - 1 == 1 else 2 * ms)


@pytest.mark.parametrize("ns,mname", BC_MATRIX_3D, ids=[_tag(c[0]) for c in BC_MATRIX_3D])
def test_port_to_colour_passes_residual_cycle_and_solve_3d(hip, port, ns, mname):
    mesh, u, rhs = bc_matrix_case(ns, mname)
    zero = np.zeros_like(u)
    exact = loose = 0
    for bcs in ALL_BCS_3D:
        for lap in (False, True):
            what = (bcs, "zero rhs" if lap else "rhs")
            f = zero if lap else rhs
            # the coarsest-grid solve capped at 30 sweeps, on both sides: nearly all-Neumann sets converge in thousands
            # there, an incompatible all-Neumann problem never does, and it is not this test's subject
            kw = dict(nmax_exact=30)
            S = _solver(hip, ns, mesh, bcs, None if lap else rhs, **kw)
            try:
                want, tol = {0: u}, {0: 0.0}
                for s in (1, 2, 3):
                    want[s] = port.relax3d(want[s - 1], f, mesh, bcs)
                    v = np.abs(want[s - 1]).max() + np.abs(f).max()
                    tol[s] = 2.0 * tol[s - 1] + 8.0 * (mean_sum_bound(u.size) + 2.0 ** -53) * v
                for s in (1, 3):
                    assert [q["kind"] for q in _plan(ns, s, bcs, variant=1)["passes"]] == ["color3d"] * s
                    S.upload(1, hip.BUF_U, u)
                    S.op(hip.OP_RELAX_COLOR, 1, s)
                    got = S.download(1, hip.BUF_U)
                    if _nn(bcs):
                        assert np.abs(got - want[s]).max() <= tol[s], (what, "relax", s)
                    else:
                        assert np.array_equal(got, want[s]), (what, "relax", s)
                S.upload(1, hip.BUF_U, u)
                S.op(hip.OP_RESIDUAL, 1)
                assert np.array_equal(S.download(1, hip.BUF_R), port.residual3d(u, f, mesh, bcs)), (what, "residual")
                S.upload(1, hip.BUF_U, u)
                S.vcycle(1)
                cyc = S.download(1, hip.BUF_U)
                if _nn(bcs):
                    # (module docstring) the cycle against its own single operations, the solve against cycles
                    L = hip.load_library()
                    L.ndsm_hip_debug_tail(0)
                    try:
                        S.upload(1, hip.BUF_U, u)
                        _vcycle_by_ops(hip, S, 5)
                        assert np.array_equal(S.download(1, hip.BUF_U), cyc), (what, "vcycle by operations")
                    finally:
                        L.ndsm_hip_debug_tail(1)
                    its = [u, cyc]
                    for _ in range(2):
                        S.vcycle(1)
                        its.append(S.download(1, hip.BUF_U))
                    S.upload(1, hip.BUF_U, u)
                    ie, du, nc, h = S.solve(vc_tol=1e-10, nmax=3, hist_len=8)
                    assert np.array_equal(S.download(1, hip.BUF_U), its[3]), (what, "solve")
                    assert (ie, nc) == (1, 3) and du == h[2], (what, ie, nc)
                    assert list(h) == [float(np.abs(its[k + 1] - its[k]).max()) for k in range(3)], (what, list(h))
                    loose += 1
                else:
                    assert np.array_equal(cyc, port.vcycle(u, f, mesh, bcs, **kw)), (what, "vcycle")
                    ie2, u2, du2, h2, nc2, _sw = port.solve_bvp(u.copy(), f, mesh, bcs, nmax=3, hist_len=8, **kw)
                    S.upload(1, hip.BUF_U, u)
                    ie, du, nc, h = S.solve(vc_tol=1e-10, nmax=3, hist_len=8)
                    assert (ie, nc, du) == (ie2, nc2, du2) and list(h) == list(h2[:nc2]), (what, list(h), list(h2))
                    assert np.array_equal(S.download(1, hip.BUF_U), u2), (what, "solve")
                    exact += 1
            finally:
                S.close()
    assert (exact, loose) == (2 * 63, 2 * 1)


# [70, 60]: 4200 points, the first size class above the single-workgroup one; [150, 131]: 19650 > kMed2D = 19456
SHAPES_2D = tuple((ns, m, k) for (ns, m), k in zip(BC_MATRIX_2D, ("small2d", "small2d"))) + (
    ([70, 60], "uniform", "medium2d"), ([150, 131], "uniform", "color2d"))


@pytest.mark.parametrize("ns,mname,kind", SHAPES_2D, ids=[_tag(c[0]) for c in SHAPES_2D])
def test_port_to_2d_kernels(hip, port, ns, mname, kind):
    mesh, u, rhs = bc_matrix_case(ns, mname)
    exact = loose = 0
    for bcs in ALL_BCS_2D:
        S = _solver(hip, ns, mesh, bcs, rhs)
        try:
            want = {1: port.relax_nd(u, rhs, mesh, bcs)}
            want[3] = port.relax_nd(port.relax_nd(want[1], rhs, mesh, bcs), rhs, mesh, bcs)
            for op, variant, kinds in ((hip.OP_RELAX, 0, (kind,)), (hip.OP_RELAX_COLOR, 1, ("color2d",))):
                for s in (1,) if _nn(bcs) else (1, 3):
                    # (the one-workgroup kernels take all sweeps in one launch, the colour passes one per sweep)
                    p = _plan(ns, s, bcs, variant=variant)
                    assert {q["kind"] for q in p["passes"]} == set(kinds), (bcs, op, p)
                    S.upload(1, hip.BUF_U, u)
                    S.op(op, 1, s)
                    got = S.download(1, hip.BUF_U)
                    if _nn(bcs):
                        np.testing.assert_allclose(got, want[s], rtol=0, atol=1e-14)
                    else:
                        assert np.array_equal(got, want[s]), (bcs, op, s)
            S.upload(1, hip.BUF_U, u)
            S.op(hip.OP_RESIDUAL, 1)
            assert np.array_equal(S.download(1, hip.BUF_R), port.residual_nd(u, rhs, mesh, bcs)), (bcs, "residual")
            exact += not _nn(bcs)
            loose += _nn(bcs)
        finally:
            S.close()
    assert (exact, loose) == (15, 1)


# ---------------------------------------------------------------------------------------------------------------------
# layer 3: colour passes -> the single-workgroup smoother
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,meshf", [([9, 8, 7], aniso_mesh), ([5, 5, 5], uniform_mesh), ([16, 16, 16], uniform_mesh)],
                         ids=("9x8x7", "5x5x5", "16x16x16"))
def test_single_workgroup_smoother(hip, ns, meshf):
    """rbgs3_small: <= 4096 points (16^3 is exactly that many), 1, 2 and 5 sweeps in one launch"""
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    assert np.prod(ns) <= 4096
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    ran = declined = 0
    for bcs in ALL_BCS_3D:
        for lap in (False, True):
            S = _solver(hip, ns, mesh, bcs, None if lap else rhs)
            try:
                want = _colour(hip, S, u, (1, 2, 5))
                for n in (1, 2, 5):
                    p = _plan(ns, n, bcs, rhs=not lap)
                    if _nn(bcs):        # the planner declines: colour passes + mean shift, one sweep each
                        assert [(q["kind"], q["mean_shift"]) for q in p["passes"]] == [("color3d", True)] * n
                    else:
                        assert [(q["kind"], q["sweeps"]) for q in p["passes"]] == [("small3d", n)]
                    S.upload(1, hip.BUF_U, u)
                    S.op(hip.OP_RELAX, 1, n)
                    assert np.array_equal(S.download(1, hip.BUF_U), want[n]), (bcs, lap, n)
            finally:
                S.close()
        ran += not _nn(bcs)
        declined += _nn(bcs)
    assert (ran, declined) == (63, 1)


# ---------------------------------------------------------------------------------------------------------------------
# layer 3: colour passes -> the block-resident smoother
# ---------------------------------------------------------------------------------------------------------------------
# the smallest level above the single-workgroup limit (odd nx); both faces of y, then of x, in one halo; a thin z
BLOCK_SHAPES = ([17, 16, 16], [40, 6, 20], [6, 40, 24], [34, 33, 9])


def _block_family(hip, ns, bz_knob):
    """all 64 sets on one shape; bz_knob: the block height NDSM_BLOCK_CFG of THIS process asks for (0: by level size).
    Returns the number of sets whose launches were block passes."""
    mesh = (aniso_mesh if ns[0] & 1 else uniform_mesh)(ns)
    shp = tuple(ns[::-1])
    assert np.prod(ns) > 4096
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    counts = (1, 2, 3, 5)
    ran = 0
    for bcs in ALL_BCS_3D:
        for lap in (False, True):
            S = _solver(hip, ns, mesh, bcs, None if lap else rhs)
            try:
                want = _colour(hip, S, u, counts)
                for n in counts:
                    p = _plan(ns, n, bcs, rhs=not lap, block_cfg=(bz_knob, 0))
                    if _nn(bcs):        # the fallback: the colour passes themselves, so equality is exact there too
                        assert [(q["kind"], q["mean_shift"]) for q in p["passes"]] == [("color3d", True)] * n
                    else:
                        assert {(q["kind"], q["bz"]) for q in p["passes"]} == {("block", bz_knob or 4)}, (ns, bcs, p)
                        assert [q["sweeps"] for q in p["passes"]] == [2] * (n // 2) + [1] * (n & 1)
                    S.upload(1, hip.BUF_U, u)
                    S.op(hip.OP_RELAX, 1, n)
                    assert np.array_equal(S.download(1, hip.BUF_U), want[n]), (ns, bcs, lap, n)
            finally:
                S.close()
        ran += not _nn(bcs)
    return ran


@pytest.mark.parametrize("ns", BLOCK_SHAPES, ids=_tag)
def test_block_smoother(hip, ns):
    """blocks of height 4, the planner's own choice on levels of fewer than 64 blocks of 16 x 8 x 8"""
    assert "NDSM_BLOCK_CFG" not in os.environ and "NDSM_HIP_NO_BLOCK" not in os.environ
    assert _block_family(hip, ns, 0) == 63


def _block_child():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    print("block8 sets", [_block_family(_lib, ns, 8) for ns in BLOCK_SHAPES])


def test_block_smoother_height_8():
    """the same with blocks of height 8 - the knob is read from the environment once per process, hence a fresh one"""
    env = dict(os.environ, NDSM_BLOCK_CFG="8,0")
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_bc_matrix as t; t._block_child()"
            % (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "block8 sets %s" % ([63] * len(BLOCK_SHAPES)) in out.stdout, out.stdout[-500:]


# ---------------------------------------------------------------------------------------------------------------------
# layer 3: colour passes -> the fused smoother, forced onto small shapes
# ---------------------------------------------------------------------------------------------------------------------
# instantiation -> (TXH, TYH, sweeps, residual stage) of launch_fused_t (csrc/smooth_fused.hip)
FUSED_TILES = {"F2 136x30/1024": (136, 30, 2, 0), "F2 136x30/1024 L1": (136, 30, 2, 0), "F2 136x22/768": (136, 22, 2, 0),
               "F2 72x28/512": (72, 28, 2, 0), "F1 132x23/768": (132, 23, 1, 0), "F1 132x31/1024": (132, 31, 1, 0),
               "F1R 136x22/768": (136, 22, 1, 1)}


def fused_tile_counts(inst, ns):
    """(tiles in x, tiles in y) as launch_cfg derives them: a tile of TXH x TYH points owns the inner
    TXH - 2 HX by TYH - 2 NST (HX = NST rounded up to even, NST = 2 sweeps (+ 1 for the residual stage)), and the
    last tile of a row or column also owns its halo inside the domain"""
    txh, tyh, s, res = FUSED_TILES[inst]
    nst = 2 * s + res
    hx = (nst + 1) & ~1
    txi, tyi = txh - 2 * hx, tyh - 2 * nst
    ntx = (ns[0] - hx + txi - 1) // txi if ns[0] > hx else 1
    nty = (ns[1] - nst + tyi - 1) // tyi if ns[1] > nst else 1
    return ntx, nty


# (two, one, res, big) of ndsm_hip_debug_fused_cfg: between them every instantiation fused_pass can select for a plain
# or a sweep + residual request.  Odd nx has one two-sweep and one sweep + residual instantiation and both one-sweep
# tiles, so the first two rows cover it.
FUSED_CFGS = ((0, 0, 0, -1),     # small levels: F2 72x28, F1 132x23, F1R
              (3, 7, 0, -1),     # F2 136x22, F1 132x31
              (1, 8, 0, 0),      # F2 136x30, F1 132x23
              (1, 0, 0, 1))      # the level-1 symbol of F2 136x30, F1 132x31 (the tiles of >= 64 M-point levels)
# [70, 30, 10] / [71, 30, 10]: two tiles in x AND y for the narrow tile, two in y for every wide one, and so few planes
# that the first and the last z chunk both touch a face; [32, 32, 42] / [33, 32, 42]: two in y, several chunks.
# ([70, 24, 10] gives the narrow tile (24 - 4) / 20 = 1 tile in y and the wide ones 1 as well: ny = 30 is the first
# that gives every instantiation two.)
FUSED_SHAPES = ([70, 30, 10], [71, 30, 10], [32, 32, 42], [33, 32, 42])


def test_fused_shapes_have_the_tiles_they_are_meant_to():
    for ns in FUSED_SHAPES:
        for inst in FUSED_TILES:
            assert fused_tile_counts(inst, ns)[1] >= 2, (ns, inst)
    assert fused_tile_counts("F2 72x28/512", [70, 30, 10]) == (2, 2)
    assert fused_tile_counts("F2 72x28/512", [70, 24, 10]) == (2, 1)      # (why ny is not 24)


@pytest.mark.parametrize("ns", FUSED_SHAPES, ids=_tag)
def test_forced_fused_smoother(hip, ns):
    """OP_RELAX_FUSED at 1, 2 and 5 (2 + 2 + 1) sweeps and OP_RELAX_RES_FUSED at 1 and 3, every tile configuration, the
    planner's z chunking and two work items per tile, general and declared-zero rhs.  All-Neumann: one sweep per
    pass, the mean shift of the colour path after each; the sweep + residual launch is not offered there."""
    L = hip.load_library()
    odd = bool(ns[0] & 1)
    mesh = (aniso_mesh if odd else uniform_mesh)(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    nan = np.full(shp, np.nan)
    seen, ran, no_res = set(), 0, []
    try:
        for bcs in ALL_BCS_3D:
            for lap in (False, True):
                S = _solver(hip, ns, mesh, bcs, None if lap else rhs)
                try:
                    want = _colour(hip, S, u, (1, 2, 3, 5), residual=True)
                    for two, one, res, big in FUSED_CFGS[:2] if odd else FUSED_CFGS:
                        first = _plan(ns, 2, bcs, variant=2, fused_cfg=(two, one, res, 0, big))["passes"][0]["inst"]
                        ntx, nty = fused_tile_counts(first, ns)
                        for w in (0, 2 * ntx * nty):
                            cfg = (two, one, res, w, big)
                            L.ndsm_hip_debug_fused_cfg(*cfg)
                            for n in (1, 2, 5):
                                p = _plan(ns, n, bcs, variant=2, rhs=not lap, fused_cfg=cfg)
                                assert all(q["kind"] == "fused" and q["odd_nx"] == odd and q["src"] != q["dst"]
                                           for q in p["passes"]), (bcs, cfg, p)
                                assert all(q["mean_shift"] == _nn(bcs) for q in p["passes"])
                                seen |= {q["inst"] for q in p["passes"]}
                                S.upload(1, hip.BUF_U, u)
                                S.op(hip.OP_RELAX_FUSED, 1, n)
                                assert np.array_equal(S.download(1, hip.BUF_U), want[n][0]), (bcs, lap, cfg, n)
                            for n in (1, 3):
                                p = _plan(ns, n, bcs, variant=2, rhs=not lap, want_res=True, fused_cfg=cfg)
                                if not p["res_done"]:
                                    no_res.append(bcs)
                                    continue
                                assert all(q["kind"] == "fused" for q in p["passes"]) and p["passes"][-1]["mode"] == "R"
                                seen |= {q["inst"] for q in p["passes"]}
                                S.upload(1, hip.BUF_U, u)
                                S.upload(1, hip.BUF_R, nan)
                                S.op(hip.OP_RELAX_RES_FUSED, 1, n)
                                assert np.array_equal(S.download(1, hip.BUF_U), want[n][0]), (bcs, lap, cfg, n, "u")
                                assert np.array_equal(S.download(1, hip.BUF_R), want[n][1]), (bcs, lap, cfg, n, "r")
                finally:
                    S.close()
            ran += 1
    finally:
        L.ndsm_hip_debug_fused_cfg(0, 0, 0, 0, -1)
    assert ran == 64 and set(no_res) == {"NNNNNN"}
    if odd:
        assert seen == {"F2 136x30/1024", "F1 132x23/768", "F1 132x31/1024", "F1R 136x22/768"}
    else:
        assert seen == set(FUSED_TILES)


# ---------------------------------------------------------------------------------------------------------------------
# layer 3: colour passes -> the fused smoother at its own size
# ---------------------------------------------------------------------------------------------------------------------
OWN_SIZE = [161, 120, 115]          # just above 2 Mi points: the smallest level the planner sends there by itself
_own_fields = {}


@pytest.mark.parametrize("bcs", ARRAY16)
def test_fused_smoother_at_its_own_size(hip, bcs):
    ns = OWN_SIZE
    shp = tuple(ns[::-1])
    if not _own_fields:
        _own_fields["u"], _own_fields["rhs"] = rand_field(shp, 2112), rand_field(shp, 2113)
    u, rhs = _own_fields["u"], _own_fields["rhs"]
    p = _plan(ns, 5, bcs)
    assert [(q["kind"], q["inst"], q["odd_nx"], q["sweeps"]) for q in p["passes"]] == [
        ("fused", "F2 136x30/1024", True, 2), ("fused", "F2 136x30/1024", True, 2), ("fused", "F1 132x23/768", True, 1)]
    p = _plan(ns, 5, bcs, variant=2, want_res=True)
    assert p["res_done"] and [(q["kind"], q["inst"], q["mode"]) for q in p["passes"]] == [
        ("fused", "F2 136x30/1024", ""), ("fused", "F2 136x30/1024", ""), ("fused", "F1R 136x22/768", "R")]
    S = _solver(hip, ns, uniform_mesh(ns), bcs, rhs)
    try:
        uw, rw = _colour(hip, S, u, (5,), residual=True)[5]
        S.upload(1, hip.BUF_U, u)
        S.op(hip.OP_RELAX, 1, 5)
        assert np.array_equal(S.download(1, hip.BUF_U), uw), (bcs, "relax")
        S.upload(1, hip.BUF_U, u)
        S.upload(1, hip.BUF_R, np.full(shp, np.nan))
        S.op(hip.OP_RELAX_RES_FUSED, 1, 5)
        assert np.array_equal(S.download(1, hip.BUF_U), uw), (bcs, "sweep + residual: u")
        assert np.array_equal(S.download(1, hip.BUF_R), rw), (bcs, "sweep + residual: r")
    finally:
        S.close()


# ---------------------------------------------------------------------------------------------------------------------
# layer 3: level by level -> the tail cycle
# ---------------------------------------------------------------------------------------------------------------------
def _tail_run(hip, ns, mesh, bcs, u, rhs, ms, du_max):
    S = hip.MGSolver(ns, mesh, bcs, ms=ms, du_max=du_max)
    try:
        S.upload(1, hip.BUF_U, u)
        S.upload(1, hip.BUF_RHS, rhs)
        S.vcycle(2)
        lev = [(S.download(l, hip.BUF_U), S.download(l, hip.BUF_RHS)) for l in range(1, S.ngrids + 1)]
        info = S.info()
        ie, du, nc, h = S.solve(vc_tol=1e-9, nmax=6, hist_len=8)
        return lev, info, (ie, du, nc, list(h)), S.download(1, hip.BUF_U), [int(np.prod(sh)) for sh in S.shapes]
    finally:
        S.close()


@pytest.mark.parametrize("ns,meshf", [([22, 22, 22], uniform_mesh), ([33, 22, 27], aniso_mesh)], ids=("22x22x22", "33x22x27"))
def test_tail_cycle(hip, ns, meshf):
    """test_tail_cycle_bitwise's procedure: the tail launch switched off against on - two V-cycles, every level's u and
    rhs, the coarsest-grid counters, a six-cycle solve history.  All 64 sets at ms = 5 with the max metric; ms = 1 and
    the mean metric on the 16 sets of the array.  The coarsest levels here (5 x 5 x 5 and 8 x 5 x 6 points) have 27 and
    72 updated points under DDDDDD and 100 and 200 under NNNNND: either side of the 64 updated points below which
    tail.hip takes its single-wave paths.  (3-D all-Neumann hierarchies are not offered to the tail launch; NNNNNN
    runs level by level both times.)"""
    L = hip.load_library()
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 7), rand_field(shp, 8)
    cases = [(b, 5, True) for b in ALL_BCS_3D] + [(b, ms, dm) for b in ARRAY16 for ms, dm in ((1, True), (5, False), (1, False))]
    ran = 0
    try:
        for bcs, ms, du_max in cases:
            L.ndsm_hip_debug_tail(0)
            want = _tail_run(hip, ns, mesh, bcs, u, rhs, ms, du_max)
            L.ndsm_hip_debug_tail(1)
            got = _tail_run(hip, ns, mesh, bcs, u, rhs, ms, du_max)
            sizes = want[4]
            assert len(sizes) >= 3 and sizes[-2] <= 6144        # the two coarsest levels qualify
            ran += 1
            for l, (a, b) in enumerate(zip(want[0], got[0]), start=1):
                assert np.array_equal(a[0], b[0]), (bcs, ms, du_max, "u", l)
                assert np.array_equal(a[1], b[1]), (bcs, ms, du_max, "rhs", l)
            assert want[1] == got[1], (bcs, ms, du_max, want[1], got[1])
            assert want[2] == got[2], (bcs, ms, du_max, want[2], got[2])
            assert np.array_equal(want[3], got[3]), (bcs, ms, du_max)
    finally:
        L.ndsm_hip_debug_tail(1)
    assert ran == 64 + 3 * 16


# ---------------------------------------------------------------------------------------------------------------------
# layer 3 (against the port: there is no second device path): the coarsest-grid solve
# ---------------------------------------------------------------------------------------------------------------------
# a one-level hierarchy, so that OP_EXACT solves level 1: the smallest grid a solver takes (4 points per axis: eight
# updated points under DDDDDD), 1716 points (solve_exact_k, <= 2048), 6120 points (the host loop over the colour passes)
EXACT_SHAPES = ([4, 4, 4], [12, 11, 13], [20, 18, 17])
# (ex_tol, max metric, nmax_exact): the stop test decides (du is a max: no sum enters, so the port's decisions are the
# device's); five sweeps that never stop early, with the mean metric
EXACT_OPTIONS = ((1e-2, True, 40), (0.0, False, 5))


@pytest.mark.parametrize("ns", EXACT_SHAPES, ids=_tag)
def test_coarsest_grid_solve(hip, port, ns):
    mesh = aniso_mesh(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    exact = loose = 0
    for bcs in ALL_BCS_3D:
        for ex_tol, du_max, nmax in EXACT_OPTIONS[1:] if _nn(bcs) else EXACT_OPTIONS:
            what = (bcs, ex_tol, du_max, nmax)
            kw = dict(ex_tol=ex_tol, du_max=du_max, nmax_exact=nmax)
            _ie, want, _du, _h, _nc, sweeps = port.solve_bvp(u, rhs, mesh, bcs, ngrids=1, nmax=1, hist_len=1, **kw)
            S = hip.MGSolver(ns, mesh, bcs, ngrids=1, **kw)
            try:
                assert S.ngrids == 1
                S.upload(1, hip.BUF_U, u)
                S.upload(1, hip.BUF_RHS, rhs)
                S.op(hip.OP_EXACT, 1)
                got = S.download(1, hip.BUF_U)
                done, unconverged = S.info()
            finally:
                S.close()
            # (the stop test comes BEFORE each sweep: a solve that used all its sweeps did not converge)
            assert (done, unconverged) == (sweeps, int(sweeps == nmax)), (what, done, unconverged, sweeps)
            if _nn(bcs):
                tol, it = 0.0, u
                for _ in range(nmax):       # the bound of test_gpu_block_smoother.py along the port's own sweeps
                    v = np.abs(it).max() + np.abs(rhs).max()
                    tol = 2.0 * tol + 8.0 * (mean_sum_bound(u.size) + 2.0 ** -53) * v
                    it = port.relax3d(it, rhs, mesh, bcs)
                assert sweeps == nmax and np.array_equal(it, want), what
                assert np.abs(got - want).max() <= tol, what
                loose += 1
            else:
                assert np.array_equal(got, want), what
                exact += 1
    assert (exact, loose) == (63 * len(EXACT_OPTIONS), 1)


# ---------------------------------------------------------------------------------------------------------------------
# layer 3: zeros in memory -> the zero first guess by declaration
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", ([16, 16, 8], [17, 16, 9], [40, 33, 12]), ids=_tag)
def test_zero_first_guess_forced_pass(hip, ns):
    """test_gpu_zero_guess.py's forced passes on its shapes: the source array NaN and declared zero (OP_ZERO_U) against
    zeros in memory, and both against the colour passes from zeros"""
    L = hip.load_library()
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    rhs = rand_field(shp, 2113)
    zero, nan = np.zeros(shp), np.full(shp, np.nan)
    runs = [(hip.OP_RELAX_FUSED, 1), (hip.OP_RELAX_FUSED, 2), (hip.OP_RELAX_RES_FUSED, 1), (hip.OP_RELAX_RES_FUSED, 2),
            (hip.OP_RELAX_RES_FUSED, 3)]
    ran = 0
    try:
        for bcs in ARRAY16:
            S = _solver(hip, ns, mesh, bcs, rhs)
            try:
                for lap in (False, True):
                    if lap:
                        S.zero_rhs()
                    want = _colour(hip, S, zero, (1, 2, 3), residual=True)
                    for op, nsw in runs:
                        what = (bcs, lap, op, nsw)
                        with_res = op == hip.OP_RELAX_RES_FUSED
                        mat, sched, _head = zplan(ns, nsw, variant=2, rhs=not lap, want_res=with_res)
                        assert not mat and sched[0].endswith(" Z"), (what, sched)   # the first pass takes the descriptor
                        out = []
                        for on in (0, 1):
                            L.ndsm_hip_debug_zero_guess(on)
                            S.upload(1, hip.BUF_U, nan if on else zero)
                            S.upload(1, hip.BUF_UALT, nan)
                            S.upload(1, hip.BUF_R, nan)
                            if on:
                                S.op(hip.OP_ZERO_U, 1)
                                assert L.ndsm_hip_debug_u_declared_zero(S.h, 1) == 1, what
                            S.op(op, 1, nsw)
                            assert L.ndsm_hip_debug_u_declared_zero(S.h, 1) == 0, what
                            out.append((S.download(1, hip.BUF_U), S.download(1, hip.BUF_R)))
                        assert np.array_equal(out[0][0], want[nsw][0]), what
                        assert np.array_equal(out[1][0], out[0][0]), what
                        if with_res:
                            assert np.array_equal(out[0][1], want[nsw][1]), what
                            assert np.array_equal(out[1][1], out[0][1]), what
            finally:
                S.close()
            ran += 1
    finally:
        L.ndsm_hip_debug_zero_guess(1)
    assert ran == 16


def test_zero_first_guess_in_the_cycle(hip):
    """64^3, the smallest hierarchy of test_gpu_zero_guess.py (level 2: the block-resident launch, level 3: the tail):
    OP_DESCEND, then a V-cycle and a short solve with every coarse array NaN first, the feature off against on"""
    L = hip.load_library()
    ns = [64, 64, 64]
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    ran = 0

    def run(bcs, on):
        L.ndsm_hip_debug_zero_guess(on)
        S = _solver(hip, ns, mesh, bcs, rhs)
        try:
            S.upload(1, hip.BUF_U, u)
            for l in range(2, S.ngrids + 1):
                nan = np.full(S._npshape(l), np.nan)
                S.upload(l, hip.BUF_U, nan)
                S.upload(l, hip.BUF_UALT, nan)
            S.op(hip.OP_RELAX_RES, 1, 2)
            S.op(hip.OP_DESCEND, 1)
            out = [S.download(2, hip.BUF_RHS), S.download(2, hip.BUF_U)]
            assert not out[1].any()
            S.upload(1, hip.BUF_U, u)
            S.vcycle(1)
            out += [S.download(l, hip.BUF_U) for l in range(1, S.ngrids + 1)]
            assert all(L.ndsm_hip_debug_u_declared_zero(S.h, l) == 0 for l in range(1, S.ngrids + 1))
            ie, du, nc, h = S.solve(vc_tol=1e-6, nmax=4, hist_len=8)
            out += [S.download(l, hip.BUF_U) for l in range(1, S.ngrids + 1)]
            return out, (ie, du, nc, list(h)), S.info()
        finally:
            S.close()

    try:
        for bcs in ARRAY16:
            off, on = run(bcs, 0), run(bcs, 1)
            assert off[1:] == on[1:] and off[1][2] >= 2, (bcs, off[1:], on[1:])
            assert len(off[0]) == len(on[0]) and all(np.array_equal(a, b) for a, b in zip(off[0], on[0])), bcs
            ran += 1
    finally:
        L.ndsm_hip_debug_zero_guess(1)
    assert ran == 16


# ---------------------------------------------------------------------------------------------------------------------
# layer 3: the single domain -> z-slab worlds (loop-back)
# ---------------------------------------------------------------------------------------------------------------------
SLAB_SHAPES = ([32, 24, 32], [17, 16, 26])      # three slabs of 10, 11, 11 and 8, 9, 9 owned planes


@pytest.mark.parametrize("ns", SLAB_SHAPES, ids=_tag)
def test_slab_worlds(hip, ns):
    """World.relax(3) and vcycle(2) with 2 and 3 slabs against MGSolver on the whole domain.  A slab has no launch
    but the fused one (the planner answers a slab level without it with an error), so a world that runs has run it;
    the z letters decide what the bottom and the top slab do at their outer faces, the middle slab has none."""
    mesh = (aniso_mesh if ns[0] & 1 else uniform_mesh)(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    for nr in (2, 3):
        plan = hip.slab_plan(ns, mesh, nr)
        assert len(plan) == nr and all(s["z1"] - s["z0"] >= 8 for s in plan) and ns[0] >= 16 and ns[1] >= 16
    ran, zpairs = 0, set()
    for bcs in ARRAY16:
        S = _solver(hip, ns, mesh, bcs, rhs)
        try:
            S.upload(1, hip.BUF_U, u)
            S.op(hip.OP_RELAX_COLOR, 1, 3)
            swept = S.download(1, hip.BUF_U)
            S.upload(1, hip.BUF_U, u)
            S.vcycle(2)
            cycled = S.download(1, hip.BUF_U)
        finally:
            S.close()
        for nr in (2, 3):
            W = hip.World(ns, mesh, bcs, nr)
            try:
                assert W.nlocal == nr and W.slabs[0]["z0"] == 0 and W.slabs[-1]["z1"] == ns[2]
                W.upload(hip.BUF_RHS, rhs)
                W.upload(hip.BUF_U, u)
                W.relax(3)
                assert np.array_equal(W.download(hip.BUF_U), swept), (bcs, nr, "sweeps")
                W.upload(hip.BUF_U, u)
                W.vcycle(2)
                assert np.array_equal(W.download(hip.BUF_U), cycled), (bcs, nr, "vcycle")
            finally:
                W.close()
        zpairs.add(bcs[2] + bcs[5])
        ran += 1
    assert ran == 16 and zpairs == set(_PAIRS)


# ---------------------------------------------------------------------------------------------------------------------
# the mixed-precision cycle against tests/mixed_model.py
# ---------------------------------------------------------------------------------------------------------------------
MIXED_NS = mm.MIXED_SHAPES[0][0]        # [64, 32, 32]: the smallest level the gate admits


@pytest.mark.parametrize("bcs", ARRAY16)
def test_mixed_precision_cycle(hip, port, bcs):
    """test_gpu_mixed.py's comparison A (and the metric that follows from it): u after 1, 2 and 3 cycles is the float32
    model's, bit for bit, and the history is the model's max|e|.  The model takes any letters: its fp64 sweep and
    residual are the port's under all 63 sets (asserted here for this set).  None of the array's sets is all-Neumann."""
    ns = MIXED_NS
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    u0, rhs = rand_field(shp, 2112), rand_field(shp, 2113) * 10.0
    assert np.array_equal(mm.sweep(u0, rhs, mesh, bcs), port.relax3d(u0, rhs, mesh, bcs))
    assert np.array_equal(mm.residual(u0, rhs, mesh, bcs), port.residual3d(u0, rhs, mesh, bcs))
    um, dum = mm.mixed_cycles(port, u0, rhs, mesh, bcs, 5, 3, False, np.float32)
    ref = port.vcycle(u0, rhs, mesh, bcs)
    assert 0.0 < np.abs(um[0] - ref).max() < 1e-4 * np.abs(ref - u0).max()     # (fp32 against fp64: close, not equal)
    S = _solver(hip, ns, mesh, bcs, rhs)
    try:
        assert S.set_precision(2) is True, bcs
        for k in (1, 2, 3):
            S.upload(1, hip.BUF_U, u0)
            ie, du, nc, h = S.solve(vc_tol=0.0, nmax=k, hist_len=8)
            assert (ie, nc) == (1, k) and list(h) == dum[:k] and du == dum[k - 1], (bcs, k, list(h), dum)
            assert np.array_equal(S.download(1, hip.BUF_U), um[k - 1]), (bcs, k)
    finally:
        S.close()


def test_mixed_precision_gate_refuses_all_neumann(hip):
    ns = MIXED_NS
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    u0, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    rhs = rhs - rhs.mean()
    out = []
    for precision in (None, 2):
        S = _solver(hip, ns, mesh, "NNNNNN", rhs)
        try:
            if precision is not None:
                assert S.set_precision(precision) is False
            S.upload(1, hip.BUF_U, u0)
            res = S.solve(vc_tol=1e-10, nmax=2, hist_len=8)
            out.append((res[0], res[1], res[2], list(res[3]), S.download(1, hip.BUF_U)))
        finally:
            S.close()
    assert out[0][:4] == out[1][:4] and out[0][2] == 2
    assert np.array_equal(out[0][4], out[1][4])
