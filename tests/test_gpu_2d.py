"""The 2-D solver's kernels against the oracle in every size class (run with -m gpu on an MI355X).

relax_impl sends a 2-D level to rbgs2_small (n <= 4096), rbgs2_medium (n <= 19456) or rbgs2_color +
launch_mean_shift by its point count; the shapes of model2d.SHAPES_2D sit on both sides of every threshold, with odd,
thin and trailing-loop sizes in between.  Everything goes through MGSolver / ndsm_hip_mg_op.

Every assertion is bit for bit:
  * boundary sets with a Dirichlet face, max metric: against the oracle (port.relax_nd, residual_nd, restrict,
    interp, vcycle, solve_bvp);
  * the all-Neumann set and the mean metric, where the order of a sum enters the result: against tests/model2d.py,
    which restates the device's summation orders and which test_model2d.py ties to the oracle (it IS the oracle when
    it sums in index order).  An all-Neumann sweep is ALSO held to the rounding bound of that sum against the
    oracle itself (model2d.neumann_bound), so that a wrong model cannot hide a wrong kernel.
"""
import numpy as np
import pytest

import model2d as m2
from golden_inputs import aniso_mesh, rand_field, uniform_mesh

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


def _cases(shapes=m2.SHAPES_2D):
    return ([pytest.param(ns, uniform_mesh, id=_tag(ns)) for ns in shapes] +
            [pytest.param(ns, aniso_mesh, id="aniso-" + _tag(ns)) for ns in shapes if ns in list(m2.ANISO_2D)])


def _fields(ns):
    shp = tuple(int(n) for n in ns[::-1])
    return rand_field(shp, 2112), rand_field(shp, 2113)


def _rhs_for(bcs, rhs):
    return rhs - rhs.mean() if m2.all_neumann(bcs) else rhs


def _pad_r(solver, arr, fill=0.0):
    """a level-l array at the start of the level-1 sized residual scratch"""
    full = np.full(solver._npshape(1), fill)
    full.ravel()[:arr.size] = arr.ravel()
    return full


def _iterate(step, u, n):
    out = [u]
    for _ in range(n):
        out.append(step(out[-1]))
    return out


def _check_sweeps(hip, port, S, level, mesh, bcs, u, rhs, tag):
    """OP_RELAX x 1, 2, 5 and OP_RELAX_COLOR x 1, 3 on one level: the oracle's bits; on the all-Neumann set the model's
    bits in the order of the level's size class (variant 0) or of the two-stage kernels (variant 1), and after one
    sweep within the summation bound of the oracle"""
    alln = m2.all_neumann(bcs)
    oracle = _iterate(lambda v: port.relax_nd(v, rhs, mesh, bcs), u, 5)
    for op, variant, counts in ((hip.OP_RELAX, 0, (1, 2, 5)), (hip.OP_RELAX_COLOR, 1, (1, 3))):
        want = _iterate(lambda v: m2.relax2d(v, rhs, mesh, bcs, 1, variant), u, max(counts)) if alln else oracle
        for count in counts:
            S.upload(level, hip.BUF_U, u)
            S.op(op, level, count)
            got = S.download(level, hip.BUF_U)
            assert np.array_equal(got, want[count]), (tag, bcs, "op", op, "sweeps", count)
            if alln and count == 1:
                assert np.abs(got - oracle[1]).max() <= m2.neumann_bound(oracle[1], got.size), (tag, op)


@pytest.mark.parametrize("ns,meshf", _cases())
def test_sweeps_and_residual_bitwise(hip, port, ns, meshf):
    mesh = meshf(ns)
    u, rhs = _fields(ns)
    shapes, meshes = port.hierarchy(ns, mesh)
    for bcs in m2.BCS_2D:
        r = _rhs_for(bcs, rhs)
        S = hip.MGSolver(ns, mesh, bcs)
        assert [tuple(int(v) for v in s) for s in shapes] == S.shapes
        S.upload(1, hip.BUF_RHS, r)
        _check_sweeps(hip, port, S, 1, mesh, bcs, u, r, _tag(ns))
        # residual2, into a scratch full of NaN
        S.upload(1, hip.BUF_U, u)
        S.upload(1, hip.BUF_R, np.full(u.shape, np.nan))
        S.op(hip.OP_RESIDUAL, 1)
        assert np.array_equal(S.download(1, hip.BUF_R), port.residual_nd(u, r, mesh, bcs)), (bcs, "residual")
        if ns == [300, 260]:     # levels 2 (19500 points) and 3 (4875): the other two size classes, odd coarse shapes
            for lvl in (2, 3):
                ul, rl = _fields(shapes[lvl - 1])
                rl = _rhs_for(bcs, rl)
                S.upload(lvl, hip.BUF_RHS, rl)
                _check_sweeps(hip, port, S, lvl, meshes[lvl - 1], bcs, ul, rl, "level %d" % lvl)
                S.upload(lvl, hip.BUF_U, ul)
                S.upload(1, hip.BUF_R, np.full(u.shape, np.nan))
                S.op(hip.OP_RESIDUAL, lvl)
                assert np.array_equal(S.download(lvl, hip.BUF_R, shape_level=lvl),
                                      port.residual_nd(ul, rl, meshes[lvl - 1], bcs)), (bcs, "residual", lvl)
        # a declared-zero right-hand side: the kernels skip the read
        S.zero_rhs()
        zero = np.zeros_like(u)
        for op, variant, count in ((hip.OP_RELAX, 0, 2), (hip.OP_RELAX_COLOR, 1, 2)):
            S.upload(1, hip.BUF_U, u)
            S.op(op, 1, count)
            if m2.all_neumann(bcs):
                want = m2.relax2d(u, None, mesh, bcs, count, variant)
            else:
                want = _iterate(lambda v: port.relax_nd(v, zero, mesh, bcs), u, count)[count]
            assert np.array_equal(S.download(1, hip.BUF_U), want), (bcs, "zero rhs", op)
        S.upload(1, hip.BUF_U, u)
        S.upload(1, hip.BUF_R, np.full(u.shape, np.nan))
        S.op(hip.OP_RESIDUAL, 1)
        assert np.array_equal(S.download(1, hip.BUF_R), port.residual_nd(u, zero, mesh, bcs)), (bcs, "residual, zero rhs")
        S.close()


@pytest.mark.parametrize("ns,meshf", _cases())
def test_transfers_bitwise(hip, port, ns, meshf):
    """restrict_k<2> / prolong_add_k<2> on every level pair: the restriction writes rhs(l + 1) and zeroes u(l + 1), the
    prolongation adds onto a zero and onto a non-zero u(l)"""
    mesh = meshf(ns)
    S = hip.MGSolver(ns, mesh, "NDDN")
    shapes, _ = port.hierarchy(ns, mesh)
    for lvl in range(1, len(shapes)):
        f = rand_field(tuple(int(v) for v in shapes[lvl - 1][::-1]), 3000 + lvl)
        c = rand_field(tuple(int(v) for v in shapes[lvl][::-1]), 4000 + lvl)
        S.upload(1, hip.BUF_R, _pad_r(S, f, np.nan))
        S.upload(lvl + 1, hip.BUF_U, c)
        S.upload(lvl + 1, hip.BUF_RHS, np.full(c.shape, np.nan))
        S.op(hip.OP_RESTRICT, lvl)
        assert np.array_equal(S.download(lvl + 1, hip.BUF_RHS), port.restrict(f, ns, mesh, lvl)), f"restrict {lvl}"
        assert not S.download(lvl + 1, hip.BUF_U).any(), f"u({lvl + 1}) not zeroed"
        S.upload(lvl + 1, hip.BUF_U, c)
        S.upload(lvl, hip.BUF_U, np.zeros_like(f))
        S.op(hip.OP_PROLONG, lvl)
        assert np.array_equal(S.download(lvl, hip.BUF_U), port.interp(c, ns, mesh, lvl)), f"interp {lvl}"
        S.upload(lvl, hip.BUF_U, f)
        S.op(hip.OP_PROLONG, lvl)
        assert np.array_equal(S.download(lvl, hip.BUF_U), f + port.interp(c, ns, mesh, lvl)), f"interp onto u {lvl}"
    S.close()


@pytest.mark.parametrize("root,ngrids,level", m2.EXACT_ROOTS, ids=lambda v: _tag(v) if isinstance(v, list) else str(v))
@pytest.mark.parametrize("meshf", (uniform_mesh, aniso_mesh), ids=("uniform", "aniso"))
def test_coarsest_grid_solve_bitwise(hip, port, root, ngrids, level, meshf):
    """OP_EXACT: solve_exact_k (2-D and 3-D branch, up to its 2048-point limit) and the host-driven loop above it - u,
    the sweep count and the unconverged count against the model's loop, whose stop decisions test_model2d.py shows to
    be the oracle's and clear of ex_tol; a second call continues from the result and accumulates both counters"""
    mesh = meshf(root)
    shapes, meshes = port.hierarchy(root, mesh, ngrids)
    ns = [int(v) for v in shapes[level - 1]]
    u, rhs = _fields(ns)
    exact = m2.exact2d if len(ns) == 2 else m2.exact3d
    for bcs in m2.EXACT_BCS[len(ns)]:
        r = _rhs_for(bcs, rhs)
        for ex_tol, use_max, nmax in m2.EXACT_OPTIONS:
            tag = (bcs, ex_tol, use_max, nmax)
            S = hip.MGSolver(root, mesh, bcs, ngrids=ngrids, ex_tol=ex_tol, du_max=use_max, nmax_exact=nmax)
            assert S.shapes[level - 1] == tuple(ns)
            S.upload(level, hip.BUF_U, u)
            S.upload(level, hip.BUF_RHS, r)
            S.op(hip.OP_EXACT, level)
            want, sweeps, conv, _dus = exact(u, r, meshes[level - 1], bcs, ex_tol, use_max, nmax)
            got = S.download(level, hip.BUF_U)
            assert S.info() == (sweeps, 0 if conv else 1), tag
            assert np.array_equal(got, want), tag
            S.op(hip.OP_EXACT, level)
            want2, sweeps2, conv2, _dus = exact(want, r, meshes[level - 1], bcs, ex_tol, use_max, nmax)
            assert S.info() == (sweeps + sweeps2, (0 if conv else 1) + (0 if conv2 else 1)), tag
            assert np.array_equal(S.download(level, hip.BUF_U), want2), tag
            S.close()


_BCS_IDS = [pytest.param(b, id=b) for b in m2.BCS_2D]


@pytest.mark.parametrize("bcs", _BCS_IDS)
@pytest.mark.parametrize("ns,meshf", _cases(m2.VCYCLE_SHAPES))
def test_vcycle_and_solve_bitwise(hip, port, ns, meshf, bcs):
    """two V-cycles, then a solve that continues from them, level by level and with the tail launch off and on: every
    level's u and rhs, the coarsest-grid counters, the solve's history, cycle count and result"""
    L = hip.load_library()
    mesh = meshf(ns)
    u, rhs = _fields(ns)
    rhs = _rhs_for(bcs, rhs)
    try:
        for ms in (1, 5):
            for du_max in (True, False):
                tag = (bcs, ms, du_max)
                kw = dict(ms=ms, du_max=du_max, **m2.VCYCLE_KW)
                lev, sw1, un1 = m2.vcycle2d(port, u, rhs, mesh, bcs, **kw)
                lev, sw2, un2 = m2.vcycle2d(port, lev[0][0], rhs, mesh, bcs, **kw)
                ierr, out, du, hist, nc, sw3, un3 = m2.solve2d(port, lev[0][0], rhs, mesh, bcs, vc_tol=1e-9, nmax=6, **kw)
                if du_max and not m2.all_neumann(bcs):      # no sum enters: the model must be the oracle here
                    two = port.vcycle(port.vcycle(u, rhs, mesh, bcs, **kw), rhs, mesh, bcs, **kw)
                    assert np.array_equal(lev[0][0], two), tag
                    o = port.solve_bvp(two, rhs, mesh, bcs, vc_tol=1e-9, nmax=6, hist_len=8, **kw)
                    assert (ierr, du, nc, hist) == (o[0], o[2], o[4], list(o[3])) and np.array_equal(out, o[1]), tag
                for tail in (0, 1):
                    L.ndsm_hip_debug_tail(tail)
                    S = hip.MGSolver(ns, mesh, bcs, **kw)
                    S.upload(1, hip.BUF_U, u)
                    S.upload(1, hip.BUF_RHS, rhs)
                    S.vcycle(2)
                    for l in range(1, S.ngrids + 1):
                        assert np.array_equal(S.download(l, hip.BUF_U), lev[l - 1][0]), (tag, tail, "u", l)
                        assert np.array_equal(S.download(l, hip.BUF_RHS), lev[l - 1][1]), (tag, tail, "rhs", l)
                    assert S.info() == (sw1 + sw2, un1 + un2), (tag, tail)
                    res = S.solve(vc_tol=1e-9, nmax=6, hist_len=8)
                    assert (res[0], res[1], res[2], list(res[3])) == (ierr, du, nc, hist), (tag, tail)
                    assert np.array_equal(S.download(1, hip.BUF_U), out), (tag, tail)
                    assert S.info() == (sw1 + sw2 + sw3, un1 + un2 + un3), (tag, tail)
                    S.close()
    finally:
        L.ndsm_hip_debug_tail(1)
