"""The zero first guess of a coarse level, kept out of memory ("Which launch a relax call makes"):
the descent's restriction does not write it and the level's first pre-smoothing launch - an out-of-place fused pass -
takes it from a buffer descriptor of zero records.  Every test here is BITWISE and compares the feature on against
the feature off (ndsm_hip_debug_zero_guess; off = the zeros are written and loaded as before); arrays that must not
be read are filled with NaN first, so a single load of them, or a point of the partner array the launch does not
store, shows in the result.  The forced passes and the small hierarchy are also held against the oracle port."""
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
    yield _lib
    L.ndsm_hip_debug_zero_guess(1)


def _declared(hip, S, level):
    return S.L.ndsm_hip_debug_u_declared_zero(S.h, level)


# the smallest shapes the forced fused pass accepts: even nx, odd nx (the ghost column), a partial last y tile
@pytest.mark.parametrize("ns", ([16, 16, 8], [17, 16, 9], [40, 33, 12]), ids=lambda ns: "x".join(map(str, ns)))
def test_forced_fused_pass_on_a_zero_source(hip, port, ns):
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    rhs = rand_field(shp, 2113)
    zero, nan = np.zeros(shp), np.full(shp, np.nan)
    L = hip.load_library()
    # (op, sweeps): plain one- and two-sweep passes; sweep + residual as the first pass (1), behind a one-sweep
    # pass (2) and behind a two-sweep pass (3)
    runs = [(hip.OP_RELAX_FUSED, 1), (hip.OP_RELAX_FUSED, 2), (hip.OP_RELAX_RES_FUSED, 1), (hip.OP_RELAX_RES_FUSED, 2),
            (hip.OP_RELAX_RES_FUSED, 3)]
    for bcs in ("NDDNDD", "DDDDDD", "DDNDDN"):          # the last one: Neumann faces on z
        S = hip.MGSolver(ns, mesh, bcs)
        for laplace in (False, True):
            if laplace:
                S.zero_rhs()
            else:
                S.upload(1, hip.BUF_RHS, rhs)
            f = zero if laplace else rhs
            for op, nsw in runs:
                what = (ns, bcs, laplace, op, nsw)
                with_res = op == hip.OP_RELAX_RES_FUSED
                # the feature off, from zeros that are in memory
                L.ndsm_hip_debug_zero_guess(0)
                S.upload(1, hip.BUF_U, zero)
                S.upload(1, hip.BUF_UALT, nan)
                S.upload(1, hip.BUF_R, nan)
                S.op(op, 1, nsw)
                u_off, r_off = S.download(1, hip.BUF_U), S.download(1, hip.BUF_R)
                # the oracle: sweeps from zero, then the residual
                want = zero
                for _ in range(nsw):
                    want = port.relax3d(want, f, mesh, bcs)
                assert np.array_equal(u_off, want), what
                if with_res:
                    assert np.array_equal(r_off, port.residual3d(want, f, mesh, bcs)), what
                # the feature on: the source array is NaN and only DECLARED zero, so is its partner
                L.ndsm_hip_debug_zero_guess(1)
                S.upload(1, hip.BUF_U, nan)
                S.upload(1, hip.BUF_UALT, nan)
                S.upload(1, hip.BUF_R, nan)
                S.op(hip.OP_ZERO_U, 1)
                assert _declared(hip, S, 1) == 1, what
                S.op(op, 1, nsw)
                assert _declared(hip, S, 1) == 0, what
                u_on, r_on = S.download(1, hip.BUF_U), S.download(1, hip.BUF_R)
                assert np.array_equal(u_on, u_off), what          # (NaN != NaN: a NaN anywhere fails)
                if with_res:
                    assert np.array_equal(r_on, r_off), what
        S.close()


def _cycles(hip, ns, bcs, on, u, rhs, vc_tol):
    """one V-cycle, then a solve to vc_tol, with every coarse u and its partner filled with NaN first; returns all
    that can be observed: every level's u after the cycle and after the solve, the du history, the cycle count, the
    return code and the coarse sweep counters"""
    L = hip.load_library()
    L.ndsm_hip_debug_zero_guess(1 if on else 0)
    S = hip.MGSolver(ns, uniform_mesh(ns), bcs)
    S.upload(1, hip.BUF_U, u)
    S.upload(1, hip.BUF_RHS, rhs)
    for l in range(2, S.ngrids + 1):
        nan = np.full(S._npshape(l), np.nan)
        S.upload(l, hip.BUF_U, nan)
        S.upload(l, hip.BUF_UALT, nan)
    S.vcycle(1)
    out = [S.download(l, hip.BUF_U) for l in range(1, S.ngrids + 1)]
    assert all(_declared(hip, S, l) == 0 for l in range(1, S.ngrids + 1))
    ierr, du, nc, hist = S.solve(vc_tol=vc_tol, nmax=25, hist_len=25)
    out += [S.download(l, hip.BUF_U) for l in range(1, S.ngrids + 1)]
    res = dict(u=out, ierr=ierr, du=du, nc=nc, hist=hist, info=S.info(), shapes=S.shapes)
    S.close()
    return res


# 256x128x128 and 258x130x130 (odd coarse nx): level 2 has 512 K points and takes the colour passes, so its zeros
# are written as before; 256^3 and 258x256x256 (coarse nx = 129): level 2 has 2 Mi points and more and takes the
# fused pass without forcing - the zero guess stays out of memory there; 64^3: level 2 takes the block-resident
# launch, level 3 the tail launch
@pytest.mark.parametrize("ns", ([256, 128, 128], [258, 130, 130], [256, 256, 256], [258, 256, 256], [64, 64, 64]),
                         ids=lambda ns: "x".join(map(str, ns)))
def test_vcycle_and_solve_same_bits_on_and_off(hip, port, ns):
    shp = tuple(ns[::-1])
    bcs = "NDDNDD"
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    on = _cycles(hip, ns, bcs, True, u, rhs, 1e-6)
    off = _cycles(hip, ns, bcs, False, u, rhs, 1e-6)
    assert on["shapes"] == off["shapes"]
    assert len(on["u"]) == len(off["u"])
    for a, b in zip(on["u"], off["u"]):
        assert np.array_equal(a, b)
    assert on["ierr"] == off["ierr"] == 0
    assert on["nc"] == off["nc"] and on["nc"] >= 2
    assert on["du"] == off["du"] and np.array_equal(on["hist"], off["hist"])
    assert on["info"] == off["info"]
    if ns == [64, 64, 64]:      # the oracle, as test_gpu_parity.py does
        assert np.array_equal(on["u"][0], port.vcycle(u, rhs, uniform_mesh(ns), bcs))


def test_descent_declares_and_every_reader_materialises(hip):
    """256^3: level 2 (128^3) takes the fused pass.  The descent's restriction leaves u(2) alone and declares it zero;
    a download reads zeros; the single restriction still writes them; a prolongation from the declared guess adds
    exactly nothing"""
    ns = [256, 256, 256]
    L = hip.load_library()
    S = hip.MGSolver(ns, uniform_mesh(ns), "NDDNDD")
    r = rand_field(S._npshape(1), 77)
    u1 = rand_field(S._npshape(1), 78)
    nan2 = np.full(S._npshape(2), np.nan)
    try:
        S.upload(1, hip.BUF_R, r)
        # the single operation: zeros in memory
        L.ndsm_hip_debug_zero_guess(1)
        S.upload(2, hip.BUF_U, nan2)
        S.op(hip.OP_RESTRICT, 1)
        assert _declared(hip, S, 2) == 0
        z = S.download(2, hip.BUF_U)
        assert not z.any() and not np.signbit(z).any()
        rhs2 = S.download(2, hip.BUF_RHS)
        # the descent's restriction: the same right-hand side, u(2) declared, a download reads zeros
        S.upload(2, hip.BUF_U, nan2)
        S.upload(2, hip.BUF_RHS, nan2)
        S.op(hip.OP_DESCEND, 1)
        assert _declared(hip, S, 2) == 1
        assert np.array_equal(S.download(2, hip.BUF_RHS), rhs2)
        assert _declared(hip, S, 2) == 1                    # (the right-hand side is not u)
        z = S.download(2, hip.BUF_U)
        assert _declared(hip, S, 2) == 0
        assert not z.any() and not np.signbit(z).any()
        # a reader other than the relax call: the interpolation of a declared guess
        S.upload(2, hip.BUF_U, nan2)
        S.op(hip.OP_DESCEND, 1)
        assert _declared(hip, S, 2) == 1
        S.upload(1, hip.BUF_U, u1)
        S.op(hip.OP_PROLONG, 1)
        assert _declared(hip, S, 2) == 0
        assert np.array_equal(S.download(1, hip.BUF_U), u1)
        # an upload replaces a declared guess
        S.op(hip.OP_DESCEND, 1)
        c = rand_field(S._npshape(2), 79)
        S.upload(2, hip.BUF_U, c)
        assert _declared(hip, S, 2) == 0 and np.array_equal(S.download(2, hip.BUF_U), c)
        # the feature off: the descent writes the zeros
        L.ndsm_hip_debug_zero_guess(0)
        S.upload(2, hip.BUF_U, nan2)
        S.op(hip.OP_DESCEND, 1)
        assert _declared(hip, S, 2) == 0
        assert not S.download(2, hip.BUF_U).any()
    finally:
        L.ndsm_hip_debug_zero_guess(1)
        S.close()
