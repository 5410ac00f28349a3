"""GPU tests of the nonlinear force-free field (run with -m gpu on an MI355X): VecPot.solve_current, VecPot.force_free
and their one-shot and device-resident forms.  What is checked: the solve for a prescribed current against the discrete
problems and against solve_field; the Grad-Rubin driver against the chain alpha_map -> numpy alpha * b -> solve_current
that it is documented to be, bit for bit; alpha0 = 0 (the potential field at every pass); a flux tube with a compact
current, force-free in closed form, as the fixed point and as the target from the potential start; determinism, the
stopping rule, the potential pipeline untouched on the same handle, the argument checks."""
import numpy as np
import pytest

from alpha_model import ZLO, flux_tube
from golden_inputs import BCS3, aniso_mesh, uniform_mesh
from line_model import sheared

pytestmark = pytest.mark.gpu

VC_TOL = 1e-12


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def abc_field(ns):
    """test_gpu_field.py's: mesh [x, y, z] (equal spacing, x on [0, 1]) and B in numpy order (3, nz, ny, nx)"""
    mesh = uniform_mesh(ns)
    Z, Y, X = np.meshgrid(mesh[2], mesh[1], mesh[0], indexing="ij")
    k = np.pi
    b = np.stack([np.sin(k * Z) + np.cos(k * Y), np.sin(k * X) + np.cos(k * Z), np.sin(k * Y) + np.cos(k * X)])
    return mesh, b


def grad(f, mesh, axis):
    """d/dq with derivq's stencil (centred inside, 3-point one-sided on the end planes); numpy axis order"""
    return np.gradient(f, mesh[axis][1] - mesh[axis][0], axis=2 - axis, edge_order=2)


def curl(v, mesh):
    return np.stack([grad(v[2], mesh, 1) - grad(v[1], mesh, 2), grad(v[0], mesh, 2) - grad(v[2], mesh, 0),
                     grad(v[1], mesh, 0) - grad(v[0], mesh, 1)])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def tube_case(n, qa=1.0):
    """the flux tube of alpha_model on the box [0,1] x [0,1] x [0,1/2] with equal spacings, n points along x"""
    mesh = uniform_mesh([n, n, (n - 1) // 2 + 1])
    b, alpha, r, a = flux_tube(mesh, qa)
    return mesh, b, alpha, r <= 0.8 * a


def weights(mesh):
    """trapezoid weights, numpy order (nz, ny, nx)"""
    ws = []
    for q in mesh:
        h = q[1] - q[0]
        w = np.full(len(q), h)
        w[0] = w[-1] = 0.5 * h
        ws.append(w)
    return ws[2][:, None, None] * ws[1][None, :, None] * ws[0][None, None, :]


def history_row(mesh, b_new, b_old):
    """hist[k][0..2] of include/ndsm_hip.h in numpy, on this file's own curl: max |B_new - B_old|, 1/2 sum w |B|^2,
    sum w |J x B| / |B| over sum w |J| (points with |B| not > 0 skipped; 0 when the denominator is 0)"""
    w = weights(mesh)
    j = curl(b_new, mesh)
    bm = np.sqrt((b_new * b_new).sum(axis=0))
    ok = bm > 0.0
    cross = np.cross(j, b_new, axis=0)
    num = (w * np.sqrt((cross * cross).sum(axis=0)) / np.where(ok, bm, 1.0))[ok].sum()
    den = (w * np.sqrt((j * j).sum(axis=0)))[ok].sum()
    return (float(np.abs(b_new - b_old).max()), float(0.5 * (w * (b_new * b_new).sum(axis=0)).sum()),
            float(num / den) if den > 0.0 else 0.0)


def check_history(mesh, hist, fields):
    """every row of hist against numpy on the fields B^0 .. B^m of the passes: [0] exactly (a maximum of exact
    differences has no rounding of its own), [1] to 1e-13 and [2] to 1e-12 relative.  Both sides sum positive terms in
    blocks and trees (numpy pairwise; the kernel a row walk per thread, then halving trees), so each sum is good to
    about (tree depth + block length) eps, ~1e2 eps: 1e-13 is 450 eps.  [2] is a quotient of two such sums whose
    terms carry the rounding of two restatements of curl_h, each a difference of products that may cancel: ten times
    the room."""
    assert len(hist) == len(fields) - 1
    for k in range(len(hist)):
        change, energy, sine = history_row(mesh, fields[k + 1], fields[k])
        print("pass", k, "hist", hist[k].tolist(), "numpy", (change, energy, sine))
        assert hist[k, 0] == change
        assert abs(hist[k, 1] - energy) <= 1e-13 * energy
        assert abs(hist[k, 2] - sine) <= 1e-12 * sine


def core_error(f, b, core):
    return float(np.abs(f - b)[:, core].max())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the solve for a prescribed current
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (17, 33))
def test_solve_current_on_the_abc_field(hip, port, n):
    """with J = curl_h B (numpy) the discrete problems laplace_7(A_c) = -J_c hold to solve_field's bound, and A is
    solve_field's to 1e-10 max |A|: the two right-hand sides differ by rounding only and both solves run to vc_tol =
    1e-12; with J = 0 the field is solve()'s potential field to the same relative 1e-10; the device-resident entry
    gives the host entry's bits"""
    import ndsm_amd
    mesh, b = abc_field([n, n, n])
    J = curl(b, mesh)
    V = ndsm_amd.VecPot(*mesh)
    try:
        ierr, A, B = V.solve_current(b, J, vc_tol=VC_TOL)
        ierr_f, Af, Bf = V.solve_field(b, vc_tol=VC_TOL)
        ierr_p, Ap, Bp = V.solve(b, vc_tol=VC_TOL)
        ierr_0, A0, B0 = V.solve_current(b, np.zeros_like(b), vc_tol=VC_TOL)
        ierr_d, Ad, Bd = V.solve_current(b, J, vc_tol=VC_TOL, device=True)
        one = ndsm_amd.vector_potential_current(*mesh, b, J, vc_tol=VC_TOL)
    finally:
        V.close()
    assert ierr == 0 and ierr_f == 0 and ierr_p == 0 and ierr_0 == 0 and ierr_d == 0
    for c in range(3):
        r = port.residual3d(A[c], -J[c], mesh, BCS3[c])
        print(n, c, "max residual / max |J_c|:", np.abs(r).max() / np.abs(J[c]).max())
        assert np.abs(r).max() <= 1e-9 * np.abs(J[c]).max(), (c, np.abs(r).max())
    print(n, "max |A - A_solve_field| / max |A|:", np.abs(A - Af).max() / np.abs(Af).max(),
          "J = 0: max |B - B_p| / max |B_p|:", np.abs(B0 - Bp).max() / np.abs(Bp).max())
    assert np.abs(A - Af).max() <= 1e-10 * np.abs(Af).max()
    assert np.abs(B0 - Bp).max() <= 1e-10 * np.abs(Bp).max()
    assert same_bits(A, Ad) and same_bits(B, Bd)
    assert one[0] == 0 and same_bits(one[1], A) and same_bits(one[2], B)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the driver against the chain it is documented to be
# ---------------------------------------------------------------------------------------------------------------------
def chain(V, b, alpha0, passes, step, **opts):
    """alpha_map -> numpy j = alpha * b -> solve_current(b's B.n, j, the last A), `passes` times from (b, A = 0);
    returns the last A, the fields B^0 .. B^passes and the last alpha"""
    fields, ak, alpha = [b], None, None
    for _ in range(passes):
        alpha, _status = V.alpha_map(fields[-1], alpha0, step=step)
        ierr, ak, bk = V.solve_current(b, alpha * fields[-1], a_init=ak, **opts)
        assert ierr == 0
        fields.append(bk)
    return ak, fields, alpha


@pytest.mark.parametrize("kind,shape", [("aniso", (17, 12, 9)), ("uniform", (17, 17, 17))])
def test_driver_equals_the_hand_built_chain(hip, kind, shape):
    """force_free(start="given") with niter_max = 1 and 3 equals one and three chained steps bit for bit in A, B and
    alpha: the driver runs the same kernels in the same order, and -(alpha * b) is one rounding and a sign on both
    sides.  The sheared field has B_z = 1 > 0 everywhere; alpha0 is boundary_alpha's.  The chain's fields are on the
    host, so every history row is checked against numpy on them (check_history): the change exactly, the energy and
    the current-weighted sine to rounding."""
    import ndsm_amd
    mesh = (aniso_mesh if kind == "aniso" else uniform_mesh)(shape)
    b = sheared(mesh)
    alpha0 = ndsm_amd.boundary_alpha(mesh[0], mesh[1], b, 1e-3)
    assert np.abs(alpha0).max() > 0.1
    V = ndsm_amd.VecPot(*mesh)
    try:
        for passes in (1, 3):
            ierr, A, B, alpha, status, hist = V.force_free(b, alpha0, start="given", niter_max=passes, step=0.5,
                                                           vc_tol=VC_TOL)
            ak, fields, al = chain(V, b, alpha0, passes, 0.5, vc_tol=VC_TOL)
            bk = fields[-1]
            print(kind, passes, "max |A - chain|:", np.abs(A - ak).max(), "max |B - chain|:", np.abs(B - bk).max(),
                  "max |alpha - chain|:", np.abs(alpha - al).max(), "hist:", hist.tolist())
            assert ierr == 0 and hist.shape == (passes, 4)
            assert same_bits(alpha, al)
            assert same_bits(A, ak)
            assert same_bits(B, bk)
            assert hist[-1, 3] == (status == ZLO).sum() > 0
            check_history(mesh, hist, fields)
        # the device-resident entry gives the same bits, the history included
        dev = V.force_free(b, alpha0, start="given", niter_max=3, step=0.5, vc_tol=VC_TOL, device=True)
        for got, want in zip(dev[1:], (A, B, alpha, status, hist)):
            assert np.array_equal(got, want)
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. alpha0 = 0: the potential field at every pass
# ---------------------------------------------------------------------------------------------------------------------
def test_zero_alpha_gives_the_potential_field(hip):
    import ndsm_amd
    mesh, b = abc_field([17, 17, 17])
    zero = np.zeros((17, 17))
    V = ndsm_amd.VecPot(*mesh)
    try:
        ierr_p, Ap, Bp = V.solve(b, vc_tol=VC_TOL)
        _alpha, st0 = V.alpha_map(Bp, zero, step=0.5)
        scale = np.abs(Bp).max()
        for passes in (1, 2, 3):
            ierr, A, B, alpha, status, hist = V.force_free(b, zero, niter_max=passes, step=0.5, vc_tol=VC_TOL)
            assert ierr == 0 and ierr_p == 0 and len(hist) == passes
            print(passes, "max |B - B_p| / max |B_p|:", np.abs(B - Bp).max() / scale, "hist:", hist.tolist())
            assert np.abs(B - Bp).max() <= 1e-10 * scale
            assert np.all(alpha == 0.0)
            assert np.all(hist[:, 0] <= 1e-10 * scale)
            # the first pass maps the potential field itself (the bits of solve()); the last pass's map comes back
            assert hist[0, 3] == (st0 == ZLO).sum()
            assert hist[-1, 3] == (status == ZLO).sum()
    finally:
        V.close()


def test_history_of_the_tube_and_of_a_zero_field(hip):
    """The history against numpy where the current is strong (the flux tube at n = 17, start="given": B^0 is on the
    host, B^1 comes back), and on the zero field: B.n = 0 gives B^1 = 0 at every node, so every point has |B| not > 0
    and is skipped, the denominator is 0 and the sine is 0 by definition, not NaN; no line starts (all NULL), the
    energy and the change are 0."""
    import ndsm_amd
    mesh, b, alpha, _core = tube_case(17)
    V = ndsm_amd.VecPot(*mesh)
    try:
        ierr, _A, B1, _al, _st, hist = V.force_free(b, alpha[0], start="given", niter_max=1, step=0.5, vc_tol=VC_TOL)
        assert ierr == 0
        check_history(mesh, hist, [b, B1])
        assert 0.0 < hist[0, 2] < 1.0
        zero = np.zeros_like(b)
        ierr, A, B, al, st, hist = V.force_free(zero, alpha[0], start="given", niter_max=2, step=0.5, vc_tol=VC_TOL)
        print("zero field: hist", hist.tolist(), "max |B|", np.abs(B).max())
        assert ierr == 0 and hist.shape == (2, 4)
        assert np.all(B == 0.0) and np.all(al == 0.0) and np.all(st == 7)
        assert np.all(hist == 0.0)
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the flux tube: fixed point, and the target from the potential start
# ---------------------------------------------------------------------------------------------------------------------
_TUBE = {}


def tube_pass(n):
    """(error of one pass from the tube itself, error of the potential field) over r <= 0.8 a, cached"""
    if n not in _TUBE:
        import ndsm_amd
        mesh, b, alpha, core = tube_case(n)
        V = ndsm_amd.VecPot(*mesh)
        try:
            ierr, _A, B1, _al, status, _hist = V.force_free(b, alpha[0], start="given", niter_max=1, step=0.5)
            ierr_p, _Ap, Bp = V.solve(b)
        finally:
            V.close()
        assert ierr == 0 and ierr_p == 0
        assert np.all(status[core] == ZLO)
        _TUBE[n] = (core_error(B1, b, core), core_error(Bp, b, core))
    return _TUBE[n]


def test_flux_tube_is_a_fixed_point(hip):
    """One pass from the tube itself (q a = 1, alpha0 its analytic alpha on k = 0, polarity +1) returns the tube up to
    the discretisation: the max error of B^1 over r <= 0.8 a falls from n = 17 to 33 to 65, and at each n it is below
    the error of the potential field of the same B.n.  Measured on an MI355X (|B| <= 1), B^1 / potential field:
    3.13e-2 / 0.502 (n = 17), 8.12e-3 / 0.529 (33), 2.05e-3 / 0.532 (65): ratios 3.9 and 4.0 per halving.  (At q a =
    0.5: 8.20e-3 / 0.321, 2.07e-3 / 0.355, 1.39e-3 / 0.363.)  DESIGN.md section 25."""
    errs = [tube_pass(n) for n in (17, 33, 65)]
    print("flux tube, one pass from the tube: (error of B^1, error of the potential field) at n = 17, 33, 65:", errs)
    for (e1, ep) in errs:
        assert e1 < ep, errs
    assert errs[0][0] > errs[1][0] > errs[2][0], errs


def test_flux_tube_from_the_potential_start(hip):
    """n = 33, eight passes from the potential field: the change per pass falls, the final field is closer to the tube
    over r <= 0.8 a than the potential field, and the current-weighted sine ends below the first pass's.  Measured on
    an MI355X: the change per pass 0.513, 0.286, 0.0931, 0.0726, 0.0198, 0.0160, 0.00435, 0.00349; the sine 0.475,
    0.102, 0.0765, 0.0262, 0.0250, 0.0116, 0.0149, 0.0114 (not monotonic once it is near the 1.1e-2 of the tube's own
    curl_h B at this n); the final error 8.12e-3 against the potential field's 0.529.  DESIGN.md section 25."""
    import ndsm_amd
    mesh, b, alpha, core = tube_case(33)
    V = ndsm_amd.VecPot(*mesh)
    try:
        ierr, _A, B, _al, _st, hist = V.force_free(b, alpha[0], niter_max=8, step=0.5)
        _ip, _Ap, Bp = V.solve(b)
    finally:
        V.close()
    e, ep = core_error(B, b, core), core_error(Bp, b, core)
    print("flux tube from the potential start, n = 33: hist =", hist.tolist(), "error:", e, "potential:", ep)
    assert ierr == 0 and len(hist) == 8
    assert hist[-1, 0] < hist[0, 0]
    assert e < ep
    assert hist[-1, 2] < hist[0, 2]
    assert hist[-1, 1] > hist[0, 1] * 0.5 and np.all(np.isfinite(hist))


# ---------------------------------------------------------------------------------------------------------------------
# 5. determinism, the stopping rule, the potential pipeline on the same handle, arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_repeatable_stopping_rule_and_untouched_pipeline(hip):
    import ndsm_amd
    mesh = uniform_mesh((17, 17, 17))
    b = sheared(mesh)
    alpha0 = ndsm_amd.boundary_alpha(mesh[0], mesh[1], b, 1e-3)
    V = ndsm_amd.VecPot(*mesh)
    try:
        before = V.solve(b, vc_tol=VC_TOL)
        first = V.force_free(b, alpha0, niter_max=4, step=0.5, vc_tol=VC_TOL)
        again = V.force_free(b, alpha0, niter_max=4, step=0.5, vc_tol=VC_TOL)
        after = V.solve(b, vc_tol=VC_TOL)
        hist = first[5]
        assert len(hist) == 4
        for x, y in zip(first[1:], again[1:]):
            assert np.array_equal(x, y)
        assert same_bits(hist, again[5])
        assert before[0] == after[0] and same_bits(before[1], after[1]) and same_bits(before[2], after[2])
        # tol: the loop stops after the first pass whose change is below it
        big = V.force_free(b, alpha0, niter_max=4, tol=1e300, step=0.5, vc_tol=VC_TOL)
        assert len(big[5]) == 1 and same_bits(big[5], hist[:1])
        tol = float(hist[1:, 0].max()) * 1.0000001
        k = int(np.nonzero(hist[:, 0] < tol)[0][0])
        some = V.force_free(b, alpha0, niter_max=4, tol=tol, step=0.5, vc_tol=VC_TOL)
        print("hist[:, 0] =", hist[:, 0].tolist(), "tol =", tol, "passes:", len(some[5]))
        assert len(some[5]) == k + 1 and same_bits(some[5], hist[:k + 1])
        one = ndsm_amd.force_free_field(*mesh, b, alpha0, niter_max=4, step=0.5, vc_tol=VC_TOL)
        for x, y in zip(first[1:], one[1:]):
            assert np.array_equal(x, y)
    finally:
        V.close()


def test_bad_scalars_and_null_arrays(hip):
    import ctypes
    import ndsm_amd
    mesh = uniform_mesh((9, 9, 9))
    b = sheared(mesh)
    alpha0 = np.ones((9, 9))
    V = ndsm_amd.VecPot(*mesh)
    try:
        for kw in (dict(polarity=0), dict(polarity=2), dict(niter_max=0), dict(niter_max=-1), dict(tol=-1e-3),
                   dict(tol=float("inf")), dict(tol=float("nan"))):
            with pytest.raises(hip.NdsmHipError, match="9004"):
                V.force_free(b, alpha0, **kw)
        # the C entry itself: start, step and max_steps (the Python layer refuses these before the call), NULL arrays
        L = V.L
        ioptc, ropt = V._options(10000, 1024, 1e-13, 1e-10, 5, False, False, False)
        B, a0 = np.ascontiguousarray(b).reshape(-1).copy(), alpha0.reshape(-1).copy()
        A, alpha = np.zeros(B.size), np.full(B.size // 3, 7.0)
        hist, niter = np.full((2, 4), 7.0), ctypes.c_int(7)

        def call(pB, pa0, start, step, ms, pA, pal, phist):
            B[:] = b.reshape(-1)                              # (a failed call clears its in/out arrays too)
            return L.ndsm_hip_vecpot_nlfff(V.h, ioptc.ctypes.data_as(hip._ip), hip._d(ropt), pB, pa0, 1, start, 2, 0.0,
                                           step, ms, pA, pal, None, phist, ctypes.byref(niter))
        ptr = [v.ctypes.data for v in (B, a0, A, alpha)]
        for start, step, ms in ((2, 0.5, 10), (-1, 0.5, 10), (0, 0.0, 10), (0, float("nan"), 10), (0, 0.5, 0)):
            assert call(ptr[0], ptr[1], start, step, ms, ptr[2], ptr[3], hip._d(hist)) == 9004, (start, step, ms)
            assert niter.value == 0 and np.all(hist == 0.0) and np.all(alpha == 0.0)
            hist[:], alpha[:], niter.value = 7.0, 7.0, 7
        assert call(None, ptr[1], 0, 0.5, 10, ptr[2], ptr[3], hip._d(hist)) == 9002
        assert call(ptr[0], None, 0, 0.5, 10, ptr[2], ptr[3], hip._d(hist)) == 9002
        assert call(ptr[0], ptr[1], 0, 0.5, 10, None, ptr[3], hip._d(hist)) == 9002
        assert call(ptr[0], ptr[1], 0, 0.5, 10, ptr[2], None, hip._d(hist)) == 9002
        assert call(ptr[0], ptr[1], 0, 0.5, 10, ptr[2], ptr[3], None) == 9002
        # and a good call with status = NULL runs
        assert call(ptr[0], ptr[1], 0, 0.5, 10, ptr[2], ptr[3], hip._d(hist)) == 0 and niter.value == 2
        with pytest.raises(hip.NdsmHipError, match="9002"):
            V.solve_current(b, np.zeros((3, 9, 9, 8)))
    finally:
        V.close()
