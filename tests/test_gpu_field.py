"""GPU tests of the current-carrying field (run with -m gpu on an MI355X): VecPot.solve_field, VecPot.helicity
and their one-shot and device-resident forms, on the ABC field

    B = (sin kz + cos ky, sin kx + cos kz, sin ky + cos kx),  k = pi,  curl B = k B,

whose potential-field answer is O(1) wrong.  What is checked: second-order reconstruction of B, the discrete
3-D problems laplace(A_c) = -(curl_h B)_c solved to the tolerance, the same gauge and tangential boundary
values as the potential field, the potential pipeline untouched by field solves on the same handle, the
helicity reduction against numpy on the returned arrays (and its determinism), and the options."""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_inputs import BCS3, uniform_mesh

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
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
    """mesh [x, y, z] (equal spacing, x on [0, 1]) and B in numpy order (3, nz, ny, nx)"""
    mesh = uniform_mesh(ns)
    Z, Y, X = np.meshgrid(mesh[2], mesh[1], mesh[0], indexing="ij")
    k = np.pi
    b = np.stack([np.sin(k * Z) + np.cos(k * Y), np.sin(k * X) + np.cos(k * Z), np.sin(k * Y) + np.cos(k * X)])
    return mesh, b


def weights(mesh):
    """trapezoid weights, numpy order (nz, ny, nx)"""
    ws = []
    for q in mesh:
        h = q[1] - q[0]
        w = np.full(len(q), h)
        w[0] = w[-1] = 0.5 * h
        ws.append(w)
    return ws[2][:, None, None] * ws[1][None, :, None] * ws[0][None, None, :]


def grad(f, mesh, axis):
    """d/dq with derivq's stencil (centred inside, 3-point one-sided on the end planes); numpy axis order"""
    return np.gradient(f, mesh[axis][1] - mesh[axis][0], axis=2 - axis, edge_order=2)


def curl(v, mesh):
    return np.stack([grad(v[2], mesh, 1) - grad(v[1], mesh, 2), grad(v[0], mesh, 2) - grad(v[2], mesh, 0),
                     grad(v[1], mesh, 0) - grad(v[0], mesh, 1)])


def div(v, mesh):
    return grad(v[0], mesh, 0) + grad(v[1], mesh, 1) + grad(v[2], mesh, 2)


def recon(brec, b, w):
    e = brec - b
    return np.abs(e).max(), np.sqrt((w * (e * e).sum(axis=0)).sum() / w.sum())


def dirichlet_faces(a, c):
    """the four faces on which component c carries Dirichlet data (every face but its normal pair)"""
    out = []
    for ax in range(3):
        if ax == c:
            continue
        sl = [slice(None)] * 3
        for end in (0, -1):
            sl[2 - ax] = end
            out.append(a[c][tuple(sl)])
    return out


_RUNS = {}


def field_run(hip, n, flxcrl=False):
    """(mesh, b, solve result, solve_field result) at n^3, one handle, cached for the module"""
    key = (n, flxcrl)
    if key not in _RUNS:
        import ndsm_amd
        mesh, b = abc_field([n, n, n])
        V = ndsm_amd.VecPot(*mesh)
        pot = V.solve(b, vc_tol=VC_TOL, flxcrl=flxcrl)
        fld = V.solve_field(b, vc_tol=VC_TOL, flxcrl=flxcrl)
        V.close()
        _RUNS[key] = (mesh, b, pot, fld)
    return _RUNS[key]


@pytest.mark.parametrize("flxcrl", (False, True), ids=("FLXCRL0", "FLXCRL1"))
def test_reconstruction_is_second_order(hip, flxcrl):
    errs = []
    for n in (17, 33, 65):
        mesh, b, pot, fld = field_run(hip, n, flxcrl)
        assert fld[0] == 0 and pot[0] == 0
        w = weights(mesh)
        emax, erms = recon(fld[2], b, w)
        errs.append((emax, erms))
        assert recon(pot[2], b, w)[1] >= 0.5           # the potential field alone is O(1) off
    for (m0, r0), (m1, r1) in zip(errs, errs[1:]):
        assert m0 / m1 >= 3.5 and r0 / r1 >= 3.5, errs
    assert errs[-1][0] <= 1.5e-3 and errs[-1][1] <= 1.5e-3, errs


@pytest.mark.parametrize("n", (17, 33, 65))
def test_discrete_problems_solved(hip, port, n):
    mesh, b, pot, fld = field_run(hip, n)
    A = fld[1]
    J = curl(b, mesh)
    for c in range(3):
        r = port.residual3d(A[c], -J[c], mesh, BCS3[c])
        assert np.abs(r).max() <= 1e-9 * np.abs(J[c]).max(), (c, np.abs(r).max())


@pytest.mark.parametrize("ns", ([33, 33, 33], [33, 25, 41], [40, 24, 32]), ids=lambda s: "x".join(map(str, s)))
def test_same_gauge_and_boundary_values(hip, ns):
    """odd and anisotropic shapes with equal spacing: the tangential Dirichlet data of A are those of A_p bit for
    bit, A is divergence-free to the tolerance, B is reconstructed to O(h^2)"""
    import ndsm_amd
    mesh, b = abc_field(ns)
    V = ndsm_amd.VecPot(*mesh)
    ie0, Ap, Bp = V.solve(b, vc_tol=VC_TOL)
    ie1, A, Br = V.solve_field(b, vc_tol=VC_TOL)
    V.close()
    assert ie0 == 0 and ie1 == 0
    for c in range(3):
        for fa, fp in zip(dirichlet_faces(A, c), dirichlet_faces(Ap, c)):
            assert np.array_equal(fa, fp), c
    assert np.abs(div(A, mesh)).max() <= 1e-8 * np.abs(A).max()
    h = mesh[0][1] - mesh[0][0]
    assert recon(Br, b, weights(mesh))[1] <= 8.0 * h * h


def _order_check(n):
    """solve -> solve_field -> helicity -> solve on one handle, against a fresh handle's solve"""
    import ndsm_amd
    mesh, b = abc_field([n, n, n])
    F = ndsm_amd.VecPot(*mesh)
    want = F.solve(b, vc_tol=VC_TOL)
    F.close()
    V = ndsm_amd.VecPot(*mesh)
    s1 = V.solve(b, vc_tol=VC_TOL)
    fld = V.solve_field(b, vc_tol=VC_TOL)
    hel = V.helicity(b, vc_tol=VC_TOL, return_fields=True)
    s2 = V.solve(b, vc_tol=VC_TOL)
    V.close()
    for got in (s1, s2):
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.array_equal(hel.A_p, want[1]) and np.array_equal(hel.B_p, want[2])
    assert np.array_equal(hel.A, fld[1])          # helicity's field solve is solve_field's, bit for bit
    return "order ok"


@pytest.mark.parametrize("n", (17, 33))
def test_potential_part_unchanged(hip, n):
    assert _order_check(n) == "order ok"


def test_potential_part_unchanged_without_lanes(hip):
    env = dict(os.environ, NDSM_HIP_NO_SIDE3D="1")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_field as t; "
            "print(t._order_check(33))" % (os.path.dirname(HERE), HERE))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "order ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def _numpy_helicity(A, Ap, b, Bp, Br, mesh):
    w = weights(mesh)
    d = b - Bp
    terms = {"H_R": w * ((A + Ap) * d).sum(axis=0), "H_J": w * ((A - Ap) * d).sum(axis=0),
             "E": 0.5 * w * (b * b).sum(axis=0), "E_p": 0.5 * w * (Bp * Bp).sum(axis=0)}
    return {k: (v.sum(), np.abs(v).sum()) for k, v in terms.items()}


@pytest.mark.parametrize("n", (17, 33, 65))
def test_helicity_numbers(hip, n):
    import ndsm_amd
    mesh, b = abc_field([n, n, n])
    V = ndsm_amd.VecPot(*mesh)
    h1 = V.helicity(b, vc_tol=VC_TOL, return_fields=True)
    h2 = V.helicity(b, vc_tol=VC_TOL)
    ie, A, Br = V.solve_field(b, vc_tol=VC_TOL)
    V.close()
    assert h1.ierr == 0 and ie == 0 and np.array_equal(h1.A, A)
    # the reduction against numpy on the returned arrays
    ref = _numpy_helicity(h1.A, h1.A_p, b, h1.B_p, Br, mesh)
    for k, (val, scale) in ref.items():
        assert abs(getattr(h1, k) - val) <= 1e-12 * scale, (k, getattr(h1, k), val)
    emax, erms = recon(Br, b, weights(mesh))
    assert h1.recon_max == emax
    assert abs(h1.recon_rms - erms) <= 1e-12 * erms
    h = mesh[0][1] - mesh[0][0]
    assert abs(h1.divB_max - np.abs(div(b, mesh)).max()) <= 1e-14 * np.abs(b).max() / h
    assert abs(h1.divA_max - np.abs(div(h1.A, mesh)).max()) <= 1e-14 * np.abs(h1.A).max() / h
    # deterministic, and physically sensible
    assert h1[:10] == h2[:10]
    assert h1.E_free == h1.E - h1.E_p and h1.E_free > 0
    if n == 65:
        assert abs(h1.H_R - 0.47064) <= 2e-3, h1.H_R
        w = weights(mesh)
        berger = (w * ((h1.A * b).sum(axis=0) - (h1.A_p * h1.B_p).sum(axis=0))).sum()
        assert abs(berger - h1.H_R) <= 2e-3 * abs(h1.H_R), (berger, h1.H_R)


def test_helicity_of_the_potential_field_vanishes(hip):
    """B_p fed back in: H_R is a discretisation error and falls at second order"""
    import ndsm_amd
    hr = []
    for n in (33, 65):
        mesh, b = abc_field([n, n, n])
        bp = field_run(hip, n)[2][2]
        hr.append(abs(ndsm_amd.relative_helicity(*mesh, bp, vc_tol=VC_TOL).H_R))
    assert hr[0] / hr[1] >= 3.0, hr


def test_device_entries_give_the_host_bits(hip):
    import ndsm_amd
    mesh, b = abc_field([33, 25, 41])
    V = ndsm_amd.VecPot(*mesh)
    a0 = 0.01 * np.cos(b)                       # a non-zero initial guess goes in both ways alike
    f_host = V.solve_field(b, a_init=a0, vc_tol=VC_TOL)
    f_dev = V.solve_field(b, a_init=a0, vc_tol=VC_TOL, device=True)
    h_host = V.helicity(b, vc_tol=VC_TOL, return_fields=True)
    h_dev = V.helicity(b, vc_tol=VC_TOL, return_fields=True, device=True)
    V.close()
    assert f_host[0] == f_dev[0] == 0
    assert np.array_equal(f_host[1], f_dev[1]) and np.array_equal(f_host[2], f_dev[2])
    assert h_host[:10] == h_dev[:10]
    for k in ("A", "A_p", "B_p"):
        assert np.array_equal(getattr(h_host, k), getattr(h_dev, k)), k


def test_options_mean_level_cap_and_iteration_limit(hip):
    import ndsm_amd
    L = ndsm_amd.load_library()
    mesh, b = abc_field([33, 33, 33])
    w = weights(mesh)
    base = recon(field_run(hip, 33)[3][2], b, w)[1]
    for kw in (dict(mean=True), dict(ngrids=3)):
        ng = kw.pop("ngrids", 0)
        V = ndsm_amd.VecPot(*mesh, ngrids=ng)
        ie, A, Br = V.solve_field(b, vc_tol=VC_TOL, **kw)
        hel = V.helicity(b, vc_tol=VC_TOL, **kw)
        V.close()
        assert ie == 0 and hel.ierr == 0, (kw, ng)
        assert recon(Br, b, w)[1] <= 1.05 * base, (kw, ng)
        assert abs(hel.H_R - 0.471) < 5e-3
    V = ndsm_amd.VecPot(*mesh)
    ie, A, Br = V.solve_field(b, vc_tol=VC_TOL, ncycles_max=1)
    assert ie == 1 and V.last_ioptc[3] == 1                            # IOPT_IERR (slot 3) holds the same
    assert V.last_ioptc[L.get_iopt_fail3d()] == 0b111
    hel = V.helicity(b, vc_tol=VC_TOL, ncycles_max=1)
    assert hel.ierr == 1 and V.last_ioptc[L.get_iopt_fail3d()] == 0b111111
    ie, A, Br = V.solve_field(b, vc_tol=VC_TOL)                        # and the handle is fine afterwards
    V.close()
    assert ie == 0 and np.array_equal(Br, field_run(hip, 33)[3][2])


def test_mixed_precision(hip):
    import ndsm_amd
    mesh, b = abc_field([64, 64, 64])
    V = ndsm_amd.VecPot(*mesh)
    ie0, A0, B0 = V.solve_field(b, vc_tol=VC_TOL)
    ie1, A1, B1 = V.solve_field(b, vc_tol=VC_TOL, mixed_precision=2)
    h0 = V.helicity(b, vc_tol=VC_TOL)
    h1 = V.helicity(b, vc_tol=VC_TOL, mixed_precision=2)
    V.close()
    assert ie0 == ie1 == 0
    h = mesh[0][1] - mesh[0][0]
    assert not np.array_equal(A0, A1)                  # the fp32 correction cycle did run
    assert np.abs(A1 - A0).max() <= 1e-9 * np.abs(A0).max()
    assert np.abs(B1 - B0).max() <= 1e-9 * np.abs(A0).max() * 4 / h
    assert abs(h1.H_R - h0.H_R) <= 1e-8 * abs(h0.H_R)


def test_errors_are_clean(hip):
    import ctypes
    import ndsm_amd
    mesh, b = abc_field([17, 17, 17])
    V = ndsm_amd.VecPot(*mesh)
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        V.solve_field(b[:, :, :, :16])
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        V.helicity(b[:2])
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.relative_helicity(mesh[0], mesh[1], mesh[2][:16], b)
    assert V.solve_field(b, vc_tol=VC_TOL)[0] == 0
    V.close()
    # a grid whose fields cannot fit in HBM (2048^3: 64 GiB per array, 15 of them): refused before any allocation
    # or launch - the tiny device buffers below are never touched
    L = ndsm_amd.load_library()
    n = 2048
    x = np.linspace(0, 1, n)
    V = ndsm_amd.VecPot(x, x, x)
    bufs = []
    for _ in range(4):
        p = ctypes.c_void_p()
        assert L.ndsm_hip_device_alloc(64, ctypes.byref(p)) == 0
        bufs.append(p)
    ioptc, ropt = V._options(10000, 1024, 1e-13, VC_TOL, 5, False, 0, False)
    out = np.zeros(8)
    dp = ctypes.POINTER(ctypes.c_double)
    try:
        rc = L.ndsm_hip_vecpot_helicity_device(V.h, ioptc.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                               ropt.ctypes.data_as(dp), *bufs, out.ctypes.data_as(dp))
        assert rc == 9001, rc
        rc = L.ndsm_hip_vecpot_solve_field_device(V.h, ioptc.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                  ropt.ctypes.data_as(dp), bufs[0], bufs[1])
        assert rc == 9001, rc
    finally:
        for p in bufs:
            L.ndsm_hip_device_free(p)
        V.close()
    # nothing leaks into the next call
    assert ndsm_amd.vector_potential_field(*mesh, b, vc_tol=VC_TOL)[0] == 0
