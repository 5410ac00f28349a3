"""GPU tests on meshes with a spacing of its own on every axis and no origin at 0 (run with -m gpu on an MI355X).

With one spacing for all three axes and the origin at 0, a kernel that reads the wrong axis's weight or spacing, or
a coordinate measured from the wrong origin, still returns the right bits.  Here the mesh is golden_inputs.aniso_mesh
(h_y = 0.73 h_x, h_z = 1.37 h_x, origins 0.25, -0.4, 1.1).  The per-operator, transfer, large-level, slab and
mixed-precision cases are 'aniso-' parameters of the tests in test_gpu_parity.py, test_gpu_project.py and
test_gpu_devore.py; this file holds the checks that have no uniform-mesh test to take a parameter.  Checkers: the
oracle (pinned to the reference on these meshes by test_oracle.py), the reference's own outputs
(golden/reference_aniso.json, golden/pipeline_aniso_*.npz), the host face phase, and numpy restatements.

Nothing downstream of the face phase is checked against the analytic answer: with unequal spacings the reference's
quirk Q4 (face fluxes with dq(1) dq(2) on every face, grad chi with the normal spacing), which the library keeps on
purpose, makes the potential field inconsistent."""
import ctypes
import json
import os

import numpy as np
import pytest

import test_gpu_field as fld
from golden_inputs import ANISO_SHAPES_3D, BCS3, aniso_mesh, aniso_pipeline_cases, manufactured_poisson
from test_gpu_devore import abc, flux

pytestmark = pytest.mark.gpu

VC_TOL = 1e-12
WIDE = [300, 40, 60]         # rows longer than a 256-thread block, more rows (ny nz) than the 2048 reduction blocks


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


def _case(name):
    return [c for c in aniso_pipeline_cases() if c[0] == name][0][1:]


# ---------------------------------------------------------------------------
# whole solves against the oracle and the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ns", ANISO_SHAPES_3D, ids=_tag)
def test_poisson_solves_vs_oracle(hip, port, golden_dir, ns):
    """poisson_solve and MGSolver.solve on the manufactured problems of the three components' BC sets: du history,
    cycle count and solution bits of the oracle's solve_bvp, and (first shape) the reference's own history"""
    with open(os.path.join(golden_dir, "reference_aniso.json")) as fh:
        want = json.load(fh)
    mesh = aniso_mesh(ns)
    for bcs in BCS3:
        us, rhs = manufactured_poisson(mesh, bcs)
        ie2, u2, du2, h2, nc2, _sw = port.solve_bvp(np.zeros_like(us), rhs, mesh, bcs, hist_len=64)
        ie, u, du, hist, nc = hip.poisson_solve(np.zeros_like(us), rhs, mesh, bcs, hist_len=64)
        assert ie == ie2 == 0 and nc == nc2, (bcs, nc, nc2)
        assert list(hist) == list(h2[:nc2]) and du == du2, bcs
        assert np.array_equal(u, u2), bcs
        S = hip.MGSolver(ns, mesh, bcs)
        S.upload(1, hip.BUF_U, np.zeros_like(us))
        S.upload(1, hip.BUF_RHS, rhs)
        ie3, du3, nc3, h3 = S.solve(hist_len=64)
        u3 = S.download(1, hip.BUF_U)
        S.close()
        assert (ie3, nc3, du3) == (0, nc2, du2) and list(h3) == list(h2[:nc2]), bcs
        assert np.array_equal(u3, u2), bcs
        key = f"solve_{_tag(ns)}_{bcs}"
        if key in want:
            assert nc == want[key]["ncycles"] and list(hist) == want[key]["du"], bcs


# ---------------------------------------------------------------------------
# the pipeline, quirk Q4 and the flux-balance fields at coordinates away from 0
# ---------------------------------------------------------------------------
def _vector_solve(x, y, z, b):
    """ndsm_vector_solve with the reference's default options; (ierr, A, B, ioptc as the call left it)"""
    import ndsm_amd
    L = ndsm_amd.load_library()
    ns = np.array(b.shape[::-1], dtype=np.intc)
    io = np.zeros(16, dtype=np.intc)
    ro = np.zeros(16)
    io[0], io[1], io[6], io[7] = 5, 1024, 1, 10000
    ro[0], ro[1] = 1e-10, 1e-13
    A, B = np.zeros(b.size), np.ascontiguousarray(b, dtype=np.float64).ravel().copy()
    f = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    q = [np.ascontiguousarray(v, dtype=np.float64) for v in (x, y, z)]
    rc = L.ndsm_vector_solve(ctypes.c_size_t(b.size), ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                             io.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), f(ro), f(q[0]), f(q[1]), f(q[2]), f(A), f(B))
    return rc, A.reshape(b.shape), B.reshape(b.shape), io


@pytest.mark.parametrize("name", ("analytic", "unbalanced"))
def test_pipeline_golden_and_oracle(hip, port, golden_dir, name):
    """the reference's pipeline output on the anisotropic box (tolerances of test_pipeline_golden), and the oracle's:
    the same return code and option slots"""
    import ndsm_amd
    g = np.load(os.path.join(golden_dir, f"pipeline_aniso_{name}.npz"))
    x, y, z, b = _case(name)
    ierr, A, B, io = _vector_solve(x, y, z, b)
    ierr2, A2, B2, io2, _ro = port.vector_potential(x, y, z, b)
    assert ierr == ierr2 == 0 and list(io[:8]) == list(io2[:8]) == list(g["ioptc"][:8])
    scale = np.abs(g["A"]).max()
    h = x[1] - x[0]
    for got_A, got_B in ((A, B), (A2, B2)):
        assert np.abs(got_A - g["A"]).max() <= 1e-12 * scale, np.abs(got_A - g["A"]).max()
        assert np.abs(got_B - g["B"]).max() <= 1e-12 * scale * 4 / h, np.abs(got_B - g["B"]).max()
    # the Python loader: same bits as the raw entry point
    i3, A3, B3 = ndsm_amd.vector_potential(x, y, z, b.copy())
    assert i3 == ierr and np.array_equal(A3, A) and np.array_equal(B3, B)


def test_device_face_phase_equals_host_face_phase(hip):
    """test_gpu_parity's host / device face-phase comparison where every face's spacings differ: the device phase
    (faces.hip) must take quirk Q4 exactly as the host phase (vecpot_faces) does - balanced and unbalanced data,
    both flux-balance orders, a non-zero initial guess, the device-resident entry; VecPot.solve is
    vector_potential, bit for bit"""
    import ndsm_amd
    x, y, z, b = _case("analytic")
    bn = _case("unbalanced")[3]
    a0 = 0.01 * np.random.default_rng(6).uniform(-1, 1, b.shape)
    V = ndsm_amd.VecPot(x, y, z)
    for field, guess, flx in ((b, None, False), (b, None, True), (bn, None, False), (bn, a0, True)):
        os.environ["NDSM_HIP_HOST_FACES"] = "1"
        try:
            i1, A1, B1 = V.solve(field, a_init=guess, flxcrl=flx)
        finally:
            os.environ.pop("NDSM_HIP_HOST_FACES", None)
        i2, A2, B2 = V.solve(field, a_init=guess, flxcrl=flx)
        i3, A3, B3 = V.solve(field, a_init=guess, flxcrl=flx, device=True)
        assert i1 == i2 == i3
        assert np.array_equal(A1, A2) and np.array_equal(B1, B2), (guess is not None, flx)
        assert np.array_equal(A2, A3) and np.array_equal(B2, B3), (guess is not None, flx)
    for field in (b, bn):
        s = V.solve(field)
        v = ndsm_amd.vector_potential(x, y, z, field.copy())
        assert s[0] == v[0] and np.array_equal(s[1], v[1]) and np.array_equal(s[2], v[2])
    V.close()


# ---------------------------------------------------------------------------
# the current-carrying field and the helicity reduction (Coulomb gauge; the DeVore gauge's reduction is
# test_gpu_devore.py::test_reduction_against_numpy[aniso-*])
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ns", ([33, 22, 27], WIDE), ids=_tag)
def test_field_problems_solved(hip, port, ns):
    """solve_field's 3-D problems laplace(A_c) = -(curl_h B)_c are solved: the oracle's residual against a numpy
    curl that takes each axis's own spacing"""
    import ndsm_amd
    mesh = aniso_mesh(ns)
    b = abc(mesh)
    V = ndsm_amd.VecPot(*mesh)
    ie, A, Br = V.solve_field(b, vc_tol=VC_TOL)
    V.close()
    assert ie == 0
    J = fld.curl(b, mesh)
    for c in range(3):
        r = port.residual3d(A[c], -J[c], mesh, BCS3[c])
        assert np.abs(r).max() <= 1e-9 * np.abs(J[c]).max(), (c, np.abs(r).max())


@pytest.mark.parametrize("field", ("abc", "flux"))
@pytest.mark.parametrize("ns", ([33, 22, 27], WIDE), ids=_tag)
def test_helicity_reduction_against_numpy(hip, ns, field):
    """test_gpu_field's reduction check (trapezoid weights, B_rec error, both divergences) with unequal weights and
    differences per axis, in the Coulomb gauge; the DeVore half of gauge="both" reduces the same B and B_p"""
    import ndsm_amd
    mesh = aniso_mesh(ns)
    b = {"abc": abc, "flux": flux}[field](mesh)
    V = ndsm_amd.VecPot(*mesh)
    hc, hd = V.helicity(b, vc_tol=VC_TOL, return_fields=True, gauge="both")
    ie, A, Br = V.solve_field(b, vc_tol=VC_TOL)
    V.close()
    assert hc.ierr == 0 and hd.ierr == 0 and ie == 0 and np.array_equal(hc.A, A)
    w = fld.weights(mesh)
    hmin = min(q[1] - q[0] for q in mesh)
    for h in (hc, hd):
        ref = fld._numpy_helicity(h.A, h.A_p, b, h.B_p, None, mesh)
        for k, (val, scale) in ref.items():
            assert abs(getattr(h, k) - val) <= 1e-12 * scale, (k, getattr(h, k), val)
        assert abs(h.divB_max - np.abs(fld.div(b, mesh)).max()) <= 1e-14 * np.abs(b).max() / hmin
        assert h.E_free == h.E - h.E_p
    emax, erms = fld.recon(Br, b, w)
    assert hc.recon_max == emax
    assert abs(hc.recon_rms - erms) <= 1e-12 * erms
    assert abs(hc.divA_max - np.abs(fld.div(hc.A, mesh)).max()) <= 1e-14 * np.abs(hc.A).max() / hmin
