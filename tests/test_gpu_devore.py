"""GPU tests of the DeVore-gauge vector potentials (run with -m gpu on an MI355X): VecPot.devore, devore_potentials
and gauge= on the helicity entries, on the ABC field of test_gpu_field.py

    B = (sin kz + cos ky, sin kx + cos kz, sin ky + cos kx),  k = pi,

and on ABC plus a current-free part with net flux through each pair of faces.  What is checked: A and A_p against
a numpy restatement of the recurrences (bitwise), the reduction against numpy, the potential field untouched,
gauge invariance of H_R and H_J against the Coulomb gauge and second-order reconstruction of B and B_p,
determinism, host against device, gauge="both", project=True, and the arguments."""
import ctypes

import numpy as np
import pytest

from golden_inputs import aniso_mesh, uniform_mesh

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


def grids(mesh):
    return np.meshgrid(mesh[2], mesh[1], mesh[0], indexing="ij")[::-1]   # X, Y, Z, each (nz, ny, nx)


def abc(mesh):
    X, Y, Z = grids(mesh)
    k = np.pi
    return np.stack([np.sin(k * Z) + np.cos(k * Y), np.sin(k * X) + np.cos(k * Z), np.sin(k * Y) + np.cos(k * X)])


def flux(mesh):
    """ABC + grad(x^2/2 - z^2/2 + xyz/2) + a uniform field: still solenoidal (each added component is linear in
    its own coordinate or independent of it, so div_h is 0 to rounding), with net flux through every face pair"""
    X, Y, Z = grids(mesh)
    return abc(mesh) + np.stack([0.4 * X + 0.5 * Y * Z + 0.2, 0.5 * X * Z - 0.1, -0.4 * Z + 0.5 * X * Y + 0.3])


def grad_psi(mesh):
    """grad of psi = cos(pi x/Lx) cos(pi y/Ly) cos(pi z/Lz): a divergent addition with d psi / dn = 0"""
    X, Y, Z = grids(mesh)
    L = [q[-1] - q[0] for q in mesh]
    kx, ky, kz = (np.pi / l for l in L)
    cx, cy, cz = np.cos(kx * X), np.cos(ky * Y), np.cos(kz * Z)
    sx, sy, sz = np.sin(kx * X), np.sin(ky * Y), np.sin(kz * Z)
    return np.stack([-kx * sx * cy * cz, -ky * cx * sy * cz, -kz * cx * cy * sz])


FIELDS = {"abc": abc, "flux": flux}


def weights(mesh):
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


def rms(e, mesh):
    w = weights(mesh)
    return np.sqrt((w * (e * e).sum(axis=0)).sum() / w.sum())


def devore_numpy(b, bp, mesh):
    """the recurrences of include/ndsm_hip.h, one plane (or line) at a time, in the same operand order"""
    hx, hy, hz = (q[1] - q[0] for q in mesh)
    qx, qy, h2 = 0.25 * hx, 0.25 * hy, 0.5 * hz
    nz = b.shape[1]
    A, Ap = np.zeros_like(b), np.zeros_like(b)
    bz = b[2, 0]                                            # (ny, nx)
    for j in range(1, bz.shape[0]):
        A[0, 0, j] = A[0, 0, j - 1] - (bz[j - 1] + bz[j]) * qy
    for i in range(1, bz.shape[1]):
        A[1, 0, :, i] = A[1, 0, :, i - 1] + (bz[:, i - 1] + bz[:, i]) * qx
    for k in range(1, nz):
        A[0, k] = A[0, k - 1] + (b[1, k - 1] + b[1, k]) * h2
        A[1, k] = A[1, k - 1] - (b[0, k - 1] + b[0, k]) * h2
    Ap[:, nz - 1] = A[:, nz - 1]
    for k in range(nz - 2, -1, -1):
        Ap[0, k] = Ap[0, k + 1] - (bp[1, k] + bp[1, k + 1]) * h2
        Ap[1, k] = Ap[1, k + 1] + (bp[0, k] + bp[0, k + 1]) * h2
    return A, Ap


IDS = lambda s: "x".join(map(str, s))   # noqa: E731
_RUNS = {}


def both_run(hip, field, n):
    """(mesh, b, coulomb, devore) of helicity(gauge="both", return_fields=True) at n^3, cached for the module"""
    key = (field, n)
    if key not in _RUNS:
        import ndsm_amd
        mesh = uniform_mesh([n, n, n])
        b = FIELDS[field](mesh)
        V = ndsm_amd.VecPot(*mesh)
        hc, hd = V.helicity(b, vc_tol=VC_TOL, return_fields=True, gauge="both")
        V.close()
        assert hc.ierr == 0 and hd.ierr == 0
        _RUNS[key] = (mesh, b, hc, hd)
    return _RUNS[key]


@pytest.mark.parametrize("field", sorted(FIELDS))
@pytest.mark.parametrize("ns", ([33, 33, 33], [33, 22, 27]), ids=IDS)
def test_potentials_bitwise_against_numpy(hip, field, ns):
    import ndsm_amd
    mesh = uniform_mesh(ns)
    b = FIELDS[field](mesh)
    V = ndsm_amd.VecPot(*mesh)
    h = V.helicity(b, vc_tol=VC_TOL, return_fields=True, gauge="devore")
    d = V.devore(b, h.B_p)
    V.close()
    assert h.ierr == 0 and d.ierr == 0
    A, Ap = devore_numpy(b, h.B_p, mesh)
    for got in (h, d):
        assert np.array_equal(got.A, A) and np.array_equal(got.A_p, Ap)
        assert not np.any(got.A[2]) and not np.any(got.A_p[2])          # A_z = A_p,z = 0 exactly
        assert np.array_equal(got.A_p[:, -1], got.A[:, -1])            # the top plane is a copy
    assert np.array_equal(d.B_p, h.B_p) and d[1:10] == h[1:10]


def test_potentials_bitwise_with_unequal_spacings(hip):
    """h_x, h_y, h_z all different and a mesh that does not start at 0: each factor goes where it belongs.  B_p
    is the caller's own here (any field with b's B.n; this one has other values inside)"""
    import ndsm_amd
    mesh = [np.linspace(0.0, 1.0, 33), np.linspace(-0.3, 0.5, 22), np.linspace(0.1, 1.3, 27)]
    b = flux(mesh)
    bp = b.copy()
    bp[:, 1:-1, 1:-1, 1:-1] *= 0.5
    d = ndsm_amd.devore_potentials(*mesh, b, bp)
    A, Ap = devore_numpy(b, bp, mesh)
    assert np.array_equal(d.A, A) and np.array_equal(d.A_p, Ap) and np.array_equal(d.B_p, bp)
    V = ndsm_amd.VecPot(*mesh)
    e = V.devore(b, bp, device=True)
    V.close()
    assert e[:10] == d[:10] and np.array_equal(e.A, A) and np.array_equal(e.A_p, Ap)


@pytest.mark.parametrize("field", sorted(FIELDS))
@pytest.mark.parametrize("ns,meshf", [pytest.param(ns, uniform_mesh, id=IDS(ns)) for ns in ([33, 33, 33], [33, 22, 27])] +
                         [pytest.param(ns, aniso_mesh, id="aniso-" + IDS(ns)) for ns in ([33, 22, 27], [300, 40, 60])])
def test_reduction_against_numpy(hip, field, ns, meshf):
    import ndsm_amd
    mesh = meshf(ns)
    b = FIELDS[field](mesh)
    V = ndsm_amd.VecPot(*mesh)
    h = V.helicity(b, vc_tol=VC_TOL, return_fields=True, gauge="devore")
    V.close()
    assert_reduction(h, b, mesh)


def assert_reduction(h, b, mesh):
    """the scalars of a DeVore-gauge Helicity h of b (with its A, A_p, B_p) against numpy on the returned arrays"""
    w = weights(mesh)
    db = b - h.B_p
    terms = {"H_R": w * ((h.A + h.A_p) * db).sum(axis=0), "H_J": w * ((h.A - h.A_p) * db).sum(axis=0),
             "E": 0.5 * w * (b * b).sum(axis=0), "E_p": 0.5 * w * (h.B_p * h.B_p).sum(axis=0)}
    for k, v in terms.items():
        assert abs(getattr(h, k) - v.sum()) <= 1e-13 * np.abs(v).sum(), (k, getattr(h, k), v.sum())
    assert h.E_free == h.E - h.E_p
    hmin = min(q[1] - q[0] for q in mesh)
    tol = 1e-13 * np.abs(h.A).max() / hmin                  # rounding of a difference quotient of A
    e = curl(h.A, mesh) - b
    assert abs(h.recon_max - np.abs(e).max()) <= tol, (h.recon_max, np.abs(e).max())
    assert abs(h.recon_rms - rms(e, mesh)) <= tol, (h.recon_rms, rms(e, mesh))
    assert abs(h.divB_max - np.abs(div(b, mesh)).max()) <= 1e-13 * np.abs(b).max() / hmin
    assert abs(h.divA_max - np.abs(div(h.A, mesh)).max()) <= tol
    assert h.divA_max > 0.1                                 # the DeVore gauge is not divergence-free


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_potential_field_unchanged(hip, field):
    import ndsm_amd
    mesh = uniform_mesh([33, 22, 27])
    b = FIELDS[field](mesh)
    V = ndsm_amd.VecPot(*mesh)
    s = V.solve(b, vc_tol=VC_TOL)
    hd = V.helicity(b, vc_tol=VC_TOL, return_fields=True, gauge="devore")
    hc = V.helicity(b, vc_tol=VC_TOL, return_fields=True)
    s2 = V.solve(b, vc_tol=VC_TOL)
    V.close()
    assert np.array_equal(hd.B_p, s[2]) and np.array_equal(hc.B_p, s[2])
    assert s2[0] == s[0] and np.array_equal(s2[1], s[1]) and np.array_equal(s2[2], s[2])


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_gauge_invariance_and_reconstruction(hip, field):
    """H_R and H_J of the two gauges agree to O(h^2); curl_h A - B is O(h^2).  curl_h A_p - B_p: the x and y
    components are O(h^2).  The z-component is B_p,z(top) reconstructed minus the trapezoid sum of d_z B_p,z, which
    telescopes to B_p,z only up to (h^2/4) d_zz B_p,z - and the library's discrete potential field has O(h) second
    z-differences in a layer of a few planes at the two z faces, so that component converges as h^1.5 in the rms
    (x 2.8 per halving)"""
    rel_r, rel_j, rec, rec_p, rec_pxy = [], [], [], [], []
    for n in (33, 65, 129):
        mesh, b, hc, hd = both_run(hip, field, n)
        rel_r.append(abs(hd.H_R - hc.H_R) / abs(hc.H_R))
        rel_j.append(abs(hd.H_J - hc.H_J) / abs(hc.H_J))
        rec.append(hd.recon_rms)
        e = curl(hd.A_p, mesh) - hd.B_p
        rec_p.append(rms(e, mesh))
        rec_pxy.append(rms(np.stack([e[0], e[1], 0 * e[2]]), mesh))
        h = mesh[0][1] - mesh[0][0]
        assert abs(hd.recon_rms - rms(curl(hd.A, mesh) - b, mesh)) <= 1e-13 * np.abs(hd.A).max() / h
    print(field, "dH_R/H_R", rel_r, "dH_J/H_J", rel_j, "recon_rms", rec, "A_p:", rec_p, "A_p x,y:", rec_pxy)
    for series in (rel_r, rel_j, rec, rec_pxy):
        for e0, e1 in zip(series, series[1:]):
            assert e0 / e1 >= 3.0, series
    for e0, e1 in zip(rec_p, rec_p[1:]):
        assert e0 / e1 >= 2.5, rec_p


def test_divergent_input_shows_in_the_reconstruction(hip):
    """B + 0.3 grad(psi): the z-component of the DeVore B_rec misses int_z0^z div_h B dz' (to O(h^2)), a
    reconstruction error that is 0 on the base plane and grows with height; project=True removes most of it"""
    import ndsm_amd
    mesh = uniform_mesh([33, 33, 33])
    b = abc(mesh) + 0.3 * grad_psi(mesh)
    V = ndsm_amd.VecPot(*mesh)
    raw = V.helicity(b, vc_tol=VC_TOL, return_fields=True, gauge="devore")
    clean = V.helicity(b, vc_tol=VC_TOL, gauge="devore", project=True)
    V.close()
    ez = curl(raw.A, mesh)[2] - b[2]
    d = div(b, mesh)
    cum = np.zeros_like(d)
    for k in range(1, d.shape[0]):
        cum[k] = cum[k - 1] + (d[k - 1] + d[k]) * (0.5 * (mesh[2][1] - mesh[2][0]))
    assert np.abs(ez + cum).max() <= 0.02 * np.abs(cum).max(), (np.abs(ez + cum).max(), np.abs(cum).max())
    assert np.abs(ez[0]).max() <= 0.02 * np.abs(ez).max()
    assert clean.recon_rms * 5 <= raw.recon_rms, (clean.recon_rms, raw.recon_rms)


def test_determinism_host_device_and_both(hip):
    import ndsm_amd
    mesh = uniform_mesh([33, 22, 27])
    b = flux(mesh)
    V = ndsm_amd.VecPot(*mesh)
    h1 = V.helicity(b, vc_tol=VC_TOL, return_fields=True, gauge="devore")
    h2 = V.helicity(b, vc_tol=VC_TOL, return_fields=True, gauge="devore")
    hc = V.helicity(b, vc_tol=VC_TOL, return_fields=True)
    pair = V.helicity(b, vc_tol=VC_TOL, return_fields=True, gauge="both")
    nofields = V.helicity(b, vc_tol=VC_TOL, gauge="devore")
    d_host = V.devore(b, h1.B_p)
    d_host2 = V.devore(b, h1.B_p)
    d_dev = V.devore(b, h1.B_p, device=True)
    V.close()
    d_one = ndsm_amd.devore_potentials(*mesh, b, h1.B_p)
    assert h1.ierr == 0 and hc.ierr == 0

    def same(x, y):
        return x[:10] == y[:10] and all(np.array_equal(p, q) for p, q in zip(x[10:], y[10:]))
    assert same(h1, h2) and same(pair[1], h1) and same(pair[0], hc)
    assert nofields[:10] == h1[:10] and nofields.A is None and nofields.B_p is None
    for d in (d_host, d_host2, d_dev, d_one):
        assert d[1:10] == h1[1:10] and np.array_equal(d.A, h1.A) and np.array_equal(d.A_p, h1.A_p)
        assert np.array_equal(d.B_p, h1.B_p) and d.ierr == 0
    # the one-shot form with the gauge forwarded
    r = ndsm_amd.relative_helicity(*mesh, b, vc_tol=VC_TOL, gauge="both")
    assert r[0][:10] == hc[:10] and r[1][:10] == h1[:10]


def test_project_composes_and_arguments(hip):
    import ndsm_amd
    mesh = uniform_mesh([33, 22, 27])
    b = abc(mesh) + 0.3 * grad_psi(mesh)
    V = ndsm_amd.VecPot(*mesh)
    h = V.helicity(b, vc_tol=VC_TOL, return_fields=True, gauge="devore", project=True)
    pr = V.last_projection
    d = V.devore(pr.B, h.B_p)
    s = V.solve(pr.B, vc_tol=VC_TOL)
    hb = V.helicity(b, vc_tol=VC_TOL, gauge="both", project=True)
    hc = V.helicity(b, vc_tol=VC_TOL, project=True)
    assert h.ierr == 0 and pr.ierr == 0
    assert h[1:10] == d[1:10] and np.array_equal(h.A, d.A) and np.array_equal(h.A_p, d.A_p)
    assert np.array_equal(h.B_p, s[2])
    assert hb[0][:10] == hc[:10] and hb[1][:10] == h[:10]
    # wrong shapes: argument errors; an unknown gauge: ValueError; the handle is fine afterwards
    for args in ((b[:2], h.B_p), (b, h.B_p[:, :, :, :-1]), (b[:, :-1], h.B_p)):
        with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
            V.devore(*args)
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        V.helicity(b[:, :, :, :-1], gauge="devore")
    with pytest.raises(ndsm_amd.NdsmHipError, match="9002"):
        ndsm_amd.devore_potentials(mesh[0], mesh[1], mesh[2][:-1], b, b)
    with pytest.raises(ValueError):
        V.helicity(b, gauge="temporal")
    with pytest.raises(ValueError):
        ndsm_amd.relative_helicity(*mesh, b, gauge="DeVore")
    again = V.devore(pr.B, h.B_p)
    assert again[:10] == d[:10]
    # NULL arrays through the C entries: 9002, out cleared
    L = ndsm_amd.load_library()
    dp = ctypes.POINTER(ctypes.c_double)
    out = np.full(8, np.nan)
    B = np.ascontiguousarray(b, dtype=np.float64)
    rc = L.ndsm_hip_vecpot_devore(V.h, B.ctypes.data_as(dp), None, B.ctypes.data_as(dp), B.ctypes.data_as(dp),
                                  out.ctypes.data_as(dp))
    V.close()
    assert rc == 9002 and np.all(out == 0.0)


def test_too_large_is_refused(hip):
    """2048^3: five fields of 24 B/pt cannot fit in HBM; refused before any allocation or launch - the tiny
    device buffers below are never touched"""
    import ndsm_amd
    L = ndsm_amd.load_library()
    x = np.linspace(0, 1, 2048)
    V = ndsm_amd.VecPot(x, x, x)
    bufs = []
    for _ in range(4):
        p = ctypes.c_void_p()
        assert L.ndsm_hip_device_alloc(64, ctypes.byref(p)) == 0
        bufs.append(p)
    out = np.full(8, np.nan)
    dp = ctypes.POINTER(ctypes.c_double)
    try:
        rc = L.ndsm_hip_vecpot_devore_device(V.h, *bufs, out.ctypes.data_as(dp))
        assert rc == 9001 and np.all(out == 0.0), rc
    finally:
        for p in bufs:
            L.ndsm_hip_device_free(p)
        V.close()
    mesh = uniform_mesh([17, 17, 17])
    b = abc(mesh)
    assert ndsm_amd.relative_helicity(*mesh, b, vc_tol=VC_TOL, gauge="devore").ierr == 0
