"""GPU tests of the solenoidal projection (run with -m gpu on an MI355X): VecPot.project, solenoidal_projection
and project=True on the helicity entries, on

    B = ABC + eps grad(psi) + (a smooth non-solenoidal term),  psi = cos(pi x/Lx) cos(pi y/Ly) cos(pi z/Lz),

against a host reference made of numpy differences and the oracle's all-Neumann solve.  What is checked: the
3-D all-Neumann multigrid underneath against the oracle, the projected field, c, the divergences, phi and the
energy removed against that reference, the invariants (B.n on the faces bitwise, the potential field bitwise,
a discretely solenoidal field bitwise), second-order convergence to ABC, the net-flux part being reported and
not removed, and the entries and options."""
import ctypes

import numpy as np
import pytest

from golden_inputs import aniso_mesh, uniform_mesh

pytestmark = pytest.mark.gpu

VC_TOL = 1e-12
EPS = 0.3


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


def grad_psi(mesh):
    """grad of psi = cos(pi x/Lx) cos(pi y/Ly) cos(pi z/Lz): d psi / dn = 0 on every face"""
    X, Y, Z = grids(mesh)
    L = [q[-1] - q[0] for q in mesh]
    kx, ky, kz = (np.pi / l for l in L)
    cx, cy, cz = np.cos(kx * X), np.cos(ky * Y), np.cos(kz * Z)
    sx, sy, sz = np.sin(kx * X), np.sin(ky * Y), np.sin(kz * Z)
    return np.stack([-kx * sx * cy * cz, -ky * cx * sy * cz, -kz * cx * cy * sz])


def smooth_random(mesh, seed=5):
    """a few seeded low modes in every component: neither solenoidal nor a gradient"""
    X, Y, Z = grids(mesh)
    rng = np.random.default_rng(seed)
    out = np.zeros((3,) + X.shape)
    for c in range(3):
        for _ in range(3):
            a, kx, ky, kz, p = rng.uniform(-0.2, 0.2), *rng.integers(0, 3, 3), rng.uniform(0, np.pi)
            out[c] += a * np.cos(kx * np.pi * X + p) * np.cos(ky * np.pi * Y) * np.sin(kz * np.pi * Z + p)
    return out


def weights(mesh):
    ws = []
    for q in mesh:
        h = q[1] - q[0]
        w = np.full(len(q), h)
        w[0] = w[-1] = 0.5 * h
        ws.append(w)
    return ws[2][:, None, None] * ws[1][None, :, None] * ws[0][None, None, :]


def div(v, mesh):
    """div_h with derivq's stencil (centred inside, 3-point one-sided on the end planes)"""
    return sum(np.gradient(v[d], mesh[d][1] - mesh[d][0], axis=2 - d, edge_order=2) for d in range(3))


def grad_h(phi, mesh):
    """G_h: centred differences inside, 0 on the two end planes of each axis"""
    g = np.zeros((3,) + phi.shape)
    g[0][:, :, 1:-1] = (phi[:, :, 2:] - phi[:, :, :-2]) / (2 * (mesh[0][1] - mesh[0][0]))
    g[1][:, 1:-1, :] = (phi[:, 2:, :] - phi[:, :-2, :]) / (2 * (mesh[1][1] - mesh[1][0]))
    g[2][1:-1, :, :] = (phi[2:, :, :] - phi[:-2, :, :]) / (2 * (mesh[2][1] - mesh[2][0]))
    return g


def reference(port, b, mesh, **kw):
    """the projection on the host: numpy divergence, weighted mean removed, the oracle's all-Neumann solve"""
    d = div(b, mesh)
    w = weights(mesh)
    c = (w * d).sum() / w.sum()
    ierr, phi, du, hist, nc, sw = port.solve_bvp(np.zeros_like(d), d - c, mesh, "NNNNNN", vc_tol=VC_TOL, **kw)
    g = grad_h(phi, mesh)
    return dict(ierr=ierr, ncycles=nc, c=c, d=d, phi=phi, B=b - g, E=0.5 * (w * (g * g).sum(axis=0)).sum())


def case(ns, seed=5, meshf=uniform_mesh):
    mesh = meshf(ns)
    return mesh, abc(mesh) + EPS * grad_psi(mesh) + smooth_random(mesh, seed)


SHAPES = ([33, 33, 33], [65, 65, 65], [33, 22, 27])
IDS = lambda s: "x".join(map(str, s))   # noqa: E731


@pytest.mark.parametrize("ns", ([33, 33, 33], [33, 22, 27]), ids=IDS)
def test_all_neumann_3d_solver_matches_oracle(hip, port, ns):
    mesh = uniform_mesh(ns)
    rng = np.random.default_rng(31)
    rhs = rng.uniform(-1, 1, tuple(ns[::-1]))
    w = weights(mesh)
    rhs = rhs - (w * rhs).sum() / w.sum()
    ierr2, u2, du2, h2, nc2, sw = port.solve_bvp(np.zeros_like(rhs), rhs, mesh, "NNNNNN", vc_tol=VC_TOL, hist_len=64)
    S = hip.MGSolver(ns, mesh, "NNNNNN")
    S.upload(1, hip.BUF_U, np.zeros_like(rhs))
    S.upload(1, hip.BUF_RHS, rhs)
    ierr, du, nc, h = S.solve(vc_tol=VC_TOL, nmax=1024)
    got = S.download(1, hip.BUF_U)
    S.close()
    assert ierr == ierr2 == 0 and nc == nc2, (nc, nc2)
    assert np.abs(got - u2).max() <= 1e-13 * np.abs(u2).max(), np.abs(got - u2).max()


def _meshes(uniform, aniso):
    """the shapes on uniform_mesh under the ids they always had, and on golden_inputs.aniso_mesh (a spacing of its own
    on every axis, no origin at 0) under 'aniso-' ids; [300, 40, 60]: rows longer than a block, more rows than blocks"""
    return ([pytest.param(ns, uniform_mesh, id=IDS(ns)) for ns in uniform] +
            [pytest.param(ns, aniso_mesh, id="aniso-" + IDS(ns)) for ns in aniso])


@pytest.mark.parametrize("ns,meshf", _meshes(SHAPES, ([33, 22, 27], [300, 40, 60])))
def test_against_numpy_and_oracle(hip, port, ns, meshf):
    import ndsm_amd
    mesh, b = case(ns, meshf=meshf)
    V = ndsm_amd.VecPot(*mesh)
    p = V.project(b, vc_tol=VC_TOL, return_phi=True)
    V.close()
    ref = reference(port, b, mesh)
    assert p.ierr == 0 and ref["ierr"] == 0
    h = min(q[1] - q[0] for q in mesh)
    scale = np.abs(b).max()
    assert np.abs(p.B - ref["B"]).max() <= 1e-12 * scale, np.abs(p.B - ref["B"]).max()
    assert abs(p.c - ref["c"]) <= 1e-14 * scale / h, (p.c, ref["c"])
    assert abs(p.divB_before - np.abs(ref["d"]).max()) <= 1e-14 * scale / h
    assert abs(p.divB_after - np.abs(div(p.B, mesh)).max()) <= 1e-14 * scale / h
    w = weights(mesh)
    g = grad_h(p.phi, mesh)
    assert abs(p.E_removed - 0.5 * (w * (g * g).sum(axis=0)).sum()) <= 1e-12 * p.E_removed
    assert abs(p.E_removed - ref["E"]) <= 1e-10 * ref["E"]
    assert np.abs(p.phi - ref["phi"]).max() <= 1e-12 * max(1.0, np.abs(ref["phi"]).max())
    assert p.ncycles == ref["ncycles"] and p.du_last < VC_TOL
    assert p.divB_after < 0.2 * p.divB_before


@pytest.mark.parametrize("ns,meshf", _meshes(([33, 33, 33], [33, 22, 27]), ([33, 22, 27],)))
def test_invariants(hip, ns, meshf):
    import ndsm_amd
    mesh, b = case(ns, meshf=meshf)
    V = ndsm_amd.VecPot(*mesh)
    p = V.project(b, vc_tol=VC_TOL)
    for d in range(3):                   # B.n on each of the six faces: bitwise unchanged
        for end in (0, -1):
            sl = [slice(None)] * 3
            sl[2 - d] = end
            assert np.array_equal(p.B[d][tuple(sl)], b[d][tuple(sl)]), (d, end)
    assert not np.array_equal(p.B, b)
    s0 = V.solve(b, vc_tol=VC_TOL)
    s1 = V.solve(p.B, vc_tol=VC_TOL)
    assert s0[0] == s1[0] and np.array_equal(s0[1], s1[1]) and np.array_equal(s0[2], s1[2])
    # a discretely solenoidal field passes through bitwise
    a = abc(mesh)
    q = V.project(a, vc_tol=VC_TOL, return_phi=True)
    V.close()
    assert q.ierr == 0 and np.array_equal(q.B, a) and not np.any(q.phi)
    assert q.c == 0.0 and q.divB_before == 0.0 and q.divB_after == 0.0 and q.E_removed == 0.0


def test_convergence_to_abc(hip):
    """B = ABC + eps grad(psi): B' -> ABC and div_h B' / div_h B -> 0 at second order.  H_R of the projected field
    is that of ABC to rounding at every size (a gradient with d psi / dn = 0 carries no relative helicity, and the
    projected field differs from ABC by one), while the projection cuts the reconstruction error 10x."""
    import ndsm_amd
    errs, ratios, dh, hr = [], [], [], []
    for n in (33, 65, 129):
        mesh = uniform_mesh([n, n, n])
        a = abc(mesh)
        b = a + EPS * grad_psi(mesh)
        V = ndsm_amd.VecPot(*mesh)
        p = V.project(b, vc_tol=VC_TOL)
        h0 = V.helicity(a, vc_tol=VC_TOL)
        h1 = V.helicity(b, vc_tol=VC_TOL, project=True)
        V.close()
        assert p.ierr == 0 and h1.ierr == 0 and h0.ierr == 0
        e = p.B - a
        errs.append((np.abs(e).max(), np.sqrt((weights(mesh) * (e * e).sum(axis=0)).sum())))
        ratios.append(p.divB_after / p.divB_before)
        dh.append(abs(h1.H_R - h0.H_R))
        hr.append(abs(h0.H_R))
        if n == 65:
            assert ratios[-1] <= 1e-2, ratios
            h2 = ndsm_amd.relative_helicity(*mesh, b, vc_tol=VC_TOL)
            assert h1.recon_rms * 10 <= h2.recon_rms, (h1.recon_rms, h2.recon_rms)
    for (m0, r0), (m1, r1) in zip(errs, errs[1:]):
        assert m0 / m1 >= 3 and r0 / r1 >= 3, errs
    for r0, r1 in zip(ratios, ratios[1:]):
        assert r0 / r1 >= 3, ratios
    assert all(d <= 1e-12 * h for d, h in zip(dh, hr)), (dh, hr)


def test_net_flux_is_reported_not_removed(hip):
    import ndsm_amd
    mesh = uniform_mesh([33, 33, 33])
    X = grids(mesh)[0]
    a = 0.7
    b = abc(mesh)
    b[0] = b[0] + a * X
    p = ndsm_amd.solenoidal_projection(*mesh, b, vc_tol=VC_TOL)
    assert p.ierr == 0
    assert abs(p.c - a) <= 1e-12, p.c
    assert np.abs(p.B - b).max() <= 1e-12, np.abs(p.B - b).max()
    assert abs(p.divB_after - a) <= 1e-12 and abs(p.divB_before - a) <= 1e-12


def test_entries_and_determinism(hip):
    import ndsm_amd
    mesh, b = case([33, 22, 27])
    V = ndsm_amd.VecPot(*mesh)
    p1 = V.project(b, vc_tol=VC_TOL, return_phi=True)
    p2 = V.project(b, vc_tol=VC_TOL, return_phi=True)
    p3 = V.project(b, vc_tol=VC_TOL, return_phi=True, device=True)
    p4 = V.project(b, vc_tol=VC_TOL, device=True)
    V.close()
    for q in (p2, p3, p4):
        assert q[3:] == p1[3:] and q.ierr == p1.ierr == 0
        assert np.array_equal(q.B, p1.B)
    for q in (p2, p3):
        assert np.array_equal(q.phi, p1.phi)
    assert p4.phi is None
    # the one-shot form: the same bits
    p5 = ndsm_amd.solenoidal_projection(*mesh, b, vc_tol=VC_TOL, return_phi=True)
    assert p5[3:] == p1[3:] and np.array_equal(p5.B, p1.B) and np.array_equal(p5.phi, p1.phi)


def test_project_leaves_later_calls_on_the_handle_alone(hip):
    import ndsm_amd
    mesh, b = case([33, 33, 33])
    F = ndsm_amd.VecPot(*mesh)
    want = (F.solve(b, vc_tol=VC_TOL), F.solve_field(b, vc_tol=VC_TOL), F.helicity(b, vc_tol=VC_TOL))
    F.close()
    V = ndsm_amd.VecPot(*mesh)
    V.project(b, vc_tol=VC_TOL)
    got = (V.solve(b, vc_tol=VC_TOL), V.solve_field(b, vc_tol=VC_TOL), V.helicity(b, vc_tol=VC_TOL))
    h_plain = V.helicity(b, vc_tol=VC_TOL)
    hp = V.helicity(b, vc_tol=VC_TOL, project=True)
    V.close()
    for w, g in zip(want[:2], got[:2]):
        assert w[0] == g[0] and np.array_equal(w[1], g[1]) and np.array_equal(w[2], g[2])
    assert want[2][:10] == got[2][:10] == h_plain[:10]
    # project=True is the helicity of the projected field, and keeps the projection
    assert V.last_projection is not None and hp.ierr == 0
    h = mesh[0][1] - mesh[0][0]
    assert abs(hp.divB_max - V.last_projection.divB_after) <= 1e-14 * np.abs(b).max() / h
    W = ndsm_amd.VecPot(*mesh)
    assert W.helicity(V.last_projection.B, vc_tol=VC_TOL)[:10] == hp[:10]
    W.close()


def test_options(hip):
    import ndsm_amd
    L = ndsm_amd.load_library()
    mesh, b = case([33, 33, 33])
    V = ndsm_amd.VecPot(*mesh)
    base = V.project(b, vc_tol=VC_TOL)
    one = V.project(b, vc_tol=VC_TOL, ncycles_max=1)
    assert one.ierr == 1 and one.ncycles == 1 and V.last_ioptc[3] == 1
    mp = V.project(b, vc_tol=VC_TOL, mixed_precision=True)
    assert mp[3:] == base[3:] and np.array_equal(mp.B, base.B)
    mn = V.project(b, vc_tol=VC_TOL, mean=True)
    assert mn.ierr == 0 and np.abs(mn.B - base.B).max() <= 1e-9 * np.abs(b).max()
    hp = V.helicity(b, vc_tol=VC_TOL, ncycles_max=1, project=True)
    assert hp.ierr == 1
    again = V.project(b, vc_tol=VC_TOL)                  # the handle is fine afterwards
    assert again[3:] == base[3:] and np.array_equal(again.B, base.B)
    # an ngrids slot other than the handle's: 9002, B untouched
    ioptc, ropt = V._options(10000, 1024, 1e-13, VC_TOL, 5, False, 0, False)
    ioptc[L.get_iopt_ngrids()] = 3
    B = np.ascontiguousarray(b, dtype=np.float64).reshape(-1).copy()
    out = np.full(4, np.nan)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = L.ndsm_hip_vecpot_project(V.h, ioptc.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ropt.ctypes.data_as(dp),
                                   B.ctypes.data_as(dp), None, out.ctypes.data_as(dp))
    V.close()
    assert rc == 9002 and np.array_equal(B, b.reshape(-1)) and np.all(out == 0.0)
    # a level cap on the handle goes through
    V = ndsm_amd.VecPot(*mesh, ngrids=3)
    p3 = V.project(b, vc_tol=VC_TOL)
    V.close()
    assert p3.ierr == 0 and np.abs(p3.B - base.B).max() <= 1e-9 * np.abs(b).max()


def test_too_large_is_refused(hip):
    """2048^3: the hierarchy and the caller's arrays cannot fit in HBM; refused before any allocation or
    launch - the tiny device buffers below are never touched"""
    import ndsm_amd
    L = ndsm_amd.load_library()
    x = np.linspace(0, 1, 2048)
    V = ndsm_amd.VecPot(x, x, x)
    bufs = []
    for _ in range(2):
        p = ctypes.c_void_p()
        assert L.ndsm_hip_device_alloc(64, ctypes.byref(p)) == 0
        bufs.append(p)
    ioptc, ropt = V._options(10000, 1024, 1e-13, VC_TOL, 5, False, 0, False)
    out = np.full(4, np.nan)
    dp = ctypes.POINTER(ctypes.c_double)
    try:
        rc = L.ndsm_hip_vecpot_project_device(V.h, ioptc.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                              ropt.ctypes.data_as(dp), *bufs, out.ctypes.data_as(dp))
        assert rc == 9001 and np.all(out == 0.0), rc
    finally:
        for p in bufs:
            L.ndsm_hip_device_free(p)
        V.close()
    mesh, b = case([33, 33, 33])
    assert ndsm_amd.solenoidal_projection(*mesh, b, vc_tol=VC_TOL).ierr == 0
