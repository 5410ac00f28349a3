"""CPU tests: pin the C restatement (oracle/ndsm_oracle.c) to the reference.

(a) committed golden vectors produced by the reference itself
    (tests/golden/make_golden.py), (b) the reference's own known-answer rows
    tests/integration_test/results_test1.txt:6-7, (c) the reference's outputs on
    fresh random inputs and on a quirk case, recorded by make_golden.py.

Tolerance: the 3-D path has no order-dependent reduction, and the restatement
keeps the reference's operand order, so 3-D results are required to be
BIT-IDENTICAL.  The 2-D all-Neumann path subtracts a mean whose summation
order is unspecified in the reference (OpenMP reduction,
ndsm_multigrid_core.f90:1214): 1e-14 absolute there.
"""
import json
import os

import numpy as np
import pytest

from golden_inputs import (ANISO_SHAPE_2D, ANISO_SHAPES_3D, BCS3, BCS_ANISO, BCS_RANDOM, HUGE, KERNEL_SHAPES_2D,
                           KERNEL_SHAPES_3D, OPTION_PIPELINE_SHAPE, analytic_case, aniso_case, aniso_mesh,
                           aniso_pipeline_cases, digest, digest16, manufactured_poisson, negative_option_cases,
                           noisy_case, option_matrix, pipeline_option_cases, quirk_case, rand_field,
                           random_reference_cases, scalar_kw, scalar_option_problems, uniform_mesh, zero_field_cases)


def _tag(ns):
    return "x".join(str(n) for n in ns)


@pytest.mark.parametrize("ns", KERNEL_SHAPES_3D, ids=_tag)
def test_kernels3d_golden(port, golden_dir, ns):
    g = np.load(os.path.join(golden_dir, f"kernels3d_{_tag(ns)}.npz"))
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    shapes, meshes = port.hierarchy(ns, mesh)
    assert np.array_equal(shapes, g["level_shapes"])
    for l, lv in enumerate(meshes):
        for d, m in enumerate(lv):
            assert np.array_equal(m, g[f"mesh_l{l+1}_d{d+1}"])
    for bcs in BCS3:
        assert np.array_equal(port.relax3d(u, rhs, mesh, bcs), g[f"relax_{bcs}"])
        assert np.array_equal(port.residual3d(u, rhs, mesh, bcs), g[f"residual_{bcs}"])
        assert np.array_equal(port.vcycle(u, rhs, mesh, bcs), g[f"vcycle_{bcs}"])
    for lvl in range(1, len(shapes)):
        f = rand_field(tuple(int(v) for v in shapes[lvl - 1][::-1]), 3000 + lvl)
        c = rand_field(tuple(int(v) for v in shapes[lvl][::-1]), 4000 + lvl)
        assert np.array_equal(port.restrict(f, ns, mesh, lvl), g[f"restrict_l{lvl}"])
        assert np.array_equal(port.interp(c, ns, mesh, lvl), g[f"interp_l{lvl}"])
    un = u.copy()
    assert np.array_equal(np.array(port.update_u(rhs, un)), g["update_u"])
    assert np.array_equal(un, rhs)


@pytest.mark.parametrize("ns", KERNEL_SHAPES_2D, ids=_tag)
def test_kernels2d_golden(port, golden_dir, ns):
    g = np.load(os.path.join(golden_dir, f"kernels2d_{_tag(ns)}.npz"))
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    rhs0 = rhs - rhs.mean()
    shapes, _ = port.hierarchy(ns, mesh)
    assert np.array_equal(shapes, g["level_shapes"])
    for bcs in ("NNNN", "DNND"):
        np.testing.assert_allclose(port.relax_nd(u, rhs, mesh, bcs), g[f"relax_{bcs}"], rtol=0, atol=1e-14)
        assert np.array_equal(port.residual_nd(u, rhs, mesh, bcs), g[f"residual_{bcs}"])
    np.testing.assert_allclose(port.vcycle(u, rhs0, mesh, "NNNN"), g["vcycle_NNNN"], rtol=0, atol=1e-14)
    ierr, us, du, hist, nc, sw = port.solve_bvp(np.zeros(shp), rhs0, mesh, "NNNN", hist_len=64)
    assert ierr == int(g["solve_NNNN_meta"][0])
    np.testing.assert_allclose(us, g["solve_NNNN"], rtol=0, atol=1e-13)
    for lvl in range(1, len(shapes)):
        f = rand_field(tuple(int(v) for v in shapes[lvl - 1][::-1]), 3000 + lvl)
        c = rand_field(tuple(int(v) for v in shapes[lvl][::-1]), 4000 + lvl)
        assert np.array_equal(port.restrict(f, ns, mesh, lvl), g[f"restrict_l{lvl}"])
        assert np.array_equal(port.interp(c, ns, mesh, lvl), g[f"interp_l{lvl}"])


@pytest.mark.parametrize("ns", ([22, 22, 22], [33, 22, 27], [64, 64, 64]), ids=_tag)
@pytest.mark.parametrize("bcs", BCS3)
def test_solve3d_history_golden(port, golden_dir, ns, bcs):
    hist_all = json.load(open(os.path.join(golden_dir, "solve3d_history.json")))
    h = hist_all[f"{_tag(ns)}_{bcs}"]
    mesh = uniform_mesh(ns)
    us, rhs = manufactured_poisson(mesh, bcs)
    ierr, u, du, hist, nc, sw = port.solve_bvp(np.zeros_like(us), rhs, mesh, bcs, hist_len=64)
    assert ierr == 0 and nc == h["ncycles"]
    assert list(hist) == h["du"]          # bit-identical residual history
    assert du == h["du"][-1]
    if ns[0] <= 33:
        assert np.array_equal(u, np.load(os.path.join(golden_dir, f"solve3d_{_tag(ns)}_{bcs}.npy")))
    else:
        p = np.load(os.path.join(golden_dir, f"solve3d_{_tag(ns)}_{bcs}_planes.npz"))
        assert np.array_equal(u[ns[2] // 2], p["kz"])
        assert np.array_equal(u[:, ns[1] // 2], p["jy"])
        assert np.array_equal(u[:, :, ns[0] // 2], p["ix"])
    # second-order truncation error of the discretisation, not of the solver
    assert abs(np.abs(u - us).max() - h["err_vs_exact"]) < 1e-15


# tests/integration_test/results_test1.txt:6-7 (dx, Ea_max, Ea_avg, Eb_max, Eb_avg)
RESULTS_TEST1 = {
    22: ("4.76190e-02", "1.86048e-03", "2.67773e-04", "7.65805e-02", "6.53421e-03"),
    44: ("2.32558e-02", "4.44560e-04", "6.18187e-05", "1.95261e-02", "1.35063e-03"),
}


@pytest.mark.parametrize("n", (22, 44))
def test_pipeline_known_answer_rows(port, n):
    x, y, z, A1, b1 = analytic_case(n)
    ierr, A, B, ioptc, ropt = port.vector_potential(x, y, z, b1)
    assert ierr == 0
    eA = np.linalg.norm(A1 - A, axis=0)
    eB = np.linalg.norm(b1 - B, axis=0)
    got = tuple("{:.5e}".format(v) for v in (x[1] - x[0], eA.max(), eA.mean(), eB.max(), eB.mean()))
    assert got == RESULTS_TEST1[n]


@pytest.mark.parametrize("name,ns", (("pipeline_22", 22), ("pipeline_33x22x27", [33, 22, 27])))
def test_pipeline_golden(port, golden_dir, name, ns):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    x, y, z, A1, b1 = analytic_case(ns)
    ierr, A, B, ioptc, ropt = port.vector_potential(x, y, z, b1)
    assert ierr == 0 and np.array_equal(ioptc, g["ioptc"])
    # 2-D face solves carry the unordered mean reduction -> not bitwise
    assert np.abs(A - g["A"]).max() <= 1e-12 * np.abs(g["A"]).max()
    h = x[1] - x[0]
    assert np.abs(B - g["B"]).max() <= 1e-12 * np.abs(g["A"]).max() / h * 4


def test_live_reference_random(port, golden_dir):
    """(c): fresh random inputs against the reference's outputs on them (golden/reference_random.json holds the
    sha256 of each bit-identical output, golden/reference_random_NNNNNN.npz the all-Neumann sweeps)."""
    want = json.load(open(os.path.join(golden_dir, "reference_random.json")))
    nn = np.load(os.path.join(golden_dir, "reference_random_NNNNNN.npz"))
    for ns, mesh, u, rhs in random_reference_cases():
        tag = _tag(ns)
        for bcs in BCS_RANDOM:
            a = port.relax3d(u, rhs, mesh, bcs)
            if bcs == "NNNNNN":
                np.testing.assert_allclose(a, nn[f"relax_{tag}"], rtol=0, atol=1e-14)
            else:
                assert digest(a) == want[f"relax_{tag}_{bcs}"], (tag, bcs)
            assert digest(port.residual3d(u, rhs, mesh, bcs)) == want[f"residual_{tag}_{bcs}"], (tag, bcs)
        assert digest(port.vcycle(u, rhs, mesh, "DNDDND", ms=3)) == want[f"vcycle_{tag}_DNDDND_ms3"], tag


def _aniso_want(golden_dir):
    with open(os.path.join(golden_dir, "reference_aniso.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("ns", ANISO_SHAPES_3D, ids=_tag)
def test_kernels3d_aniso_golden(port, golden_dir, ns):
    """test_kernels3d_golden on aniso_mesh (a spacing of its own on every axis, no origin at 0), five BC sets: the
    reference's outputs as sha256 of their bits (golden/reference_aniso.json)"""
    want = _aniso_want(golden_dir)[_tag(ns)]
    mesh, u, rhs = aniso_case(ns)
    shapes, meshes = port.hierarchy(ns, mesh)
    assert shapes.tolist() == want["level_shapes"]
    for l, lv in enumerate(meshes):
        for d, m in enumerate(lv):
            assert digest(m) == want[f"mesh_l{l+1}_d{d+1}"], (l + 1, d + 1)
    for bcs in BCS_ANISO:
        assert digest(port.relax3d(u, rhs, mesh, bcs)) == want[f"relax_{bcs}"], bcs
        assert digest(port.residual3d(u, rhs, mesh, bcs)) == want[f"residual_{bcs}"], bcs
        assert digest(port.vcycle(u, rhs, mesh, bcs)) == want[f"vcycle_{bcs}"], bcs
    for lvl in range(1, len(shapes)):
        f = rand_field(tuple(int(v) for v in shapes[lvl - 1][::-1]), 3000 + lvl)
        c = rand_field(tuple(int(v) for v in shapes[lvl][::-1]), 4000 + lvl)
        assert digest(port.restrict(f, ns, mesh, lvl)) == want[f"restrict_l{lvl}"], lvl
        assert digest(port.interp(c, ns, mesh, lvl)) == want[f"interp_l{lvl}"], lvl


@pytest.mark.parametrize("bcs", BCS3)
def test_solve3d_aniso_history_golden(port, golden_dir, bcs):
    ns = ANISO_SHAPES_3D[0]
    h = _aniso_want(golden_dir)[f"solve_{_tag(ns)}_{bcs}"]
    mesh = aniso_mesh(ns)
    us, rhs = manufactured_poisson(mesh, bcs)
    ierr, u, du, hist, nc, sw = port.solve_bvp(np.zeros_like(us), rhs, mesh, bcs, hist_len=64)
    assert ierr == 0 and nc == h["ncycles"]
    assert list(hist) == h["du"]          # bit-identical residual history
    assert du == h["du"][-1]
    assert digest(u) == h["u"]


def test_kernels2d_aniso_golden(port, golden_dir):
    """test_kernels2d_golden on the first two axes of aniso_mesh, with its tolerances"""
    ns = ANISO_SHAPE_2D
    g = np.load(os.path.join(golden_dir, "reference_aniso_2d.npz"))
    mesh, u, rhs = aniso_case(ns)
    rhs0 = rhs - rhs.mean()
    shapes, _ = port.hierarchy(ns, mesh)
    assert np.array_equal(shapes, g["level_shapes"])
    for bcs in ("NNNN", "DNND"):
        np.testing.assert_allclose(port.relax_nd(u, rhs, mesh, bcs), g[f"relax_{bcs}"], rtol=0, atol=1e-14)
        assert np.array_equal(port.residual_nd(u, rhs, mesh, bcs), g[f"residual_{bcs}"])
    np.testing.assert_allclose(port.vcycle(u, rhs0, mesh, "NNNN"), g["vcycle_NNNN"], rtol=0, atol=1e-14)
    ierr, us, du, hist, nc, sw = port.solve_bvp(np.zeros(u.shape), rhs0, mesh, "NNNN", hist_len=64)
    assert ierr == int(g["solve_NNNN_meta"][0])
    np.testing.assert_allclose(us, g["solve_NNNN"], rtol=0, atol=1e-13)
    for lvl in range(1, len(shapes)):
        f = rand_field(tuple(int(v) for v in shapes[lvl - 1][::-1]), 3000 + lvl)
        c = rand_field(tuple(int(v) for v in shapes[lvl][::-1]), 4000 + lvl)
        assert np.array_equal(port.restrict(f, ns, mesh, lvl), g[f"restrict_l{lvl}"])
        assert np.array_equal(port.interp(c, ns, mesh, lvl), g[f"interp_l{lvl}"])


@pytest.mark.parametrize("name", ("analytic", "unbalanced"))
def test_pipeline_aniso_golden(port, golden_dir, name):
    """test_pipeline_golden where quirk Q4 is live: fluxes with dq(1) dq(2) on every face, grad chi with the normal
    spacing, the flux-balance fields at coordinates away from 0 (golden/pipeline_aniso_*.npz)"""
    g = np.load(os.path.join(golden_dir, f"pipeline_aniso_{name}.npz"))
    _name, x, y, z, b = [c for c in aniso_pipeline_cases() if c[0] == name][0]
    ierr, A, B, ioptc, ropt = port.vector_potential(x, y, z, b)
    assert ierr == 0 and np.array_equal(ioptc, g["ioptc"])
    assert np.abs(A - g["A"]).max() <= 1e-12 * np.abs(g["A"]).max()
    h = x[1] - x[0]
    assert np.abs(B - g["B"]).max() <= 1e-12 * np.abs(g["A"]).max() / h * 4


def test_quirk_ierr_is_the_last_face_solve(port, golden_dir):
    """Q3': ndsm_vector_potential.f90:480 stores the flag last written at :360 (2-D face 6), because
    `solve` (:598) keeps the 3-D flags in a local.  The reference's answers: golden/reference_quirks.json."""
    want = json.load(open(os.path.join(golden_dir, "reference_quirks.json")))
    x, y, z, b = quirk_case()
    ierr_ref, io_ref = want["top_face_zero"]["ierr"], want["top_face_zero"]["ioptc"]
    ierr_port, _, _, io_port, _ = port.vector_potential(x, y, z, b, ncycles_max=2)
    assert ierr_ref == 0 and ierr_port == 0          # although no 3-D solve reached vc_tol
    assert io_ref[3] == io_port[3] == 0
    # sanity: with B.n != 0 on that face the same budget does return 1
    x, y, z, A1, b1 = analytic_case(24)
    assert want["analytic"]["ierr"] == 1
    assert port.vector_potential(x, y, z, b1, ncycles_max=2)[0] == 1


# ---- edge values of the options: the port against what the reference returned (reference_options.json) ----
# Exact: the reference ran on one thread, and the port adds the all-Neumann mean in that serial order on any number.

@pytest.fixture(scope="module")
def ref_options(golden_dir):
    return json.load(open(os.path.join(golden_dir, "reference_options.json")))


def _pipe_row(port, x, y, z, b, kw):
    ierr, A, B, ioptc, _ropt = port.vector_potential(x, y, z, b, **kw)
    assert np.isfinite(A).all() and np.isfinite(B).all(), kw
    return [int(ierr), [int(v) for v in ioptc], digest16(A), digest16(B)]


@pytest.mark.parametrize("group,cases,zero", (("pipeline", pipeline_option_cases, False),
                                              ("pipeline_negative", negative_option_cases, False),
                                              ("pipeline_zero_field", zero_field_cases, True)),
                         ids=("matrix", "negative", "zero_field"))
def test_pipeline_options_reference(port, ref_options, group, cases, zero):
    """ndsm_vector_solve on the option matrix (ms 0 ... 11, no V-cycle, no coarsest-grid sweep, zero tolerances, both
    metrics), with negative values and on an all-zero field: ierr, the whole ioptc and the bits of A and B"""
    x, y, z, b = noisy_case(OPTION_PIPELINE_SHAPE)
    if zero:
        b = np.zeros_like(b)
    kws = cases()
    want = ref_options[group]
    assert len(kws) == len(want)
    for kw, w in zip(kws, want):
        assert _pipe_row(port, x, y, z, b, kw) == w, kw
    if group == "pipeline":
        assert len(kws) == 93
        # no cycle at all: whatever ms and the coarsest-grid count, the same A and B
        same = {tuple(w[2:]) for kw, w in zip(kws, want) if kw.get("ncycles_max") == 0}
        assert len(same) == 1
    if group == "pipeline_zero_field":
        assert [w[0] for w in want] == [1, 0]          # du = 0 < vc_tol is strict


def _scalar_row(port, u, rhs, mesh, bcs, kw):
    ierr, us, du, _h, nc, _sw = port.solve_bvp(u, rhs, mesh, bcs, **kw)
    assert np.isfinite(us).all(), (bcs, kw)
    return [int(ierr), float(du), digest16(us)], nc, us


@pytest.mark.parametrize("case", list(scalar_option_problems()), ids=lambda c: c[0])
def test_scalar_options_reference(port, ref_options, case):
    """solve_poisson_bvp on the option matrix, 3-D and 2-D, uniform and unequal spacings, the component letter
    sets and all-Neumann: ierr, du_last and the bits of u; without a V-cycle u comes back as passed"""
    name, ns, mesh, bcs, u, rhs = case
    want = ref_options["scalar"][name]
    opts = option_matrix()
    assert len(opts) == len(want) == 90
    for t, w in zip(opts, want):
        row, nc, us = _scalar_row(port, u, rhs, mesh, bcs, scalar_kw(*t))
        assert row == w, (name, t)
        assert nc <= t[1]
        if t[1] == 0:
            assert row[:2] == [1, HUGE] and nc == 0 and np.array_equal(us, u), (name, t)


def test_scalar_options_reference_negative_and_zero_field(port, ref_options):
    """negative counts behave as 0 (no sweeps, no cycles, no coarsest-grid sweeps), a negative or NaN vc_tol never
    converges; an all-zero problem: du = 0 misses vc_tol = 0 after all three cycles, meets 1e-10 after one"""
    name, ns, mesh, bcs, u, rhs = next(iter(scalar_option_problems()))
    kws = (dict(ms=-1, nmax=3), dict(nmax=-2), dict(nmax_exact=-3, nmax=3), dict(vc_tol=-1.0, nmax=3),
           dict(ex_tol=-1.0, nmax=3, nmax_exact=50), dict(vc_tol=float("nan"), nmax=3))
    want = ref_options["scalar_negative"]
    assert len(kws) == len(want)
    for kw, w in zip(kws, want):
        row, nc, us = _scalar_row(port, u, rhs, mesh, bcs, kw)
        assert row == w, kw
        for key, zero in (("ms", "ms"), ("nmax", "nmax"), ("nmax_exact", "nmax_exact")):
            if kw.get(key, 0) < 0:                     # ... and is what 0 gives
                row0, nc0, us0 = _scalar_row(port, u, rhs, mesh, bcs, dict(kw, **{key: 0}))
                assert row0 == row and nc0 == nc, kw
    z0 = np.zeros_like(u)
    for vt, w, nc_want in zip((0.0, 1e-10), ref_options["scalar_zero_field"], (3, 1)):
        row, nc, us = _scalar_row(port, z0, z0, mesh, bcs, dict(vc_tol=vt, nmax=3))
        assert row == w and nc == nc_want and row[1] == 0.0 and row[0] == (1 if vt == 0.0 else 0), vt
