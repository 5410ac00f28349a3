"""The CPU model of the mixed-precision solve (tests/mixed_model.py) against the oracle - no GPU.

test_gpu_mixed.py bounds the device's mixed cycle by the distance between this model run in float32 and the fp64
V-cycle.  That bound means something only if the model IS the reference's cycle: here its V-cycle composition and its
own level-1 operators, run in float64, are compared with the oracle bit for bit, and the float64 model as a whole
(the cycle on the error equation instead of on u) must lie at least a factor 1000 closer to the oracle's V-cycle
than the float32 one (measured: a factor of about 1e8).
"""
import numpy as np
import pytest

import mixed_model as mm
from golden_inputs import rand_field

SHAPES = [pytest.param(ns, meshf, id=("aniso-" if meshf is mm.aniso_mesh else "") + "x".join(map(str, ns)))
          for ns, meshf in mm.MIXED_SHAPES]
BCS_V = ("NDDNDD", "DNNNDD", "DDDDDD")


def _fields(ns, seed=0):
    shp = tuple(ns[::-1])
    return rand_field(shp, 2112 + seed), rand_field(shp, 2113 + seed) * 10.0


def test_case_selection_covers_the_matrix():
    cases = mm.mixed_cases()
    assert len(cases) <= 60 and len({mm.case_id(c) for c in cases}) == len(cases)
    for ns, meshf in mm.MIXED_SHAPES:
        mine = [c for c in cases if c[0] == ns and c[1] is meshf]
        assert len({c[2] for c in mine}) >= 2
        assert {c[3] & 1 for c in mine} == {0, 1}
        assert {c[4] for c in mine} == {False, True}
        assert {c[5] for c in mine} == {False, True}
    assert {c[3] for c in cases} == set(mm.MIXED_MS)
    used = {c[2] for c in cases}
    assert "NNNNNN" not in used
    for f in range(6):                       # every face Neumann somewhere, and Dirichlet opposite a Neumann face
        assert any(b[f] == "N" for b in used)
        assert any(b[f] == "D" and b[(f + 3) % 6] == "N" for b in used)


@pytest.mark.parametrize("ns,meshf", SHAPES)
def test_vcycle_composition_bitwise(port, ns, meshf):
    """vcycle_from(level 1) is port.vcycle: every shape, ms 1, 2, 5, both coarsest-grid metrics, three letter sets"""
    mesh = meshf(ns)
    u, rhs = _fields(ns)
    for bcs in BCS_V:
        for ms in (1, 2, 5):
            for du_max in (True, False):
                ex_tol = 1e-13
                got = mm.vcycle_from(port, 1, u, rhs, ns, mesh, bcs, ms, ex_tol, du_max, 10000)
                want = port.vcycle(u, rhs, mesh, bcs, ms=ms, ex_tol=ex_tol, du_max=du_max, nmax_exact=10000)
                assert np.array_equal(got, want), (bcs, ms, du_max, np.abs(got - want).max())


@pytest.mark.parametrize("ns,meshf", SHAPES)
def test_level1_operators_bitwise_in_fp64(port, ns, meshf):
    """the model's own sweep, residual, restriction and prolongation in float64 are the oracle's, bit for bit, with a
    right-hand side and with none"""
    mesh = meshf(ns)
    u, rhs = _fields(ns, 7)
    _shapes, meshes = port.hierarchy(ns, mesh)
    zero = np.zeros_like(u)
    for bcs in mm.MIXED_BCS:
        for r in (rhs, None):
            rp = zero if r is None else r
            s1 = mm.sweep(u, r, mesh, bcs)
            assert np.array_equal(s1, port.relax3d(u, rp, mesh, bcs)), ("sweep", bcs, r is None)
            assert np.array_equal(mm.sweep(s1, r, mesh, bcs), port.relax3d(s1, rp, mesh, bcs)), ("sweep 2", bcs)
            assert np.array_equal(mm.residual(u, r, mesh, bcs), port.residual3d(u, rp, mesh, bcs)), ("residual", bcs)
    got = mm.restrict_from(u, meshes[0], meshes[1])
    assert np.array_equal(got, port.restrict(u, ns, mesh, 1)), "restrict"
    uc = rand_field(got.shape, 99)
    assert np.array_equal(mm.interp_to(uc, meshes[0], meshes[1]), port.interp(uc, ns, mesh, 1)), "interp"
    assert np.array_equal(mm.prolong_add(u, uc, meshes[0], meshes[1]), u + port.interp(uc, ns, mesh, 1)), "prolong + add"
    # float32: a float32 fine field restricts as its float64 copy, and the sum u + P u_c is rounded once
    u32 = u.astype(np.float32)
    assert np.array_equal(mm.restrict_from(u32, meshes[0], meshes[1]), port.restrict(u32.astype(np.float64), ns, mesh, 1))
    p32 = mm.prolong_add(u32, uc, meshes[0], meshes[1])
    assert p32.dtype == np.float32
    assert np.array_equal(p32, (u32.astype(np.float64) + port.interp(uc, ns, mesh, 1)).astype(np.float32))
    assert mm.sweep(u32, rhs, mesh, "NDDNDD", np.float32).dtype == np.float32


@pytest.mark.parametrize("case", mm.mixed_cases(), ids=mm.case_id)
def test_separation_and_dirichlet_faces(port, case):
    """dev64 <= dev32 / 1000, where dev = max|u_1(model in that type) - port.vcycle(u_0)|: the float32 signal the GPU
    test's bound is made of stands far above what the model differs from the oracle by construction (the cycle runs on
    the error equation).  And every Dirichlet face the prolongation cannot leak into (mixed_model.leak_free_faces)
    keeps u_0's bits through every cycle - the oracle's and the model's in both types."""
    ns, meshf, bcs, ms, mean, has_rhs = case
    mesh = meshf(ns)
    u0, rhs = _fields(ns)
    rhs = rhs if has_rhs else None
    want = port.vcycle(u0, np.zeros_like(u0) if rhs is None else rhs, mesh, bcs, ms=ms, du_max=not mean)
    us32, du32 = mm.mixed_cycles(port, u0, rhs, mesh, bcs, ms, 2, mean, np.float32)
    us64, _du64 = mm.mixed_cycles(port, u0, rhs, mesh, bcs, ms, 1, mean, np.float64)
    dev32, dev64 = np.abs(us32[0] - want).max(), np.abs(us64[0] - want).max()
    print("%s: dev32 %.3e dev64 %.3e ratio %.3g  (max|u1 - u0| %.3e, du %.3e -> %.3e)" % (
        mm.case_id(case), dev32, dev64, dev32 / max(dev64, 1e-300), np.abs(want - u0).max(), du32[0], du32[1]))
    assert dev32 > 0.0 and dev64 <= dev32 / 1000.0, (dev32, dev64)
    faces = mm.leak_free_faces(port, ns, mesh, bcs)
    for u in us32 + us64 + [want]:
        assert mm.faces_kept(u, u0, faces), (bcs, faces)


def test_leak_free_faces_are_all_but_the_upper_ones_of_uneven_meshes(port):
    """on the uniform meshes every Dirichlet face is leak free (so the GPU test checks all of them); on aniso_mesh the
    lower ones are, and whichever upper ones are not are faces the oracle's own V-cycle moves"""
    for ns, meshf in mm.MIXED_SHAPES:
        mesh = meshf(ns)
        faces = mm.leak_free_faces(port, ns, mesh, "DDDDDD")
        every = [(d, side) for d in range(3) for side in (0, -1)]
        assert all((d, 0) in faces for d in range(3))
        if meshf is not mm.aniso_mesh:
            assert faces == every
            continue
        u0, rhs = _fields(ns)
        got = port.vcycle(u0, rhs, mesh, "DDDDDD")
        for f in every:
            if f not in faces:
                assert not mm.faces_kept(got, u0, [f]), (ns, f)
