"""CPU tests of the skeleton semantics: the closed-form checks of test_gpu_skeleton.py run on the numpy restatement
(skeleton_model.skeleton_numpy), the property that ties it to the paths (every line is path_model.path_numpy's for its
seed and direction, a captured line a prefix of it), and the restatement behind the library's own Python layer
(model_run: the Skeleton tuple, spine_of, fan_of, connections)."""
import numpy as np
import pytest

from golden_inputs import aniso_mesh, uniform_mesh
from null_model import LINEAR
from skeleton_model import (CAPTURED, check_equals_paths, check_linear, check_no_type, check_separator, check_structure,
                            default_ring, linear_case, model_run, noise_nulls, separator_field, skeleton_numpy,
                            type_numpy)

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
SHAPE = [13, 11, 12]
SEPARATOR_CASES = [("uniform", [24, 30, 20]), ("aniso", [33, 22, 27]), ("uniform", [12, 14, 11]),
                   ("aniso", [12, 14, 11])]
CASE_ID = lambda v: v if isinstance(v, str) else "x".join(map(str, v))   # noqa: E731


@pytest.mark.parametrize("mname", list(MESHES))
@pytest.mark.parametrize("name", list(LINEAR))
def test_model_linear_nulls(mname, name):
    check_linear(skeleton_numpy, MESHES[mname](SHAPE), name)


def test_model_type_against_eig_on_random_matrices():
    """the lone eigenvalue of 20 000 random near-traceless matrices with scales 1e-6 .. 1e6 against
    numpy.linalg.eigvals: at most 40 iterations are allowed, far fewer are needed, and the relative error stays near rounding (the figures
    of DESIGN.md)"""
    rng = np.random.default_rng(41)
    n = 20000
    M = rng.uniform(-1.0, 1.0, (n, 3, 3))
    M[:, 2, 2] = -(M[:, 0, 0] + M[:, 1, 1]) + 1e-3 * rng.uniform(-1.0, 1.0, n)
    M *= 10.0 ** rng.uniform(-6.0, 6.0, n)[:, None, None]
    ok, s, kind, eig, v, w, e1, e2 = type_numpy(M)
    lam = np.linalg.eigvals(M)
    sdet = np.sign(np.linalg.det(M))
    # the lone eigenvalue: real, with the sign of the determinant, the other two on the other side
    real = np.abs(lam.imag) == 0.0
    cand = real & (np.sign(lam.real) == sdet[:, None])
    typed = cand.sum(axis=1) == 1
    lone = lam.real[np.arange(n), np.argmax(cand, axis=1)]
    assert ok[typed].mean() > 0.999
    both = ok & typed
    err = np.abs(eig[both, 0] - lone[both]) / np.abs(lone[both])
    print("random matrices: typed", int(both.sum()), "max iterations", int(type_numpy.last_iters.max()),
          "max relative error of the lone eigenvalue", err.max())
    assert type_numpy.last_iters.max() <= 20 and err.max() <= 1e-11
    assert np.all(kind[both] * sdet[both] < 0)
    # v and w are the right and left eigenvectors: |M v - lambda v| and |w M - lambda w| small, e1, e2, w orthonormal
    lamv = eig[both, 0][:, None]
    scale = np.abs(M[both]).max(axis=(1, 2))[:, None]
    gap = np.abs(lam[both] - lamv.astype(complex)).copy()
    gap.sort(axis=1)
    well = gap[:, 1] / scale[:, 0] > 1e-3                                     # (a well separated lone eigenvalue)
    rv = np.abs(np.einsum("nab,nb->na", M[both], v[both]) - lamv * v[both]) / scale
    rw = np.abs(np.einsum("na,nab->nb", w[both], M[both]) - lamv * w[both]) / scale
    assert rv[well].max() <= 1e-9 and rw[well].max() <= 1e-9
    for a, c in ((e1, e1), (e2, e2), (w, w)):
        assert np.abs((a[both] * c[both]).sum(axis=1) - 1.0).max() <= 1e-12
    for a, c in ((e1, e2), (e1, w), (e2, w)):
        assert np.abs((a[both] * c[both]).sum(axis=1)).max() <= 1e-12


@pytest.mark.parametrize("mname", list(MESHES))
def test_model_every_line_is_a_path(mname):
    """capture off: every line equals path_numpy of its seed and sign bit for bit; capture on: a captured line equals
    the matching prefix - on the nulls of white noise, where lines of every end occur"""
    mesh = MESHES[mname]([7, 5, 9])
    b, pos, jac = noise_nulls(mesh)
    assert len(pos) >= 8
    ring = default_ring(5)
    seen = set()
    for capture in (0.0, 0.5, 2.0):
        for every in (1, 3):
            sk = skeleton_numpy(mesh, b, pos, jac, ring, 0.5, capture, 0.5, 50, every)
            check_structure(sk, pos, 5, every)
            check_equals_paths(sk, mesh, b, pos, jac, ring, 0.5, 0.5, 50, every)
            assert (capture == 0.0) == (not np.any(sk.status == CAPTURED))
            seen |= set(sk.status.tolist())
    assert CAPTURED in seen and len(seen & set(range(1, 7))) >= 1, seen


@pytest.mark.parametrize("mname,shape", SEPARATOR_CASES, ids=CASE_ID)
def test_model_separator(mname, shape):
    """DESIGN.md's separator field: each null is connected to the other by exactly the four ring seeds that face it"""
    import ndsm_amd
    mesh = MESHES[mname](shape)
    for radius in (1.0, 0.5):
        sk, pos, jac, conn = check_separator(skeleton_numpy, mesh, radius)
        b, _rc, _aa = separator_field(mesh)
        # without capture the same lines do not end at the other null
        off = skeleton_numpy(mesh, b, pos, jac, default_ring(8), radius, 0.0, 0.5, 400, 1)
        assert not np.any(off.status == CAPTURED)
        for m, other, idx in conn:
            assert np.all((off.status[m * 10 + 2 + idx] == 8) | (off.status[m * 10 + 2 + idx] >= 5)), off.status
        # the same through the Python layer
        S = model_run(mesh, b, nulls=(pos, jac), radius=radius, nring=8, capture=0.5, max_steps=4000)
        got = ndsm_amd.connections(S)
        assert [(m, o) for m, o, _i in got] == [(0, 1), (1, 0)]
        for (m, o, idx), (_m, _o, want) in zip(got, conn):
            assert idx.tolist() == want.tolist() and len(idx) == 4


@pytest.mark.parametrize("mname", list(MESHES))
def test_model_nulls_without_a_type(mname):
    check_no_type(skeleton_numpy, MESHES[mname](SHAPE))


@pytest.mark.parametrize("mname", list(MESHES))
def test_model_python_layer(mname):
    """the Skeleton tuple of the Python layer and its helpers, on the restatement"""
    import ndsm_amd
    mesh = MESHES[mname](SHAPE)
    b, r0, _M = linear_case(mesh, "improper")
    S = model_run(mesh, b, nring=6)
    assert isinstance(S, ndsm_amd.Skeleton)
    assert S._fields == ("position", "kind", "eig", "spine", "normal", "paths", "hit")
    assert S.position.shape == (1, 3) and np.abs(S.position[0] - r0).max() <= 1e-12
    assert S.kind.tolist() == [1] and S.hit.shape == (1, 8) and np.all(S.hit == -1)
    fl = S.paths.lines
    assert fl.ends.shape == (1, 8, 3) and fl.status.shape == fl.nsteps.shape == fl.length.shape == (1, 8)
    assert fl.integral is None and fl.flh is None and S.paths.g is None and S.paths.integral is None
    spine, fan = ndsm_amd.spine_of(S, 0), ndsm_amd.fan_of(S, 0)
    assert len(spine) == 2 and len(fan) == 6 and ndsm_amd.connections(S) == []
    rho = 0.5 * min(q[1] - q[0] for q in mesh)
    for sign, (pts, bb) in zip((1.0, -1.0), spine):
        assert np.abs(pts[0] - (S.position[0] + sign * rho * S.spine[0])).max() <= 1e-15
        assert len(bb) == len(pts) and pts[-1].tobytes() == fl.ends[0, 0 if sign > 0 else 1].tobytes()
    for j, (pts, _bb) in enumerate(fan):
        assert abs(np.linalg.norm(pts[0] - S.position[0]) - rho) <= 1e-14
        assert abs((pts[0] - S.position[0]) @ S.normal[0]) <= 1e-15
        assert pts[-1].tobytes() == fl.ends[0, 2 + j].tobytes()
    for bad in (1, -1, 0.5):
        with pytest.raises(IndexError):
            ndsm_amd.spine_of(S, bad)
        with pytest.raises(IndexError):
            ndsm_amd.fan_of(S, bad)
