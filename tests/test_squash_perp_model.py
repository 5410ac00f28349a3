"""CPU tests of the numpy restatement of the perpendicular squashing factor (squash_perp_model.squash_perp_numpy,
the yardstick of test_gpu_squash_perp.py): its q and line outputs are line_model.squash_numpy's bit for bit, and
Q-perp passes the closed-form checks the device is held to - a uniform field (2 for every pair of faces, where Q is
not), the helical field (2 on every line, and the twist number), a hyperbolic field (a closed form on and off the
axis, with and without side faces), finite differences of traced lines, the invariance along a line, and the failure
ends.  The figures printed here are the ones quoted in DESIGN.md "Perpendicular squashing factor"."""
import numpy as np
import pytest

from golden_inputs import aniso_mesh, uniform_mesh
from line_model import abc, face_seeds, inner_seeds, squash_numpy
from test_gpu_squash import CONST_SHAPES, FD_SHAPES, along_line_spread, assert_order
from test_gpu_squash import numpy_tracer as forward_tracer
import squash_perp_model as P

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
KINDS = ["aniso", "uniform"]
SHAPE = [24, 27, 22]


@pytest.mark.parametrize("case", ["noG", "G1"])
@pytest.mark.parametrize("kind,shape,step", [("aniso", [33, 22, 27], 0.5), ("uniform", [24, 30, 20], 0.37)])
def test_q_and_the_lines_are_squash_numpy_bitwise(kind, shape, step, case):
    mesh = MESHES[kind](shape)
    b = abc(mesh)
    g = None if case == "noG" else abc(mesh, k=0.7 * np.pi, phase=0.3)
    integrand = 1 if case == "G1" else 0
    rng = np.random.default_rng(2119)
    seeds = np.concatenate([inner_seeds(mesh, rng, 60), face_seeds(mesh, rng, 6)])
    want = squash_numpy(mesh, b, g, seeds, step, 300, integrand)
    got = P.squash_perp_numpy(mesh, b, g, seeds, step, 300, integrand)
    assert len(got) == 7
    for name, x, y in zip(("q", "ends", "length", "integral", "status", "nsteps"), (got[0],) + got[2:], want):
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), name
    # Q-perp exists where Q does, is another number, and both kinds of end occur
    assert np.array_equal(np.isnan(got[1]), np.isnan(got[0])) and np.isfinite(got[1]).sum() >= len(seeds) // 2
    ok = np.isfinite(got[0])
    assert np.abs(got[1][ok] / got[0][ok] - 1.0).max() > 0.1
    assert set(got[5].reshape(-1).tolist()) >= set(P.FACES)


@pytest.mark.parametrize("kind", KINDS)
def test_uniform_field(kind):
    mesh = MESHES[kind](SHAPE)
    err, qmax = P.check_uniform(P.model_run, mesh, P.uniform_seeds(mesh))
    assert qmax > 10.0


@pytest.mark.parametrize("kind", KINDS)
def test_helical_field_and_twist(kind):
    mesh = MESHES[kind](SHAPE)
    eq, et = P.helical_errors(P.model_run, mesh)
    print(kind, "helical, |Q-perp - 2| / 2 at steps 1, 0.5, 0.25:", eq, "T_w:", et)
    assert eq[0] / eq[2] >= 100.0 and eq[2] < 1e-7
    assert et[0] / et[2] >= 100.0 and et[2] < 1e-6


@pytest.mark.parametrize("alpha_lz", [1.0, 3.0])
@pytest.mark.parametrize("kind", KINDS)
def test_hyperbolic_field(kind, alpha_lz):
    mesh = MESHES[kind](SHAPE)
    errs, want, m = P.hyperbolic_errors(P.model_run, mesh, alpha_lz)
    assert_order(errs, f"{kind} hyperbolic, alpha Lz = {alpha_lz}, Q-perp")
    ratio = np.abs(m.q / m.q_perp - 1.0)
    print("Q-perp from", want.min(), "to", want.max(), "max |Q / Q-perp - 1|", np.nanmax(ratio))
    if alpha_lz > 1.0:
        assert np.nanmax(ratio) > 0.5          # Q in its place would be far off


@pytest.mark.parametrize("kind", KINDS)
def test_against_finite_differences_of_trace(kind):
    """the coarsest mesh only (the finest takes the CPU a while and runs in the GPU test); the gap is small next to
    the difference between Q and Q-perp on the same seeds"""
    mesh = MESHES[kind](FD_SHAPES[kind][0])
    table = [P.fd_gap(P.model_run, P.numpy_tracer, mesh, d) for d in P.FD_DELTAS]
    gaps = [row[0] for row in table]
    q_perp, q = table[0][2], table[0][3]
    print(kind, "gaps at delta = 1e-3, 1e-4, 1e-5:", gaps, "left out", [r[1] for r in table],
          "|Q / Q-perp - 1| from", np.abs(q / q_perp - 1).min(), "to", np.abs(q / q_perp - 1).max())
    assert max(row[1] for row in table) <= 0.10
    assert np.abs(q / q_perp - 1).max() > 50.0 * min(gaps)          # a Q-perp that returned Q would miss by far


def test_q_perp_is_constant_along_a_line():
    kind = "aniso"
    spread = []
    for shape in CONST_SHAPES[kind][:2]:
        mesh = MESHES[kind](shape)
        s, q = along_line_spread(P.perp_as_q(P.model_run), forward_tracer, mesh)
        spread.append(s)
        assert q.max() / q.min() > 1.2
    print("spread of Q-perp along a line:", spread)
    assert spread[0] > spread[1]


@pytest.mark.parametrize("kind", KINDS)
def test_failure_ends(kind):
    P.check_failure_ends(P.model_run, P.numpy_tracer, MESHES[kind]([20, 17, 23]))


def test_seeds_do_not_depend_on_each_other():
    mesh = aniso_mesh([12, 11, 10])
    b = abc(mesh)
    seeds = inner_seeds(mesh, np.random.default_rng(5), 9)
    ref = P.squash_perp_numpy(mesh, b, None, seeds, 0.5, 100)
    rev = P.squash_perp_numpy(mesh, b, None, seeds[::-1], 0.5, 100)
    one = P.squash_perp_numpy(mesh, b, None, seeds[8:9], 0.5, 100)
    assert np.array_equal(ref[1][::-1], rev[1], equal_nan=True) and np.array_equal(ref[1][8:9], one[1], equal_nan=True)
    assert np.array_equal(ref[2][:, ::-1], rev[2]) and np.array_equal(ref[5][:, 8:9], one[5])
