"""CPU tests of the numpy model of the magnetogram preprocessing (tests/preprocess_model.py), the reference of
tests/test_gpu_preprocess.py: the gradient is the derivative of the model's own functional (which pins every term and
sign of DESIGN.md's formula), the iteration descends and stays near the observation, the stop rules and the history
layout are the documented ones, and magnetogram_balance is the documented ratio.  No threshold here comes from the
device code."""
import numpy as np
import pytest

import preprocess_model as M
from golden_inputs import aniso_mesh, uniform_mesh

MESHES = {"33x22": (np.arange(33) * 0.1, np.arange(22) * 0.13, np.arange(3) * 0.1),
          "5x7": (np.arange(5) * 0.1, np.arange(7) * 0.13, np.arange(3) * 0.1)}
# planes with a three-point axis: the kernels take them, a handle does not (four points per axis), so the GPU tests
# cannot reach them and the formula is checked on them here.  3x3 has one interior node
for _nx, _ny in ((3, 3), (3, 4), (4, 3)):
    MESHES["%dx%d" % (_nx, _ny)] = (np.arange(_nx) * 0.1, np.arange(_ny) * 0.13, np.arange(3) * 0.1)
ONE = [tuple(1.0 if i == k else 0.0 for i in range(5)) for k in range(5)]
TERMS = {"all": M.MU, "mu1": ONE[0], "mu2": ONE[1], "mu3h": ONE[2], "mu3z": ONE[3], "mu4": ONE[4]}


def derivative_error(mesh, mu, variant="full"):
    """|dL/d eps - sum G.dB| / |dL/d eps| at B = Bo + 0.1 noise for a random dB on every node, edge nodes included;
    dL/d eps by the five-point central difference at eps = 1e-3, which is exact for the quartic L up to rounding"""
    obs = M.test_magnetogram(mesh)
    rng = np.random.default_rng(5)
    b = obs + 0.1 * rng.standard_normal(obs.shape)
    db = rng.standard_normal(obs.shape)
    E, Mm = M.norms(mesh, obs)
    s, lam = M.sums(mesh, b, obs)
    pred = float(np.sum(M.gradient(mesh, b, obs, mu, s, lam, E, Mm, variant) * db))
    eps = 1e-3

    def f(k):
        return M.value(mesh, b + (k * eps) * db, obs, mu, E, Mm)
    dl = (8.0 * (f(1) - f(-1)) - (f(2) - f(-2))) / (12.0 * eps)
    return abs(dl - pred) / abs(dl)


@pytest.mark.parametrize("term", list(TERMS))
@pytest.mark.parametrize("shape", list(MESHES))
def test_gradient_is_the_derivative_of_the_functional(shape, term):
    """every mu together and each term alone.  Here: at most 1.8e-12 (33x22, mu3h alone); a wrong or missing term
    gives O(1)"""
    e = derivative_error(MESHES[shape], TERMS[term])
    print(shape, term, e)
    assert e <= 1e-9, (shape, term, e)


@pytest.mark.parametrize("variant,mu", [("no_s6", M.MU), ("no_s6", ONE[1]), ("flip_gy_x", M.MU), ("flip_gy_x", ONE[1]),
                                        ("plain_laplacian", M.MU), ("plain_laplacian", ONE[4])])
@pytest.mark.parametrize("shape", list(MESHES))
def test_the_check_has_teeth(shape, variant, mu):
    """without the S6 terms, with the sign of the x-factor of G_y flipped, or with the Laplacian of an unzeroed
    Laplacian in place of the transposed stencil, the same check fails by far.  Here: between 2.9e-2 and 1.5"""
    e = derivative_error(MESHES[shape], mu, variant)
    print(shape, variant, mu, e)
    assert e > 1e-3, (shape, variant, e)


@pytest.fixture(scope="module", params=["uniform", "aniso"])
def descent(request):
    mesh = {"uniform": uniform_mesh, "aniso": aniso_mesh}[request.param]([33, 22, 3])
    b = M.test_magnetogram(mesh)
    return request.param, b, M.run(mesh, b, niter_max=2000, check=50, tol=0.0)


# the model's own run of 2000 tries with the defaults (the thresholds below are a quarter of each factor):
#   uniform 33x22  L 2.23e-2 -> 2.66e-4 (84 x), eps_force 0.153 -> 3.6e-4 (418 x), eps_torque 3.95e-2 -> 2.8e-5 (1404 x),
#                  max |B - Bo| 0.31 / 0.23 / 0.20, 1976 accepted
#   aniso 33x22    L 2.46e-2 -> 2.04e-4 (121 x), eps_force 0.196 -> 3.5e-4 (554 x), eps_torque 6.13e-2 -> 4.4e-5 (1389 x),
#                  max |B - Bo| 0.29 / 0.21 / 0.20, 1976 accepted
FACTORS = {"uniform": (84.0, 418.0, 1404.0), "aniso": (121.0, 554.0, 1389.0)}


def test_descent_of_the_test_magnetogram(descent):
    name, b, (B, hist, info, trace) = descent
    assert info == (41, 2000, 0) and hist.shape == (41, 17)
    assert all(x > y for x, y in zip(trace, trace[1:]))           # L falls at every accepted try
    assert len(trace) == 1 + int(hist[-1, 8]) and trace[-1] == hist[-1, 1]
    assert np.array_equal(hist[:, 0], np.arange(41) * 50.0)
    ef, et = M.balance(hist)
    change = [float(np.abs(B[c] - b[c]).max()) for c in range(3)]
    print(name, "L", hist[0, 1], hist[-1, 1], "force", ef[0], ef[-1], "torque", et[0], et[-1], "change", change,
          "accepted", hist[-1, 8])
    fl, ff, ft = FACTORS[name]
    assert hist[-1, 1] <= hist[0, 1] / (fl / 4.0)
    assert ef[-1] <= ef[0] / (ff / 4.0)
    assert et[-1] <= et[0] / (ft / 4.0)
    assert max(change) < 0.5
    mu = np.array(M.MU)
    assert np.allclose(hist[:, 1], hist[:, 2:7] @ mu, rtol=1e-14, atol=0.0)
    assert hist[0, 4] == 0.0 and hist[0, 5] == 0.0                 # the start is the observation
    assert hist[-1, 8] >= 1900


def test_stop_rules_and_history_layout():
    mesh = uniform_mesh([9, 8, 3])
    b = M.test_magnetogram(mesh)
    # niter_max: 7 tries in intervals of 3 - rows at 0, 3, 6, 7
    B, hist, info, _ = M.run(mesh, b, niter_max=7, check=3, tol=0.0)
    assert info == (4, 7, 0) and hist.shape == (4, 17)
    assert list(hist[:, 0]) == [0.0, 3.0, 6.0, 7.0]
    assert hist[0, 7] == 0.01 and hist[0, 8] == 0.0
    assert hist[-1, 7] == pytest.approx(0.01 * 1.01 ** hist[-1, 8] * 0.5 ** (7 - hist[-1, 8]), rel=1e-12)
    E, Mm = M.norms(mesh, b)
    assert hist[0, 15] == E and hist[0, 16] == Mm                 # obs = None: S10, S11 of row 0 are E and M
    # rows run out: the last row is overwritten, the final state is last
    B2, hist2, info2, _ = M.run(mesh, b, niter_max=7, check=3, tol=0.0, hist_rows=2)
    assert info2 == (2, 7, 0) and np.array_equal(hist2, hist[[0, 3]]) and np.array_equal(B2, B)
    # tol: the first check finds a fall of less than 99.9 %
    _, hist, info, _ = M.run(mesh, b, niter_max=50, check=5, tol=0.999)
    assert info == (2, 5, 1) and hist[1, 0] == 5.0
    # dt_min: a first step far too large is rejected, and half of it is below dt_min
    B, hist, info, trace = M.run(mesh, b, niter_max=50, check=5, dt0=100.0, dt_min=60.0)
    assert info == (2, 1, 2) and list(hist[1, [0, 7, 8]]) == [1.0, 50.0, 0.0] and len(trace) == 1
    assert np.array_equal(B, b)
    # dt0 below dt_min: no try at all
    _, hist, info, _ = M.run(mesh, b, niter_max=50, check=5, dt0=1.0, dt_min=2.0)
    assert info == (1, 0, 2) and hist.shape == (1, 17)
    # mu all zero: L = 0, and a first try that is rejected
    B, hist, info, _ = M.run(mesh, b, mu=(0, 0, 0, 0, 0), niter_max=1, check=1, tol=0.0)
    assert hist[0, 1] == 0.0 and list(hist[1, [0, 1, 8]]) == [1.0, 0.0, 0.0] and hist[1, 7] == 0.5 * hist[0, 7]
    assert np.array_equal(B, b)
    # continuation: 3 tries, then 4 more against the original observation from the last dt = one call of 7
    B7, hist7, _, _ = M.run(mesh, b, niter_max=7, check=7, tol=0.0)
    B3, hist3, _, _ = M.run(mesh, b, niter_max=3, check=3, tol=0.0)
    B4, hist4, _, _ = M.run(mesh, B3, obs=b, niter_max=4, check=4, tol=0.0, dt0=hist3[-1, 7])
    assert np.array_equal(B4.view(np.uint64), B7.view(np.uint64)) and hist4[-1, 1] == hist7[-1, 1]
    with pytest.raises(ValueError):
        M.run(mesh, np.zeros_like(b), niter_max=1)


@pytest.mark.parametrize("nx,ny", [(3, 3), (3, 4), (4, 3), (257, 3)])
def test_planes_with_a_three_point_axis(nx, ny):
    """7 tries descend on the planes no handle exists for; at 257x3 a reduction thread walks two points of a row"""
    mesh = uniform_mesh([nx, ny, 3])
    b = M.test_magnetogram(mesh)
    B, hist, info, trace = M.run(mesh, b, niter_max=7, check=3, tol=0.0)
    assert info == (4, 7, 0) and np.isfinite(hist).all() and hist[-1, 8] >= 6
    assert all(x > y for x, y in zip(trace, trace[1:])) and hist[-1, 1] < hist[0, 1]
    lam = M.laplacians(mesh, B)
    edge = np.ones(lam.shape[1:], dtype=bool)
    edge[1:-1, 1:-1] = False
    assert not lam[:, edge].any() and lam[:, ~edge].all()


def test_magnetogram_balance():
    import ndsm_amd
    rows = np.zeros((2, 17))
    rows[0, 9:17] = [1.0, -2.0, 3.0, -4.0, 5.0, -6.0, 12.0, 30.0]
    rows[1, 9:17] = [0.0, 0.0, -0.5, 0.25, 0.0, 0.0, 2.0, 0.5]
    ef, et = ndsm_amd.magnetogram_balance(rows)
    assert list(ef) == [0.5, 0.25] and list(et) == [0.5, 0.5]
    one = ndsm_amd.magnetogram_balance(rows[0])
    assert float(one[0]) == 0.5 and float(one[1]) == 0.5
    mf, mt = M.balance(rows)
    assert np.array_equal(mf, ef) and np.array_equal(mt, et)
    with pytest.raises(ValueError):
        ndsm_amd.magnetogram_balance(np.zeros((2, 6)))
