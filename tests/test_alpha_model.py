"""CPU tests of the numpy restatement of the alpha map (tests/alpha_model.py), the reference that the device kernel
is held to bit for bit (test_gpu_alpha_map.py): on fields whose lines and alpha are known in closed form the
restatement itself is right."""
import numpy as np
import pytest

from alpha_model import ZLO, alpha_map_numpy, default_max_steps, flux_tube, node_seeds, tube_mesh
from golden_inputs import aniso_mesh, uniform_mesh
from line_model import box, uniform_b

SHAPES = [(2, 2, 2), (5, 7, 3), (17, 12, 9)]
MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}


def linear_alpha0(mesh):
    lo, _h, hi, _n = box(mesh)

    def f(x, y):
        return 0.7 + 1.3 * (x - lo[0]) / (hi[0] - lo[0]) - 0.9 * (y - lo[1]) / (hi[1] - lo[1])
    X, Y = np.meshgrid(mesh[0], mesh[1], indexing="xy")
    return f(X, Y), f


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", sorted(MESHES))
def test_uniform_tilted_field(kind, shape):
    """b = (0.3, -0.2, 0.9): RK4 lines are straight and exact, the bilinear interpolant of a linear alpha0 too.  With
    polarity +1 a node whose straight back-line meets z = lo inside the box gets alpha0 of that foot (1e-13
    relative); one whose back-line leaves through a side face first gets exactly 0 and that face's status.  With
    polarity -1 no line comes back to the lower face: all zeros."""
    mesh = MESHES[kind](shape)
    lo, _h, hi, _n = box(mesh)
    bv = (0.3, -0.2, 0.9)
    b = uniform_b(mesh, bv)
    alpha0, f = linear_alpha0(mesh)
    ms = default_max_steps(mesh, 0.5)
    alpha, status = alpha_map_numpy(mesh, b, alpha0, 1, 0.5, ms)
    P = node_seeds(mesh)
    t = (P[:, 2] - lo[2]) / bv[2]
    fx, fy = P[:, 0] - bv[0] * t, P[:, 1] - bv[1] * t
    ext = hi - lo
    margin = 1e-9
    dist = np.minimum(np.minimum(fx - lo[0], hi[0] - fx) / ext[0], np.minimum(fy - lo[1], hi[1] - fy) / ext[1])
    reach, miss = dist > margin, dist < -margin
    a, s = alpha.reshape(-1), status.reshape(-1)
    assert reach.any()
    assert np.all(s[reach] == ZLO)
    want = f(fx, fy)
    scale = np.abs(alpha0).max()
    assert np.abs(a - want)[reach].max() <= 1e-13 * scale
    if miss.any():
        assert np.all((s[miss] >= 1) & (s[miss] <= 4))
        assert np.all(a[miss] == 0.0) and not np.any(np.signbit(a[miss]))
    # along B nothing returns to the lower face
    alpha_m, status_m = alpha_map_numpy(mesh, b, alpha0, -1, 0.5, ms)
    assert np.all(alpha_m == 0.0) and not np.any(np.signbit(alpha_m))
    assert not np.any(status_m == ZLO)


def test_flux_tube_alpha_converges():
    """The Gold-Hoyle tube with a potential envelope (q a = 1), alpha0 its analytic alpha on k = 0, polarity +1: the
    mapped alpha against the analytic one over the nodes with r <= 0.8 a on (n, n, 9) boxes of fixed height.  The
    error is that of the bilinear interpolant and of the traced foot, second order in h.  Measured: 1.05e-1, 3.07e-2,
    8.36e-3 at n = 17, 33, 65 (max alpha 6.67): ratios 3.42 and 3.67.  Asserted: 2.5 per halving, the ideal 4 with the
    margin of the step-order tests (10 of an ideal 16).  test_gpu_squash.assert_order itself cannot be called here:
    its factor 10 is fixed for a fourth-order quantity under a halved step, and this one is second order in h."""
    errors = []
    for n in (17, 33, 65):
        mesh = tube_mesh(n)
        b, alpha_true, r, a = flux_tube(mesh)
        alpha, status = alpha_map_numpy(mesh, b, alpha_true[0], 1, 0.5, default_max_steps(mesh, 0.5))
        core = r <= 0.8 * a
        assert np.all(status[core] == ZLO)
        errors.append(np.abs(alpha - alpha_true)[core].max())
    print("flux tube, max |alpha - analytic| over r <= 0.8 a at n = 17, 33, 65:", errors)
    for coarse, fine in zip(errors[:-1], errors[1:]):
        assert coarse / fine >= 2.5, errors
