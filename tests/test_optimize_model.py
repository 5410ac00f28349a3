"""CPU tests of the numpy model of the optimization-method solver (tests/optimize_model.py), the reference of
tests/test_gpu_optimize.py: the force is minus half the derivative of the model's own functional (which pins every sign
of DESIGN.md's formula), the iteration descends and keeps the faces, the stop rules and the history layout are the
documented ones, and boundary_weight is the documented profile.  No threshold here comes from the device code."""
import numpy as np
import pytest

import optimize_model as M


def unit(mesh):
    u = [(q - q[0]) / (q[-1] - q[0]) for q in mesh]
    return np.meshgrid(u[2], u[1], u[0], indexing="ij")


def smooth_w(mesh):
    """a smooth weight between 0.2 and 2.3 whose gradient has all three components"""
    Z, Y, X = unit(mesh)
    return 1.0 + 0.8 * np.sin(3.0 * X + 0.5) * np.cos(2.0 * Y) + 0.5 * Z


def derivative_error(n, variant="full"):
    """|dL_h/d eps - (-2 sum W F~.dB)| / |dL_h/d eps| for the perturbed ABC field on the n box, a smooth w and a
    smooth dB that vanishes on the faces; dL_h/d eps by a central difference in eps"""
    mesh = M.box(n)
    _, b = M.perturbed_abc(mesh)
    w = smooth_w(mesh)
    g = M.bump(mesh)
    Z, Y, X = unit(mesh)
    db = np.array([g * np.cos(3 * X + Y), g * np.sin(2 * Y - Z + 0.5), g * (0.5 + X * Z)])
    eps = 1e-5      # L is smooth in eps: the O(eps^2) term is 1e-10, the rounding of L over 2 eps about 1e-11
    dl = (M.functional(mesh, b + eps * db, w)[0] - M.functional(mesh, b - eps * db, w)[0]) / (2 * eps)
    pred = -2.0 * np.sum(M.weights(mesh, b.shape[1:]) * (M.force(mesh, b, w, variant=variant) * db).sum(axis=0))
    return abs(dl - pred) / abs(dl)


@pytest.fixture(scope="module")
def errors():
    return {n: derivative_error(n) for n in (17, 33, 65)}


def test_force_is_the_derivative_of_the_functional(errors):
    """second order: the error falls by at least 2.5 per halving (the ideal is 4, the margin that of the project's
    order tests).  Here: 8.9e-3, 1.0e-3, 2.1e-4 - ratios 8.5 and 5.0"""
    print("derivative errors", errors)
    assert errors[17] / errors[33] >= 2.5 and errors[33] / errors[65] >= 2.5, errors


@pytest.mark.parametrize("variant", ["no_pxgw", "no_sgw", "wf"])
def test_every_weight_term_is_needed(errors, variant):
    """at n = 65 the full force is at least five times closer to the derivative than the force without P x grad w,
    without s grad w, or with w F alone.  Here: 2.6e-2, 2.3e-2, 3.0e-3 against 2.1e-4"""
    e = derivative_error(65, variant)
    print(variant, e, errors[65])
    assert e >= 5.0 * errors[65], (variant, e, errors[65])


@pytest.fixture(scope="module", params=[None, 12], ids=["17x17x9", "17x12x9"])
def descent(request):
    mesh = M.box(17, request.param)
    exact, b = M.perturbed_abc(mesh)
    return exact, b, M.run(mesh, b, None, niter_max=400, check=50, tol=0.0)


def test_descent_from_the_perturbed_abc_field(descent):
    """400 tries from the ABC field with a 0.3 bump.  The model's own run: 17x17x9 L 0.320 -> 2.6e-4 (1240 x), error
    0.30 -> 3.8e-3 (79 x), 396 accepted; 17x12x9 L 0.318 -> 6.2e-4 (508 x), error 0.29 -> 5.3e-3 (55 x), 397 accepted.
    The thresholds are a quarter of the smaller factor of each"""
    exact, b, (B, hist, info, trace) = descent
    assert info == (9, 400, 0)
    assert all(x > y for x, y in zip(trace, trace[1:]))           # L never rises over the accepted tries
    assert len(trace) == 1 + int(hist[-1, 5]) and trace[-1] == hist[-1, 1]
    assert np.all(np.diff(hist[:, 1]) <= 0.0) and np.array_equal(hist[:, 0], np.arange(9) * 50.0)
    face = np.ones(b.shape[1:], dtype=bool)
    face[1:-1, 1:-1, 1:-1] = False
    assert np.array_equal(B[:, face].view(np.uint64), b[:, face].view(np.uint64))
    e0, e1 = np.abs(b - exact).max(), np.abs(B - exact).max()
    print("L", hist[0, 1], hist[-1, 1], "error", e0, e1, "accepted", hist[-1, 5])
    assert hist[-1, 1] <= hist[0, 1] / 125.0
    assert e1 <= e0 / 14.0
    assert np.all(hist[:, 1] == hist[:, 2] + hist[:, 3])
    assert hist[-1, 5] >= 380


def test_stop_rules_and_history_layout():
    mesh = M.box(9)
    _, b = M.perturbed_abc(mesh)
    # niter_max: 7 tries in intervals of 3 - rows at 0, 3, 6, 7
    B, hist, info, _ = M.run(mesh, b, None, niter_max=7, check=3, tol=0.0)
    assert info == (4, 7, 0) and hist.shape == (4, 6)
    assert list(hist[:, 0]) == [0.0, 3.0, 6.0, 7.0]
    h2 = min(M.spacing(mesh)) ** 2
    assert hist[0, 4] == 0.1 * h2 and hist[0, 5] == 0.0
    assert hist[-1, 4] == pytest.approx(0.1 * h2 * 1.01 ** hist[-1, 5] * 0.5 ** (7 - hist[-1, 5]), rel=1e-12)
    # rows run out: the last row is overwritten, the final state is last
    B2, hist2, info2, _ = M.run(mesh, b, None, niter_max=7, check=3, tol=0.0, hist_rows=2)
    assert info2 == (2, 7, 0) and np.array_equal(hist2, hist[[0, 3]]) and np.array_equal(B2, B)
    # tol: the first check finds a fall of less than 99.9 %
    _, hist, info, _ = M.run(mesh, b, None, niter_max=50, check=5, tol=0.999)
    assert info == (2, 5, 1) and hist[1, 0] == 5.0
    # dt_min: a first step far too large is rejected, and half of it is below dt_min
    B, hist, info, trace = M.run(mesh, b, None, niter_max=50, check=5, dt0=100.0, dt_min=60.0)
    assert info == (2, 1, 2) and list(hist[1, [0, 4, 5]]) == [1.0, 50.0, 0.0] and len(trace) == 1
    assert np.array_equal(B, b)
    # dt0 below dt_min: no try at all
    _, hist, info, _ = M.run(mesh, b, None, niter_max=50, check=5, dt0=1.0, dt_min=2.0)
    assert info == (1, 0, 2) and hist.shape == (1, 6)


def test_zero_nodes_and_the_zero_field():
    mesh = M.box(9)
    _, b = M.perturbed_abc(mesh)
    b[:, 2, 3, 4] = 0.0
    b[:, 0, 0, :] = 0.0
    p = M.point_terms(mesh, b)
    assert not p["ok"][2, 3, 4] and np.all(p["omega"][:, 2, 3, 4] == 0.0)
    L, Lf, Ld = M.functional(mesh, b, terms=p)
    assert np.isfinite(L) and L > 0.0 and np.all(np.isfinite(M.force(mesh, b, terms=p)))
    B, hist, info, _ = M.run(mesh, b, None, niter_max=3, check=1, tol=0.0)
    assert np.all(np.isfinite(hist)) and np.all(np.isfinite(B))
    z = np.zeros_like(b)
    B, hist, info, _ = M.run(mesh, z, None, niter_max=1, check=1, tol=0.0)
    assert hist[0, 1] == 0.0 and list(hist[1, [0, 1, 5]]) == [1.0, 0.0, 0.0] and hist[1, 4] == 0.5 * hist[0, 4]
    assert np.array_equal(B, z)


def test_boundary_weight():
    import ndsm_amd
    shape = (6, 9, 8)
    assert np.array_equal(ndsm_amd.boundary_weight(shape, 0), np.ones(shape))
    w = ndsm_amd.boundary_weight(shape, 1)
    assert w.shape == shape and np.all(w[:-1, 1:-1, 1:-1] == 1.0)
    assert np.all(w[-1] == 0.0) and np.all(w[:, 0] == 0.0) and np.all(w[:, -1] == 0.0)
    assert np.all(w[:, :, 0] == 0.0) and np.all(w[:, :, -1] == 0.0)
    w = ndsm_amd.boundary_weight(shape, 3)
    f = [0.5 * (1.0 + np.cos(np.pi * (3 - d) / 3)) for d in range(3)]        # 0, 1/4, 3/4
    assert f[0] == 0.0 and f[1] == pytest.approx(0.25) and f[2] == pytest.approx(0.75)
    assert list(w[0, 4, :]) == f + [1.0, 1.0] + f[::-1]                       # the lower face is untouched
    assert list(w[0, :, 4]) == f + [1.0, 1.0, 1.0] + f[::-1]
    assert list(w[:, 4, 4]) == [1.0, 1.0, 1.0] + f[::-1]
    assert w[4, 1, 2] == (f[1] * f[1]) * f[2]                                 # the factors are multiplied
    with pytest.raises(ValueError):
        ndsm_amd.boundary_weight(shape, -1)
