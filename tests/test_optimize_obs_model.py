"""CPU tests of the numpy model of the optimization method with a measurement term and a freed lower face
(tests/optimize_obs_model.py), the reference of tests/test_gpu_optimize_obs.py: H on the freed face is minus half the
derivative of the model's own functional to second order, and every term, sign and factor of it is needed; the
iteration with a freed face descends where the fixed face stalls, and pulls a noisy face towards the exact field; the
held face, the history layout and the stop rules are the documented ones; measurement_weight is the documented
profile.  No threshold here comes from the device code."""
import numpy as np
import pytest

import optimize_model as M
import optimize_obs_model as O


def unit(mesh):
    u = [(q - q[0]) / (q[-1] - q[0]) for q in mesh]
    return np.meshgrid(u[2], u[1], u[0], indexing="ij")


def nonseparable_w(mesh):
    """test_gpu_optimize's weight that is not a product of 1-D factors, between 0.2 and 2.3"""
    Z, Y, X = unit(mesh)
    return 1.0 + 0.8 * np.sin(3.0 * X + 0.5 + Y * Z) * np.cos(2.0 * Y) + 0.5 * Z * X


def derivative_error(n, variant="full"):
    """|dL/d eps - (-2 sum W F~.dB - 2 sum W(k = 0) H.dB)| / |dL/d eps| on the n box, L = L_h + nu L_m: the perturbed
    ABC field plus a part that is neither force-free nor zero on the lower face, a non-separable w, and a smooth dB
    that vanishes on the rim, the side faces and the top but not on the lower face; dL/d eps by a central difference"""
    mesh = M.box(n)
    exact, b = M.perturbed_abc(mesh)
    Z, Y, X = unit(mesh)
    b = b + 0.2 * np.array([np.sin(np.pi * X) * np.cos(2.0 * Z), Y * np.cos(3.0 * Z), X * Y * (1.0 - Z)])
    w = nonseparable_w(mesh)
    g = (np.sin(np.pi * X) * np.sin(np.pi * Y)) ** 2 * np.cos(0.5 * np.pi * Z) ** 2
    db = np.array([1.0 * g, -0.6 * g, 0.8 * g])
    bobs = exact[:, 0] + 0.1
    wm = np.empty_like(bobs)
    wm[:2], wm[2] = 0.3, 1.0
    nu = 0.7
    eps = 1e-5      # L is smooth in eps: the O(eps^2) term is 1e-10, the rounding of L over 2 eps about 1e-11
    dl = (O.functional(mesh, b + eps * db, bobs, wm, nu, w)[0] -
          O.functional(mesh, b - eps * db, bobs, wm, nu, w)[0]) / (2 * eps)
    ft, h = O.forces(mesh, b, bobs, wm, nu, w, variant=variant)
    W = M.weights(mesh, b.shape[1:])
    pred = -2.0 * np.sum(W * (ft * db).sum(axis=0)) - 2.0 * np.sum(W[0] * (h * db[:, 0]).sum(axis=0))
    return abs(dl - pred) / abs(dl)


@pytest.fixture(scope="module")
def errors():
    return {n: derivative_error(n) for n in (17, 33, 65)}


def test_face_force_is_the_derivative_of_the_functional(errors):
    """H is a consistent discretisation, not the exact discrete gradient: the error falls with the mesh, by at least 5
    from n = 17 to n = 65.  Here: 2.9e-2, 2.0e-3, 1.7e-3 - a factor 17"""
    print("derivative errors", errors)
    assert errors[65] <= errors[17] / 5.0, errors


@pytest.mark.parametrize("n", [33, 65])
def test_the_volume_force_at_the_face_is_needed(errors, n):
    """with the surface term G alone the error is first order: 6.8e-2 at n = 33 and 3.3e-2 at n = 65 against 2.0e-3 and
    1.7e-3 - 34 and 19 times the full H's; at least 8 times is asserted"""
    e = derivative_error(n, "g_only")
    print(n, e, errors[n])
    assert e >= 8.0 * errors[n], (n, e, errors[n])


@pytest.mark.parametrize("variant", ["g_sign", "g_no_w", "g_no_s", "g_half", "no_nu", "half_nu"])
def test_every_sign_and_factor_of_the_face_force_is_needed(errors, variant):
    """at n = 65 each wrong variant is at least 3 times further from the derivative than the full H.  Here: G with the
    opposite sign 0.47, G without w 0.032, no s in G_z 0.088, 1 / h_z for 2 / h_z 0.12, no nu term 0.017, half of it
    0.0074, against 0.0017"""
    e = derivative_error(65, variant)
    print(variant, e, errors[65])
    assert e >= 3.0 * errors[65], (variant, e, errors[65])


def noisy_case(ny):
    """the perturbed ABC field on [0,2]^2 x [0,1] with noise of sigma 0.2 on the two transverse components of the lower
    face's interior, and wm = (0.05, 0.05, 1)"""
    mesh = M.box(17, ny)
    exact, b = M.perturbed_abc(mesh)
    nz, nyy, nx = b.shape[1:]
    b[:2, 0, 1:-1, 1:-1] += 0.2 * np.random.default_rng(5).standard_normal((2, nyy - 2, nx - 2))
    wm = np.empty((3, nyy, nx))
    wm[:2], wm[2] = 0.05, 1.0
    return mesh, exact, b, wm


def face_rms(b, exact):
    """rms error of the lower face's transverse field, over the whole plane"""
    return float(np.sqrt(np.mean((b[:2, 0] - exact[:2, 0]) ** 2)))


@pytest.fixture(scope="module")
def fixed_runs():
    out = {}
    for ny in (None, 12):
        mesh, exact, b, wm = noisy_case(ny)
        out[ny] = O.run(mesh, b, None, wm, 0.01, 0, None, niter_max=400, check=50, tol=0.0)
    return out


@pytest.mark.parametrize("ny,nu", [(None, 0.01), (None, 0.1), (12, 0.01), (12, 0.1)],
                         ids=["17x17x9-nu0.01", "17x17x9-nu0.1", "17x12x9-nu0.01", "17x12x9-nu0.1"])
def test_freed_face_descends_where_the_fixed_face_stalls(fixed_runs, ny, nu):
    """400 tries, w = 1.  The model's own run, 17x17x9: the fixed face stops at dt_min after 243 tries, 219 accepted,
    L 3.34 -> 1.98, face error 0.170 unchanged; freed with nu = 0.01: 396 accepted, L 5.5e-4 (3600 times lower), face
    error 0.011 (15 times lower); nu = 0.1: 396, 1.7e-3, 0.0074.  17x12x9: fixed 200 accepted, L 3.17 -> 1.76, face error
    0.165; freed 396, 6.5e-4, 0.011 and 396, 1.8e-3, 0.0072.  These are the figures of the prototype the bounds were set from: 380
    accepted tries, a 500 times lower L, a 4 times lower face error"""
    mesh, exact, b, wm = noisy_case(ny)
    Bf, histf, infof, _ = fixed_runs[ny]
    B, hist, info, trace = O.run(mesh, b, None, wm, nu, 1, None, niter_max=400, check=50, tol=0.0)
    e0, e1 = face_rms(b, exact), face_rms(B, exact)
    print("fixed", histf[0, 1], histf[-1, 1], histf[-1, 6], infof, "freed", hist[-1, 1], hist[-1, 6], "face", e0, e1)
    assert info == (9, 400, 0) and infof[2] == 2
    assert all(x > y for x, y in zip(trace, trace[1:]))           # L falls at every accepted try
    assert len(trace) == 1 + int(hist[-1, 6]) and trace[-1] == hist[-1, 1]
    assert hist[-1, 6] >= 380
    assert hist[-1, 1] <= histf[-1, 1] / 500.0
    assert e1 <= e0 / 4.0 and face_rms(Bf, exact) == e0
    assert np.all(hist[:, 1] == (hist[:, 2] + hist[:, 3]) + nu * hist[:, 4])
    held = np.ones(b.shape[1:], dtype=bool)                       # the rim and the five other faces keep their bits
    held[:-1, 1:-1, 1:-1] = False
    assert np.array_equal(B[:, held].view(np.uint64), b[:, held].view(np.uint64))
    assert not np.array_equal(B[:, 0, 1:-1, 1:-1], b[:, 0, 1:-1, 1:-1])


def small_case():
    mesh = M.box(9)
    exact, b = M.perturbed_abc(mesh)
    _, Y, X = unit(mesh)
    bobs = exact[:, 0] + 0.1 * np.array([np.cos(3.0 * X[0]), np.sin(2.0 * Y[0]), X[0] * Y[0]])
    wm = np.array([0.3 + 0.2 * X[0], 0.25 + 0.2 * Y[0], 1.0 - 0.3 * X[0] * Y[0]])
    return mesh, b, bobs, wm


def test_held_face_and_zero_confidence():
    mesh, b, bobs, wm = small_case()
    # free = 0 with nu = 0 is optimize_model.run bit for bit, whatever bobs and wm hold
    a = M.run(mesh, b, None, niter_max=7, check=3, tol=0.0)
    B, hist, info, trace = O.run(mesh, b, bobs, wm, 0.0, 0, None, niter_max=7, check=3, tol=0.0)
    assert info == a[2] and trace == a[3] and np.array_equal(B.view(np.uint64), a[0].view(np.uint64))
    assert hist[:, [0, 1, 2, 3, 5, 6]].tobytes() == a[1].tobytes() and hist.shape == (4, 7)
    # free = 0: every face bit is kept and L_m is the same in every row; L carries nu L_m
    B, hist, info, _ = O.run(mesh, b, bobs, wm, 0.3, 0, None, niter_max=7, check=3, tol=0.0)
    face = np.ones(b.shape[1:], dtype=bool)
    face[1:-1, 1:-1, 1:-1] = False
    assert np.array_equal(B[:, face].view(np.uint64), b[:, face].view(np.uint64))
    assert np.all(hist[:, 4] == hist[0, 4]) and hist[0, 4] > 0.0
    assert np.all(hist[:, 1] == (hist[:, 2] + hist[:, 3]) + 0.3 * hist[:, 4])
    # wm = 0 with nu > 0: L_m = 0 and the face is still free
    B, hist, info, _ = O.run(mesh, b, bobs, np.zeros_like(wm), 0.3, 1, None, niter_max=7, check=3, tol=0.0)
    assert np.all(hist[:, 4] == 0.0) and hist[-1, 6] > 0
    assert not np.array_equal(B[:, 0, 1:-1, 1:-1], b[:, 0, 1:-1, 1:-1])
    B0, hist0, _, _ = O.run(mesh, b, bobs, wm, 0.0, 1, None, niter_max=7, check=3, tol=0.0)
    assert np.array_equal(B.view(np.uint64), B0.view(np.uint64))            # (the term is absent either way)
    # bobs = None is the lower face of the start field, wm = None is ones
    B1, hist1, _, _ = O.run(mesh, b, None, None, 0.3, 1, None, niter_max=3, check=3, tol=0.0)
    B2, hist2, _, _ = O.run(mesh, b, b[:, 0].copy(), np.ones_like(wm), 0.3, 1, None, niter_max=3, check=3, tol=0.0)
    assert hist1[0, 4] == 0.0 and hist1.tobytes() == hist2.tobytes() and np.array_equal(B1, B2)
    # the sum takes every node of the plane, whatever |B| is
    z = np.zeros_like(b)
    L, Lf, Ld, Lm = O.functional(mesh, z, bobs, wm, 0.3)
    assert Lf == 0.0 and Ld == 0.0 and Lm > 0.0 and L == 0.3 * Lm
    assert Lm == pytest.approx(float(np.sum(O.plane_weights(mesh, b.shape[1:]) * (wm * bobs * bobs).sum(axis=0))), rel=1e-13)


def test_stop_rules_and_history_layout():
    mesh, b, bobs, wm = small_case()
    kw = dict(bobs=bobs, wm=wm, nu=0.1, free=1)
    # niter_max: 7 tries in intervals of 3 - rows at 0, 3, 6, 7
    B, hist, info, _ = O.run(mesh, b, niter_max=7, check=3, tol=0.0, **kw)
    assert info == (4, 7, 0) and hist.shape == (4, 7)
    assert list(hist[:, 0]) == [0.0, 3.0, 6.0, 7.0]
    h2 = min(M.spacing(mesh)) ** 2
    assert hist[0, 5] == 0.1 * h2 and hist[0, 6] == 0.0
    assert hist[-1, 5] == pytest.approx(0.1 * h2 * 1.01 ** hist[-1, 6] * 0.5 ** (7 - hist[-1, 6]), rel=1e-12)
    # rows run out: the last row is overwritten, the final state is last
    B2, hist2, info2, _ = O.run(mesh, b, niter_max=7, check=3, tol=0.0, hist_rows=2, **kw)
    assert info2 == (2, 7, 0) and np.array_equal(hist2, hist[[0, 3]]) and np.array_equal(B2, B)
    # tol: the first check finds a fall of less than 99.9 %
    _, hist, info, _ = O.run(mesh, b, niter_max=50, check=5, tol=0.999, **kw)
    assert info == (2, 5, 1) and hist[1, 0] == 5.0
    # dt_min: a first step far too large is rejected, and half of it is below dt_min
    B, hist, info, trace = O.run(mesh, b, niter_max=50, check=5, dt0=100.0, dt_min=60.0, **kw)
    assert info == (2, 1, 2) and list(hist[1, [0, 5, 6]]) == [1.0, 50.0, 0.0] and len(trace) == 1
    assert np.array_equal(B, b)
    # dt0 below dt_min: no try at all
    _, hist, info, _ = O.run(mesh, b, niter_max=50, check=5, dt0=1.0, dt_min=2.0, **kw)
    assert info == (1, 0, 2) and hist.shape == (1, 7)
    # a step that overflows: inf and NaN in L_T, L_m included - every try rejected, then dt_min
    B, hist, info, _ = O.run(mesh, b, niter_max=40, check=40, tol=0.0, dt0=1e300, **kw)
    assert info == (2, 20, 2) and hist[-1, 6] == 0.0 and np.isfinite(hist).all() and np.array_equal(B, b)


def test_measurement_weight():
    import ndsm_amd
    bobs = np.zeros((3, 2, 3))
    bobs[0] = [[3.0, 0.0, -6.0], [0.0, 0.0, 0.3]]
    bobs[1] = [[4.0, 0.0, 8.0], [0.0, -1.0, 0.4]]
    bobs[2] = [[9.0, -7.0, 0.0], [1.0, 2.0, 3.0]]
    t = np.array([[0.5, 0.0, 1.0], [0.0, 0.1, 0.05]])                 # |B_t| = 5, 0, 10, 0, 1, 0.5 over 10
    wm = ndsm_amd.measurement_weight(bobs)
    assert wm.shape == (3, 2, 3) and np.all(wm[2] == 1.0)
    assert np.allclose(wm[0], t, rtol=1e-15, atol=0.0) and np.array_equal(wm[0], wm[1])
    wm = ndsm_amd.measurement_weight(bobs, floor=0.08)
    assert np.allclose(wm[0], np.maximum(t, 0.08), rtol=1e-15, atol=0.0) and np.array_equal(wm[0], wm[1])
    assert wm[0, 0, 1] == 0.08 and wm[0, 1, 2] == 0.08 and np.all(wm[2] == 1.0)
    # an all-zero transverse field gives the floor
    bobs[:2] = 0.0
    for floor in (0.0, 0.25):
        wm = ndsm_amd.measurement_weight(bobs, floor)
        assert np.all(wm[:2] == floor) and np.all(wm[2] == 1.0) and np.isfinite(wm).all()
    for bad in (dict(floor=-0.1), dict(floor=1.5), dict(floor=float("nan"))):
        with pytest.raises(ValueError):
            ndsm_amd.measurement_weight(bobs, **bad)
    with pytest.raises(ValueError):
        ndsm_amd.measurement_weight(np.zeros((2, 3, 3)))
