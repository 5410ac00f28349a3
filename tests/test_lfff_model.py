"""CPU tests of tests/lfff_model.py, the numpy restatement of the constant-alpha force-free field of a magnetogram
(semantics: include/ndsm_hip.h, ndsm_hip_lfff_points): the single-pixel sum against Chiu & Hilton's closed form,
alpha = 0 against the Green's-function model bit for bit, the mirror rule of alpha's sign, curl B = alpha B and
div B = 0 by central differences, the same on a box mesh as a function of h, the refinement of the source, and
best_alpha on a field whose alpha is known.

Measured with this model (DESIGN.md section 35 holds the same figures):

    single pixel against the closed form, 200 points, alpha 0.5, 2, -2, 7: 1.26e-15 of max |G|
    curl and div by central differences, step 1e-4, of max |B|: alpha 0.5: 1.02e-6, 7.68e-7; 2: 7.53e-7, 5.54e-7;
        -2: 7.93e-7, 5.89e-7
    grid property, alpha = 1.5 (max |curl_h B - alpha B| over the interior nodes with z >= 0.375, over max |B| on all
        interior nodes): n = 17: 7.267e-2, n = 33: 1.470e-2, factor 4.94; the potential field at n = 17: 0.648
    refinement, gaps 13^2 -> 25^2 -> 49^2 -> 97^2 over max |B| at the four points: 0.571, 6.29e-2, 7.31e-3
        (factors 9.1 and 8.6; the points of this file, the lowest at z = 0.125 = a quarter of the coarsest spacing)
    best_alpha on the ABC field, |alpha - pi|: n = 17: 1.31e-2, 33: 4.13e-3, 65: 1.15e-3 (factors 3.17, 3.61: the
        one-sided differences of the edge rows weigh more on the coarse meshes)"""
import functools

import numpy as np
import pytest

import green_model as gm
import lfff_model as lm

EPS = np.finfo(float).eps


def test_single_pixel_is_the_closed_form():
    """one pixel of weight q = bz c: the sums are q 2 pi G(dx, dy, w), G the closed form.  Bound: every addend is a
    product of fewer than 8 rounded factors, so the gap stays below 8 eps M, M the model's own sum of absolute
    products; printed as well relative to |G|"""
    xs, ys = np.array([0.0, 0.5, 1.0, 1.5]), np.array([-1.0, -0.75, -0.5])
    bz = np.zeros((3, 4))
    bz[1, 2] = 3.0                                          # the pixel at (1.0, -0.75)
    rng = np.random.default_rng(3)
    n = 200
    X, Y, Z = 1.0 + rng.uniform(-2.0, 2.0, n), -0.75 + rng.uniform(-2.0, 2.0, n), 0.125 + rng.uniform(0.05, 2.0, n)
    worst = 0.0
    for alpha in (0.5, 2.0, -2.0, 7.0):
        out, mag = lm.lfff_sums(xs, ys, 0.125, bz, alpha, X, Y, Z, with_abs=True)
        want = 3.0 * (0.5 * 0.25) * lm.closed_form(alpha, X - 1.0, Y + 0.75, Z - 0.125)
        assert (np.abs(out - want) <= 8 * EPS * mag).all(), alpha
        worst = max(worst, (np.abs(out - want).max(axis=0) / np.abs(want).max(axis=0)).max())
    print("single pixel against the closed form: %.3g relative to max |G|" % worst)
    # a target on the pixel itself, on the plane: the punctured rule leaves the pixel out
    on = lm.lfff_targets(xs, ys, 0.125, bz, 2.0, [1.0], [-0.75], [0.125])
    assert on[0, 0] == 0.0 and on[1, 0] == 0.0 and on[2, 0] == 3.0
    # straight above it: only the first three terms, nothing divides by R
    up = lm.lfff_sums(xs, ys, 0.125, bz, 2.0, [1.0], [-0.75], [0.625])
    q, w = 3.0 * ((0.5 * 0.25) / gm.TWO_PI), 0.5
    assert up[0, 0] == 0.0 and up[1, 0] == 0.0
    assert up[2, 0] == (w * (q / (w * w * w))) * (np.cos(2.0 * w) + (2.0 * w) * np.sin(2.0 * w))


def rough_source(nsx=17, nsy=15, seed=5):
    rng = np.random.default_rng(seed)
    xs, ys = 0.37 + 0.013 * np.arange(nsx), -1.21 + 0.017 * np.arange(nsy)
    return xs, ys, 0.25, rng.uniform(-1.0, 1.0, size=(nsy, nsx)) + 0.3


def test_alpha_zero_is_the_green_model_bit_for_bit():
    xs, ys, zs, bz = rough_source()
    lx, ly = xs[-1] - xs[0], ys[-1] - ys[0]
    P = np.array([(xs[3], ys[4], zs),                                  # on the plane at a node
                  (xs[0] + 0.31 * lx, ys[0] + 0.77 * ly, zs),          # on it off the nodes
                  (xs[16], ys[14], zs),                                # the last node
                  (xs[5], ys[2], zs + 0.2),                            # straight above a node
                  (xs[5], ys[0] + 0.4 * ly, zs + 0.01),                # above a column of nodes (dx == 0, dy != 0)
                  (xs[0] + 0.6 * lx, ys[0] + 0.2 * ly, zs + 0.3),      # above the plane
                  (xs[-1] + 0.5, ys[0] - 0.2, zs + 0.1),               # outside the source
                  (xs[0] - 0.3, ys[3], zs),                            # outside it, on the plane
                  (xs[4], ys[4], zs - 0.1)])                           # below the plane
    for src in ((xs, ys, bz), (xs[:2], ys[:2], bz[:2, :2])):
        got = lm.lfff_sums(src[0], src[1], zs, src[2], 0.0, P[:, 0], P[:, 1], P[:, 2])
        want = gm.green_sums(src[0], src[1], zs, src[2], P[:, 0], P[:, 1], P[:, 2])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    got, want = lm.lfff_points(xs, ys, zs, bz, 0.0, P), gm.green_points(xs, ys, zs, bz, P)
    assert np.isnan(want[-1]).all() and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[:-1].view(np.uint64), want[:-1].view(np.uint64))
    # more than one slice
    xs2, ys2 = 0.1 * np.arange(65), 0.1 * np.arange(64)
    bz2 = np.random.default_rng(1).uniform(-1, 1, (64, 65))
    T = (np.array([xs2[7], 1.234, 9.0]), np.array([ys2[60], 2.345, -1.0]), np.array([0.3, 0.0, 0.2]))
    assert np.array_equal(lm.lfff_sums(xs2, ys2, 0.0, bz2, 0.0, *T).view(np.uint64),
                          gm.green_sums(xs2, ys2, 0.0, bz2, *T).view(np.uint64))


def test_the_sign_of_alpha_flips_as_the_mirror_image_does():
    """(x, Bx) <-> (-x, -Bx) with alpha <-> -alpha for the mirrored source.  The mirror reverses the order of the pixels
    of a row, so the sums agree to the rounding of the accumulation: 2 npix eps M at the very most"""
    rng = np.random.default_rng(11)
    xs, ys = 0.125 * np.arange(-6, 7), 0.2 * np.arange(-3, 4)
    bz = rng.uniform(-1.0, 1.0, (7, 13))
    X, Y, Z = rng.uniform(-1.0, 1.0, 30), rng.uniform(-1.0, 1.0, 30), rng.uniform(0.05, 1.0, 30)
    for alpha in (0.7, -3.0):
        a, mag = lm.lfff_sums(xs, ys, 0.0, bz, alpha, X, Y, Z, with_abs=True)
        b = lm.lfff_sums(xs, ys, 0.0, bz[:, ::-1], -alpha, -X, Y, Z)
        b[0] = -b[0]
        assert (np.abs(a - b) <= 2 * bz.size * EPS * mag).all()
        c = lm.lfff_sums(xs, ys, 0.0, bz[:, ::-1], alpha, -X, Y, Z)        # without the flip of alpha: off at order alpha
        c[0] = -c[0]
        assert np.abs(a - c).max() > 0.05 * np.abs(a).max()


def gauss_source(m, h, width=0.3):
    xs = np.arange(-m, m + 1) * h
    Ys, Xs = np.meshgrid(xs, xs, indexing="ij")
    return xs, xs, lm.gauss_pair(Xs, Ys, width)


def curl_div_at(xs, ys, bz, alpha, P, d=1e-4):
    """curl B, div B and B at the points P (n,3) by central differences with step d through the model's points
    function (one call for the 6 n shifted points)"""
    n = len(P)
    Q = np.concatenate([P + s * d * np.eye(3)[a] for a in range(3) for s in (1, -1)] + [P])
    F = lm.lfff_points(xs, ys, 0.0, bz, alpha, Q)
    D = [(F[2 * a * n:(2 * a + 1) * n] - F[(2 * a + 1) * n:(2 * a + 2) * n]) / (2 * d) for a in range(3)]   # D[a][:, c]
    curl = np.array([D[1][:, 2] - D[2][:, 1], D[2][:, 0] - D[0][:, 2], D[0][:, 1] - D[1][:, 0]]).T
    return curl, D[0][:, 0] + D[1][:, 1] + D[2][:, 2], F[6 * n:]


@pytest.mark.parametrize("alpha", (0.5, 2.0, -2.0))
def test_curl_is_alpha_b_and_div_is_zero(alpha):
    """the sum is a finite sum of exact solutions, so the residual is the differences' own: O(d^2) truncation and
    eps / d rounding, 1.8e-6 of max |B| at the most as measured; a wrong sign or a missing term shows at order alpha"""
    h = 0.125
    xs, ys, bz = gauss_source(8, h)                         # 17 x 17 on [-1, 1]^2
    rng = np.random.default_rng(7)
    P = np.array([rng.uniform(-1.0, 1.0, 20), rng.uniform(-1.0, 1.0, 20), rng.uniform(h / 2, 1.0, 20)]).T
    curl, div, B = curl_div_at(xs, ys, bz, alpha, P)
    scale = np.abs(B).max()
    res, dres = np.abs(curl - alpha * B).max() / scale, np.abs(div).max() / scale
    print("alpha %g: |curl B - alpha B| %.3g, |div B| %.3g, |alpha B| %.3g of max |B|"
          % (alpha, res, dres, np.abs(alpha * B).max() / scale))
    assert res < 1e-4 and dres < 1e-4
    assert np.abs(curl + alpha * B).max() / scale > 0.1     # (the other sign is far off)


def curl_h(b, x, y, z):
    g = lambda c, ax, q: np.gradient(b[c], q, axis=ax, edge_order=2)   # noqa: E731   (axes: 0 z, 1 y, 2 x)
    return np.array([g(2, 1, y) - g(1, 0, z), g(0, 0, z) - g(2, 2, x), g(1, 2, x) - g(0, 1, y)])


@functools.lru_cache(maxsize=None)
def grid_residual(n, alpha_field, alpha=1.5):
    """max |curl_h B - alpha B| over the interior nodes with z >= 0.375, over max |B| on all interior nodes, of the box
    x = y = linspace(-1, 1, n), z = arange((n + 1) // 2) h under the source arange(-m, m + 1) h, m = round(3 / h); B
    with alpha_field.  (The plane z = 0 holds no interior node and no difference looked at reaches it: left out.)"""
    x = np.linspace(-1.0, 1.0, n)
    h = x[1] - x[0]
    z = np.arange((n + 1) // 2) * h
    xs, ys, bz = gauss_source(int(round(3 / h)), h)
    assert np.array_equal(xs[(len(xs) - n) // 2:(len(xs) + n) // 2], x)      # box nodes are source nodes bit for bit
    k0 = int(np.searchsorted(z, 0.375))
    assert k0 >= 3 and z[k0] >= 0.375 > z[k0 - 1]
    b = lm.lfff_box(x, x, z[1:], bz, alpha_field, xs, ys, 0.0)
    res = curl_h(b, x, x, z[1:]) - alpha * b
    return np.abs(res[:, k0 - 1:-1, 1:-1, 1:-1]).max() / np.abs(b[:, :-1, 1:-1, 1:-1]).max()


def test_grid_residual_falls_as_h_squared():
    r17, r33 = grid_residual(17, 1.5), grid_residual(33, 1.5)
    print("grid property: %.4g at n = 17, %.4g at n = 33, factor %.3g" % (r17, r33, r17 / r33))
    assert 3.5 < r17 / r33 < 6.0


def test_the_potential_field_fails_the_grid_check_at_order_alpha():
    r17 = grid_residual(17, 0.0)
    print("the potential field in the same check: %.4g at n = 17" % r17)
    # curl B = 0: the residual is alpha B itself, alpha = 1.5 times the share of max |B| that is left at z >= 0.375
    assert r17 > 0.3 and r17 > 4 * grid_residual(17, 1.5)


def test_refinement_of_the_source():
    P = np.array([(0.21, 0.13, 0.125), (-0.47, 0.29, 0.25), (0.53, -0.61, 0.5), (-0.11, -0.35, 1.0)])
    fields = []
    for n in (13, 25, 49, 97):
        xs = np.linspace(-3.0, 3.0, n)
        Ys, Xs = np.meshgrid(xs, xs, indexing="ij")
        fields.append(lm.lfff_points(xs, xs, 0.0, lm.gauss_pair(Xs, Ys, 0.5), 1.0, P))
    scale = np.abs(fields[-1]).max()
    gaps = [np.abs(a - b).max() / scale for a, b in zip(fields, fields[1:])]
    print("refinement: gaps %s of max |B|" % ", ".join("%.3g" % g for g in gaps))
    assert gaps[0] >= 4 * gaps[1] and gaps[1] >= 4 * gaps[2]


def test_best_alpha_of_the_abc_field():
    import ndsm_amd
    errs = []
    for n in (17, 33, 65):
        x = np.linspace(0.0, 1.0, n)
        Z, Y, X = np.meshgrid(x[:2], x, x, indexing="ij")
        k = np.pi
        b = np.stack([np.sin(k * Z) + np.cos(k * Y), np.sin(k * X) + np.cos(k * Z), np.sin(k * Y) + np.cos(k * X)])
        errs.append(abs(ndsm_amd.best_alpha(x, x, b) - np.pi))
    print("best_alpha on the ABC field: errors %s, factors %.3g, %.3g"
          % (", ".join("%.3g" % e for e in errs), errs[0] / errs[1], errs[1] / errs[2]))
    assert errs[0] < 0.1
    assert 3.0 < errs[0] / errs[1] < 5.0 and 3.0 < errs[1] / errs[2] < 5.0
    # bz_min leaves pixels out; where none is left alpha is undefined
    x = np.linspace(0.0, 1.0, 17)
    Z, Y, X = np.meshgrid(x[:2], x, x, indexing="ij")
    b = np.stack([np.sin(np.pi * Z) + np.cos(np.pi * Y), np.sin(np.pi * X) + np.cos(np.pi * Z),
                  np.sin(np.pi * Y) + np.cos(np.pi * X)])
    a0, a1 = ndsm_amd.best_alpha(x, x, b), ndsm_amd.best_alpha(x, x, b, bz_min=1.0)
    assert a0 != a1 and abs(a1 - np.pi) < 0.1
    with pytest.raises(ValueError):
        ndsm_amd.best_alpha(x, x, b, bz_min=10.0)
