"""CPU tests of the numpy model of the weighted restriction and of the cascade of the measurement fit
(tests/obs_cascade_model.py) that do not depend on the model being the device's twin: what the weighted rule promises
(identity, scaling of the confidence, ones against the hat average, faces from faces only, a patch nobody trusts), what
it is for (bad pixels with confidence 0 do not reach the coarse plane), the four pastes, the two anchors, and what the
cascade is for - after the same number of tries on the finest grid the functional and the error of the freed face lie
below the single-level fit's."""
import numpy as np
import pytest

import cascade_model as C
import obs_cascade_model as OC
import optimize_model as M
import optimize_obs_model as O


def rough(shape, ncomp=3, seed=3):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(ncomp,) + tuple(shape)) + 1.5


def conf(shape, ncomp=3, seed=4):
    """confidences in (0, 1]"""
    return 1.0 - np.random.default_rng(seed).uniform(0.0, 1.0, size=(ncomp,) + tuple(shape))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("shape", [(1, 6, 9), (27, 22, 33)], ids=["9x6x1", "33x22x27"])
def test_same_shape_is_the_identity(shape):
    a, w = rough(shape), conf(shape)
    d, wd = OC.resample_weighted(a, w, shape)
    assert same_bits(d, a) and same_bits(wd, w)
    d1, wd1 = OC.resample_weighted(a[0], w[0], shape)
    assert same_bits(d1, a[0]) and same_bits(wd1, w[0])


def test_a_power_of_two_on_the_confidence_scales_it_exactly():
    a, w = rough((9, 8, 11)), conf((9, 8, 11))
    d, wd = OC.resample_weighted(a, w, (5, 4, 5))
    for s in (0.25, 8.0, 2.0 ** -40):
        ds, wds = OC.resample_weighted(a, s * w, (5, 4, 5))
        assert same_bits(ds, d) and same_bits(wds, s * wd), s


def test_ones_give_the_hat_average_to_a_few_ulp():
    """one division by Q instead of one per axis.  Measured with this model on these shapes: 3 ulp at the most in three
    dimensions, 0 on the planes (a 2:1 pair's divisors are powers of two); asserted with a factor 2"""
    worst = 0.0
    for src, dsts in (((27, 22, 33), ((14, 11, 17), (10, 9, 13), (4, 4, 4))), ((1, 6, 9), ((1, 4, 5),)),
                      ((1, 33, 33), ((1, 17, 17),))):
        a = rough(src)
        for dst in dsts:
            d, wd = OC.resample_weighted(a, np.ones_like(a), dst)
            want = C.resample(a, dst, "average")
            assert np.all(wd == 1.0), (src, dst)
            u = float((np.abs(d - want) / np.spacing(np.abs(want))).max())
            print(src, dst, u, "ulp")
            worst = max(worst, u)
    assert worst <= 6.0, worst


def test_faces_come_from_faces_only():
    a, w = rough((27, 22, 33)), conf((27, 22, 33))
    ha, hw = a.copy(), w.copy()
    ha[:, 1:-1, 1:-1, 1:-1] = np.nan
    hw[:, 1:-1, 1:-1, 1:-1] = np.nan
    for dst in ((14, 11, 17), (4, 4, 4)):
        f = C.faces(dst)
        clean, got = OC.resample_weighted(a, w, dst), OC.resample_weighted(ha, hw, dst)
        for x, y in zip(got, clean):
            assert np.isfinite(x[:, f]).all(), dst
            assert same_bits(x[:, f], y[:, f]), dst


def test_a_patch_nobody_trusts_gets_the_plain_average():
    a, w = rough((1, 17, 17)), conf((1, 17, 17))
    w[:, :, 4:11, 2:9] = 0.0                                      # wider than a hat: nodes whose taps are all zero
    d, wd = OC.resample_weighted(a, w, (1, 9, 9))
    plain = OC.resample_weighted(a, np.ones_like(a), (1, 9, 9))[0]
    dead = wd == 0.0
    assert dead[:, 0, 3:5, 2:4].all() and dead.sum() == 3 * 4
    assert same_bits(d[dead], plain[dead])
    assert np.all(wd[~dead] > 0.0) and np.isfinite(d).all()
    # a node with one trusted tap takes that tap's value
    w[:] = 0.0
    w[:, 0, 7, 9] = 0.5
    d, wd = OC.resample_weighted(a, w, (1, 9, 9))
    for j, i in ((3, 4), (3, 5), (4, 4), (4, 5)):                 # the four coarse nodes whose hats reach (7, 9)
        assert np.allclose(d[:, 0, j, i], a[:, 0, 7, 9], rtol=4e-16, atol=0.0)


def test_bad_pixels_without_confidence_do_not_reach_the_coarse_plane():
    """the reason for the rule: a smooth 33 x 33 plane with a checkerboard of pixels replaced by 1e3 and given confidence
    0.  Where the clean pixels of a patch weigh the same - they all do: the clean pixels of a checkerboard are the
    odd-parity taps, which a 1-2-1 x 1-2-1 hat gives the weight 2 each - the weighted result is the restriction of the
    clean plane over those pixels; the hat average is off by hundreds"""
    u = np.linspace(0.0, 1.0, 33)
    Y, X = np.meshgrid(u, u, indexing="ij")
    clean = (1.0 + 0.5 * np.sin(2.0 * X + 0.3) * np.cos(1.5 * Y))[None, None]
    bad = (np.add.outer(np.arange(33), np.arange(33)) % 2 == 0)[None, None]
    bad[..., 0, :] = bad[..., -1, :] = bad[..., :, 0] = bad[..., :, -1] = False      # the rim stays clean
    dirty = np.where(bad, 1e3, clean)
    w = np.where(bad, 0.0, 1.0)
    got, wd = OC.resample_weighted(dirty, w, (1, 17, 17))
    want = OC.resample_weighted(clean, w, (1, 17, 17))[0]         # the clean plane over the trusted pixels
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(got - clean[..., ::2, ::2]).max() < 2e-3        # ... which is the plane itself to O(h^2)
    hat = C.resample(dirty, (1, 17, 17), "average")
    assert np.abs(hat - clean[..., ::2, ::2])[..., 1:-1, 1:-1].min() > 100.0
    assert np.all(wd[..., 1:-1, 1:-1] > 0.0) and np.all(wd <= 1.0)


@pytest.mark.parametrize("shape", [(4, 4, 4), (4, 7, 5)], ids=["4x4x4", "5x7x4"])
def test_the_four_pastes(shape):
    nz, ny, nx = shape
    k0 = np.zeros(shape, dtype=bool)
    k0[0] = True
    freed = np.zeros(shape, dtype=bool)
    freed[0, 1:-1, 1:-1] = True
    assert freed.sum() == (ny - 2) * (nx - 2)
    m = [OC.paste_mask(shape, which) for which in range(4)]
    assert np.array_equal(m[0], k0) and np.array_equal(m[1], C.faces(shape))
    assert np.array_equal(m[2], k0 & ~freed) and np.array_equal(m[3], C.faces(shape) & ~freed)
    assert m[2].sum() == 2 * nx + 2 * ny - 4 and m[3].sum() == C.faces(shape).sum() - freed.sum()
    # what a paste leaves is the complement, bit for bit
    src, dst = rough(shape, seed=5), rough(shape, seed=6)
    for which in range(4):
        out = dst.copy()
        out[:, m[which]] = src[:, m[which]]
        assert same_bits(out[:, ~m[which]], dst[:, ~m[which]]) and same_bits(out[:, m[which]], src[:, m[which]])


def small_levels():
    meshes = [M.box(9), [np.linspace(q[0], q[-1], n) for q, n in zip(M.box(9), (5, 5, 4))]]
    exact, b = M.perturbed_abc(meshes[0])
    u = [(q - q[0]) / (q[-1] - q[0]) for q in meshes[0]]
    Y, X = np.meshgrid(u[1], u[0], indexing="ij")
    bobs = exact[:, 0] + 0.1 * np.array([np.cos(3.0 * X), np.sin(2.0 * Y), X * Y])
    wm = np.array([0.3 + 0.2 * X, 0.25 + 0.2 * Y, 1.0 - 0.3 * X * Y])
    return meshes, b, bobs, wm


def test_anchors():
    meshes, b, bobs, wm = small_levels()
    # a held face with nu = 0 is the plain cascade bit for bit, whatever bobs and wm hold
    a = C.cascade(meshes, b, None, niter_max=[3, 7], check=3, tol=0.0)
    B, hist, info, starts, _, _, _ = OC.cascade_obs(meshes, b, bobs, wm, 0.0, 0, None, niter_max=[3, 7], check=3, tol=0.0)
    assert same_bits(B, a[0]) and info == a[2]
    for l in range(2):
        assert hist[l][:, [0, 1, 2, 3, 5, 6]].tobytes() == a[1][l].tobytes() and same_bits(starts[l], a[3][l])
    # one level is the single-level fit bit for bit
    one = O.run(meshes[0], b, bobs, wm, 0.1, 1, None, niter_max=7, check=3, tol=0.0)
    B, hist, info, starts, traces, _, _ = OC.cascade_obs(meshes[:1], b, bobs, wm, 0.1, 1, None, niter_max=7, check=3, tol=0.0)
    assert same_bits(B, one[0]) and hist[0].tobytes() == one[1].tobytes() and info == [one[2]] and traces == [one[3]]
    # nu per level
    B1 = OC.cascade_obs(meshes, b, bobs, wm, [0.1, 0.0], 1, None, niter_max=[3, 7], check=3, tol=0.0)
    B2 = OC.cascade_obs(meshes, b, bobs, wm, 0.1, 1, None, niter_max=[3, 7], check=3, tol=0.0)
    assert np.all(B1[1][1][:, 1] == B1[1][1][:, 2] + B1[1][1][:, 3]) and not same_bits(B1[0], B2[0])


def noisy_case(n):
    """test_optimize_obs_model's noisy magnetogram on the n box: the perturbed ABC field on [0,2]^2 x [0,1] with noise
    of sigma 0.2 on the two transverse components of the lower face's interior, and wm = (0.05, 0.05, 1)"""
    mesh = M.box(n)
    exact, b = M.perturbed_abc(mesh)
    nz, ny, nx = b.shape[1:]
    b[:2, 0, 1:-1, 1:-1] += 0.2 * np.random.default_rng(5).standard_normal((2, ny - 2, nx - 2))
    wm = np.empty((3, ny, nx))
    wm[:2], wm[2] = 0.05, 1.0
    return mesh, exact, b, wm


def freed_rms(b, exact):
    """rms error of the transverse field on the freed nodes against the noise-free face"""
    return float(np.sqrt(np.mean((b[:2, 0, 1:-1, 1:-1] - exact[:2, 0, 1:-1, 1:-1]) ** 2)))


@pytest.fixture(scope="module")
def benefit():
    """{n: (exact, b, wm, meshes, single-level fit, cascade)} for the finest boxes of 17 and 33 nodes: nu 0.01, free, w = 1,
    100 tries on the finest grid, at most 400 on every coarser one, check 50, tol 0, dt0 = 0.1 min(h)^2 per level"""
    out = {}
    for n, levels in ((17, 2), (33, 3)):
        sizes = [n]
        for _ in range(levels - 1):
            sizes.append((sizes[-1] + 1) // 2)
        meshes = [M.box(s) for s in sizes]
        mesh, exact, b, wm = noisy_case(n)
        single = O.run(mesh, b, None, wm, 0.01, 1, None, niter_max=100, check=50, tol=0.0)
        casc = OC.cascade_obs(meshes, b, None, wm, 0.01, 1, None, niter_max=[100] + [400] * (levels - 1), check=50, tol=0.0)
        out[n] = (exact, b, wm, meshes, single, casc)
    return out


# measured with the committed models (optimize_obs_model.run is the yardstick), after 100 tries on the finest grid:
#   17x17x9,  two levels:   L 7.54e-3 -> 1.32e-3 (5.7 x),  rms of the freed face 0.0307 -> 0.0197 (1.56 x; start 0.193)
#   33x33x17, three levels: L 3.09e-2 -> 6.23e-4 (49.6 x), rms of the freed face 0.0320 -> 0.0086 (3.73 x; start 0.196)
# Each ratio is asserted at one third of the measured one; the 17-box's face ratio is below 3, so there only "not worse"
@pytest.mark.parametrize("n,l_factor,e_factor", [(17, 5.72 / 3.0, 1.0), (33, 49.6 / 3.0, 3.73 / 3.0)])
def test_the_cascade_reaches_further_in_the_same_fine_tries(benefit, n, l_factor, e_factor):
    exact, b, wm, meshes, single, casc = benefit[n]
    l_single, l_casc = single[1][-1, 1], casc[1][0][-1, 1]
    e_single, e_casc = freed_rms(single[0], exact), freed_rms(casc[0], exact)
    print("n %d: L %.4g -> %.4g (%.2f x), freed-face rms %.4g -> %.4g (%.2f x; start %.4g), tries per level %s"
          % (n, l_single, l_casc, l_single / l_casc, e_single, e_casc, e_single / e_casc, freed_rms(b, exact),
             [i[1] for i in casc[2]]))
    assert single[2][1] == 100 and casc[2][0][1] == 100 and all(i[1] <= 400 for i in casc[2][1:])
    assert l_casc <= l_single / l_factor
    assert e_casc <= e_single / e_factor


@pytest.mark.parametrize("n", [17, 33])
def test_every_level_descends_and_holds_what_is_held(benefit, n):
    exact, b, wm, meshes, single, casc = benefit[n]
    B, hist, info, starts, traces, (BO, WM), results = casc
    for l, (tr, h) in enumerate(zip(traces, hist)):
        assert all(x > y for x, y in zip(tr, tr[1:])), l                     # L falls at every accepted try
        assert len(tr) == 1 + int(h[-1, 6]) and tr[-1] == h[-1, 1]
    for l, s in enumerate(starts):
        shape = s.shape[1:]
        g = b if l == 0 else C.resample(b, shape, "average")
        held = OC.paste_mask(shape, 3)                                       # the rim and the five other faces
        assert same_bits(s[:, held], g[:, held]), l
        if l < len(starts) - 1:
            interp = C.resample(results[l + 1], shape, "linear")
            freed = ~held & C.faces(shape)
            assert same_bits(s[:, freed], interp[:, freed]) and not np.array_equal(s[:, freed], g[:, freed]), l
    assert same_bits(B[:, OC.paste_mask(B.shape[1:], 3)], b[:, OC.paste_mask(B.shape[1:], 3)])
    # the level data: the confidences are constants per component, which the weighted rule reproduces exactly
    for l in range(1, len(meshes)):
        assert np.all(WM[l][:2] == 0.05) and np.all(WM[l][2] == 1.0)
        assert BO[l].shape == (3,) + starts[l].shape[2:]

