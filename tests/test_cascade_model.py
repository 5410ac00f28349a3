"""CPU tests of the cascade's numpy model (tests/cascade_model.py) that do not depend on the model being the device's
twin: what the two 1-D rules promise (identity, constants, linear functions, the 1-2-1 weights, faces from faces only),
the shapes rule, and what the cascade is for - after the same number of tries on the finest grid the functional and
the error to the exact field lie far below the single-level run's."""
import numpy as np
import pytest

import cascade_model as C
import optimize_model as M


def rough(shape, ncomp=3, seed=3):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(ncomp,) + tuple(shape)) + 1.5


def test_same_shape_is_the_identity():
    a = rough((27, 22, 33))
    for mode in C.MODES:
        out = C.resample(a, (27, 22, 33), mode)
        assert out.tobytes() == a.tobytes(), mode
        assert C.resample(a[0], (27, 22, 33), mode).tobytes() == a[0].tobytes()


def test_constants_are_exact():
    """a power of two - the weight 1 above all - comes out exactly: fl(1 - theta) + theta rounds to 1 (for theta >= 1/2
    the difference is exact, below it the error is at most a quarter ulp of 1), and the hat's integer weights times a
    power of two are exact.  Any other constant takes the roundings of its products: three per axis at the most"""
    for c, ulps in ((1.0, 0), (-0.25, 0), (4096.0, 0), (0.0, 0), (0.1 + 0.2, 9), (-3.7e5, 9)):
        a = np.full((2, 27, 22, 33), c)
        for mode, shapes in (("linear", ((14, 11, 17), (10, 9, 13), (40, 30, 65), (4, 4, 4))),
                             ("average", ((14, 11, 17), (10, 9, 13), (4, 4, 4)))):
            for s in shapes:
                out = C.resample(a, s, mode)
                assert out.shape == (2,) + s
                assert np.abs(out - c).max() <= ulps * np.spacing(abs(c)), (c, mode, s)


def test_linear_functions_are_reproduced():
    def lin(shape):
        u = [np.linspace(0.0, 1.0, n) for n in shape]
        Z, Y, X = np.meshgrid(*u, indexing="ij")
        return 0.3 + 1.7 * X - 0.9 * Y + 0.45 * Z
    got = C.resample(lin((4, 5, 3)), (5, 9, 65), "linear")
    assert np.abs(got - lin((5, 9, 65))).max() < 1e-15


def test_full_weighting_for_a_nested_pair():
    for f in range(9):
        e = np.zeros((1, 1, 9))
        e[0, 0, f] = 4.0
        out = C.resample(e, (1, 1, 5), "average")[0, 0]
        want = np.zeros(5)
        if f in (0, 8):
            want[f // 2] = 4.0                          # the end nodes are copied ...
        elif f % 2 == 0:
            want[f // 2] = 2.0                          # ... an interior coarse node takes 1-2-1 over four
        else:
            for i in (f // 2, f // 2 + 1):
                if 0 < i < 4:
                    want[i] = 1.0                       # (the end nodes take nothing from their neighbours)
        assert np.array_equal(out, want), (f, out, want)
    assert C.taps(2, 9, 5, "average") == ([(3, 4), (4, 8), (5, 4)], 16, None)
    assert C.taps(1, 9, 5, "linear") == ([(2, None)], None, None)
    assert C.taps(1, 5, 9, "linear") == ([(0, None), (1, None)], None, 0.5)


@pytest.mark.parametrize("mode", C.MODES)
def test_faces_come_from_faces_only(mode):
    a = rough((27, 22, 33))
    holed = a.copy()
    holed[:, 1:-1, 1:-1, 1:-1] = np.nan
    for dst in ((14, 11, 17), (10, 9, 13), (4, 4, 4)):
        f = C.faces(dst)
        clean, got = C.resample(a, dst, mode), C.resample(holed, dst, mode)
        assert np.isfinite(got[:, f]).all(), dst
        assert got[:, f].tobytes() == clean[:, f].tobytes(), dst


def test_the_average_cannot_refine_and_axes_need_two_nodes():
    a = rough((4, 5, 6), 1)[0]
    for dst in ((4, 5, 7), (5, 5, 6), (4, 6, 6)):
        with pytest.raises(ValueError):
            C.resample(a, dst, "average")
    for mode in C.MODES:
        with pytest.raises(ValueError):
            C.resample(a, (4, 1, 6), mode)
        assert C.resample(a[:1], (1, 3, 4), mode).shape == (1, 3, 4)        # a plane stays a plane


def test_cascade_shapes():
    import ndsm_amd
    for fn in (C.cascade_shapes, ndsm_amd.cascade_shapes):
        assert fn((17, 33, 33), 3) == [(17, 33, 33), (9, 17, 17), (5, 9, 9)]
        assert fn((32, 9, 33), 2) == [(32, 9, 33), (16, 5, 17)]
        assert fn((5, 33, 33), 3) == [(5, 33, 33), (5, 17, 17), (5, 9, 9)]   # (5 + 1) // 2 = 3 < min_nodes: pinned
        assert fn((5, 33, 33), 2, min_nodes=3) == [(5, 33, 33), (3, 17, 17)]
        assert fn((6, 6, 5), 1) == [(6, 6, 5)]
        with pytest.raises(ValueError):
            fn((6, 6, 5), 2)
        with pytest.raises(ValueError):
            fn((9, 9, 9), 3)


def start_field(mesh):
    exact = M.abc_field(mesh)
    b = exact.copy()
    g = M.bump(mesh, 1)
    for c, a in enumerate((1.0, 0.7, -0.5)):
        b[c] += a * g
    return exact, b


@pytest.fixture(scope="module")
def benefit():
    """{n: (single-level run, cascade)} for the finest boxes of 17 and 33 nodes: 100 tries on the finest grid, at
    most 400 on every coarser one, check 50, tol 0"""
    out = {}
    for n, levels in ((17, 2), (33, 3)):
        sizes = [n]
        for _ in range(levels - 1):
            sizes.append((sizes[-1] + 1) // 2)
        meshes = [M.box(s) for s in sizes]
        exact, b = start_field(meshes[0])
        single = M.run(meshes[0], b, None, niter_max=100, check=50, tol=0.0)
        casc = C.cascade(meshes, b, None, niter_max=[100] + [400] * (levels - 1), check=50, tol=0.0)
        out[n] = (exact, b, single, casc)
    return out


@pytest.mark.parametrize("n,factor", [(17, 30.0), (33, 1000.0)])
def test_the_cascade_reaches_further_in_the_same_fine_tries(benefit, n, factor):
    """measured with this model: 17x17x9, two levels: L 4.5e-2 -> 3.5e-4 (128 x), max error 0.167 -> 8.8e-3;
    33x33x17, three levels: L 1.73 -> 3.4e-4 (5100 x), max error 0.504 -> 7.0e-3.  The bounds are about a quarter of
    the measured gain in L and a quarter of the single level's error"""
    exact, b, single, casc = benefit[n]
    l_single, l_casc = single[1][-1, 1], casc[1][0][-1, 1]
    e_single, e_casc = np.abs(single[0] - exact).max(), np.abs(casc[0] - exact).max()
    print("n %d: L %.4g -> %.4g (%.0f x), max error %.4g -> %.4g, tries per level %s"
          % (n, l_single, l_casc, l_single / l_casc, e_single, e_casc, [i[1] for i in casc[2]]))
    assert single[2][1] == 100 and casc[2][0][1] == 100
    assert l_casc <= l_single / factor
    assert e_casc < 0.25 * e_single


@pytest.mark.parametrize("n", [17, 33])
def test_every_finer_level_starts_lower_and_keeps_the_faces(benefit, n):
    exact, b, single, casc = benefit[n]
    B, hist, info, starts = casc
    for l in range(len(hist) - 2, -1, -1):
        assert hist[l][0, 1] < hist[l + 1][0, 1], (l, hist[l][0, 1], hist[l + 1][0, 1])
    f = C.faces(b.shape[1:])
    assert B[:, f].tobytes() == b[:, f].tobytes()
    for l, s in enumerate(starts[:-1]):                  # every finer level's start carries its own average's faces
        g = C.resample(b, s.shape[1:], "average")
        fl = C.faces(s.shape[1:])
        assert s[:, fl].tobytes() == g[:, fl].tobytes(), l
