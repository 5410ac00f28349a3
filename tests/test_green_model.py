"""CPU tests of tests/green_model.py, the numpy restatement of the Green's-function field of a magnetogram (semantics:
include/ndsm_hip.h, ndsm_hip_green_points): the single-pixel formula, the slice rule, the rules of the plane,
linearity, the accuracy of the point rule against an analytic field row by row, and end to end - the port oracle fed
with the model's faces against the same oracle fed with the analytic field's own faces.

Measured with this model (max |dB| over the side face x = 1, Bx and By, over max |B| there; fov = 6):

    n    row 0 (z = 0)   row 1      rows >= 2
    9    1.587e-1        3.664e-3   1.231e-3
    17   7.983e-2        7.474e-4   3.348e-5
    33   4.015e-2        3.934e-4   3.439e-5   (the truncation of the magnetogram)

row 0 falls by 1.988 and 1.989 per halving of h.  End to end (interior max |B - B_analytic| / max |B_analytic|, the
error of the 7-point solve itself): n = 17, fov 3: 7.326e-2 (exact faces 7.333e-2); n = 33, fov 3: 2.850e-2
(2.851e-2); fov 1: 7.374e-2 and 2.876e-2."""
import numpy as np
import pytest

import green_model as gm


def test_single_pixel_is_the_point_formula():
    xs, ys = np.array([0.0, 0.5, 1.0, 1.5]), np.array([-1.0, -0.75, -0.5])
    bz = np.zeros((3, 4))
    bz[1, 2] = 3.0                                          # the pixel at (1.0, -0.75)
    X, Y, Z = np.array([0.3, 1.0, -2.0]), np.array([0.2, -0.75, 5.0]), np.array([0.7, 0.25, 1.0])
    out = gm.green_sums(xs, ys, 0.125, bz, X, Y, Z)
    q = 3.0 * ((0.5 * 0.25) / gm.TWO_PI)
    dx, dy, w = X - 1.0, Y - (-0.75), Z - 0.125
    r2 = (dx * dx + dy * dy) + w * w
    t = q / (r2 * np.sqrt(r2))
    assert np.array_equal(out, np.array([dx * t, dy * t, w * t]))
    # a target on the pixel itself, on the plane: the punctured rule leaves the pixel out
    on = gm.green_targets(xs, ys, 0.125, bz, [1.0], [-0.75], [0.125])
    assert on[0, 0] == 0.0 and on[1, 0] == 0.0 and on[2, 0] == 3.0


@pytest.mark.parametrize("npix", [4, 4095, 4096, 4097, 8192, 8193, 64 * 4096, 64 * 4096 + 1, 513 * 512])
def test_slice_rule(npix):
    ns, ln = gm.slices(npix)
    assert ns == min(64, -(-npix // 4096)) and ln == -(-npix // ns)
    r = gm.slice_ranges(npix)
    assert len(r) == ns and r[0][0] == 0 and r[-1][1] == npix
    assert all(hi > lo for lo, hi in r)                                   # no slice is empty
    assert all(r[s][1] == r[s + 1][0] for s in range(ns - 1))             # every pixel in exactly one slice
    assert {4095: 1, 4096: 1, 4097: 2, 64 * 4096 + 1: 64}.get(npix, ns) == ns


def test_two_slices_are_folded_in_order():
    """65 x 64 pixels are two slices: the sum is (slice 0) + (slice 1), each left to right - not one long sum"""
    rng = np.random.default_rng(5)
    xs, ys = np.arange(65) * 0.01, np.arange(64) * 0.01
    bz = rng.standard_normal((64, 65))
    X, Y, Z = rng.uniform(0, 0.6, 7), rng.uniform(0, 0.6, 7), rng.uniform(0.01, 0.3, 7)
    got = gm.green_sums(xs, ys, 0.0, bz, X, Y, Z)
    (lo0, hi0), (lo1, hi1) = gm.slice_ranges(65 * 64)
    c = ((xs[1] - xs[0]) * (ys[1] - ys[0])) / gm.TWO_PI
    flat = bz.reshape(-1)
    parts = []
    for lo, hi in ((lo0, hi0), (lo1, hi1)):
        acc = np.zeros((3, 7))
        for p in range(lo, hi):
            dx, dy = X - xs[p % 65], Y - ys[p // 65]
            r2 = (dx * dx + dy * dy) + Z * Z
            t = (flat[p] * c) / (r2 * np.sqrt(r2))
            acc = acc + np.array([dx * t, dy * t, Z * t])
        parts.append(acc)
    assert np.array_equal(got, parts[0] + parts[1])


def test_bz_on_the_plane():
    rng = np.random.default_rng(11)
    xs, ys = np.linspace(-1.3, 0.9, 12), 0.25 + np.arange(7) * 0.3
    bz = rng.standard_normal((7, 12))
    bz[2, 3], bz[6, 11] = -0.0, np.inf
    Yg, Xg = np.meshgrid(ys, xs, indexing="ij")
    with np.errstate(all="ignore"):
        on = gm.plane_bz(xs, ys, bz, Xg, Yg)
    assert np.array_equal(on.view(np.int64), bz.view(np.int64))            # every node: that pixel, bit for bit
    # off the nodes: bilinear, and 0 outside the mesh
    mid = gm.plane_bz(xs, ys, bz, 0.5 * (xs[4] + xs[5]), ys[1] + 0.25 * (ys[2] - ys[1]))
    want = 0.75 * 0.5 * (bz[1, 4] + bz[1, 5]) + 0.25 * 0.5 * (bz[2, 4] + bz[2, 5])
    assert abs(mid - want) < 1e-13
    out = gm.plane_bz(xs, ys, bz, np.array([xs[0] - 1e-9, xs[-1] + 1e-9, 0.0, 0.0]), np.array([1.0, 1.0, ys[0] - 1e-9, 9.0]))
    assert np.array_equal(out, np.zeros(4))
    # through green_targets: w == 0 takes it, w > 0 the sum, w < 0 NaN
    t = gm.green_targets(xs, ys, 0.5, np.where(np.isfinite(bz), bz, 1.0), [xs[3]] * 3, [ys[2]] * 3, [0.5, 0.6, 0.4])
    assert t[2, 0] == 0.0 and np.signbit(t[2, 0]) and np.isfinite(t[:, 1]).all() and np.isnan(t[:, 2]).all()


def test_linear_in_bz_for_a_power_of_two():
    rng = np.random.default_rng(3)
    xs, ys = np.arange(70) * 0.02, np.arange(61) * 0.02 - 0.3
    bz = rng.standard_normal((61, 70))
    X, Y = rng.uniform(-0.2, 1.6, 9), rng.uniform(-0.5, 1.1, 9)
    Z = np.array([0.0, 0.0, 0.02, 0.04, 0.3, 1.0, 0.0, 0.5, 2.0])
    X[0], Y[0] = xs[7], ys[5]
    a = gm.green_targets(xs, ys, 0.0, bz, X, Y, Z)
    for f in (0.25, -8.0):
        assert np.array_equal(gm.green_targets(xs, ys, 0.0, f * bz, X, Y, Z), f * a)


def side_face_errors(n, fov=6):
    """(row 0, row 1, rows >= 2): max |dB| over the side face x = 1, Bx and By, over max |B| on that face"""
    x = np.linspace(-1.0, 1.0, n)
    h = x[1] - x[0]
    z = np.arange((n + 1) // 2) * h
    m = int(round(fov / h))
    xs = np.arange(-m, m + 1) * h
    Ys, Xs = np.meshgrid(xs, xs, indexing="ij")
    bz = gm.monopole_pair(Xs, Ys, 0.0)[2]
    Zg, Yg = np.meshgrid(z, x, indexing="ij")
    got = gm.green_targets(xs, xs, 0.0, bz, np.full(Yg.size, x[-1]), Yg.reshape(-1), Zg.reshape(-1))[:2]
    want = gm.monopole_pair(x[-1], Yg, Zg)[:2]
    err = np.abs(got.reshape(want.shape) - want).max(axis=(0, 2)) / np.abs(want).max()
    return err[0], err[1], err[2:].max()


@pytest.fixture(scope="module")
def face_errors():
    e = {n: side_face_errors(n) for n in (9, 17, 33)}
    for n, v in e.items():
        print("side face n=%d: row 0 %.3e  row 1 %.3e  rows >= 2 %.3e" % ((n,) + v))
    return e


def test_accuracy_against_the_monopole_pair(face_errors):
    e = face_errors
    for coarse, fine in ((9, 17), (17, 33)):
        ratio = e[coarse][0] / e[fine][0]
        print("row 0 falls by %.3f from n=%d to n=%d" % (ratio, coarse, fine))
        assert 1.7 < ratio < 2.3                      # the point rule is first order on the plane row
    assert e[17][2] < 1e-4
    assert e[17][1] < 2e-3


def open_box_case(n, fov):
    x = np.linspace(-1.0, 1.0, n)
    h = x[1] - x[0]
    z = np.arange((n + 1) // 2) * h
    m = int(round(fov / h))
    xs = np.arange(-m, m + 1) * h
    Ys, Xs = np.meshgrid(xs, xs, indexing="ij")
    bz = gm.monopole_pair(Xs, Ys, 0.0)[2]
    Zg, Yg, Xg = np.meshgrid(z, x, x, indexing="ij")
    return x, z, xs, bz, gm.monopole_pair(Xg, Yg, Zg)


def interior_error(port, x, z, faces, exact):
    ierr, A, B, _, _ = port.vector_potential(x, x, z, faces)
    assert ierr == 0
    inner = (slice(None), slice(1, -1), slice(1, -1), slice(1, -1))
    return np.abs(B[inner] - exact[inner]).max() / np.abs(exact[inner]).max()


@pytest.mark.parametrize("n", [17, 33])
def test_open_box_end_to_end(port, n):
    """the oracle fed with the model's faces is as good as the oracle fed with the exact faces: at most 1.05 times its
    interior error (the 5 % covers the Green's-function faces' own error, far smaller by the table above)"""
    x, z, xs, bz, exact = open_box_case(n, 3)
    assert z[0] == 0.0
    faces = gm.green_box(x, x, z, bz, xs=xs, ys=xs, zs=0.0)
    assert np.allclose(faces[2, 0], exact[2, 0], rtol=0.0, atol=1e-12)   # the k = 0 plane's Bz is the magnetogram
    e_open = interior_error(port, x, z, faces, exact)
    e_exact = interior_error(port, x, z, np.where(gm.face_mask(exact.shape[1:]), exact, 0.0), exact)
    print("n=%d fov=3: model faces %.4e  exact faces %.4e" % (n, e_open, e_exact))
    assert e_open <= 1.05 * e_exact
    # a magnetogram no wider than the box: worse side faces, measured and not asserted
    x, z, xs, bz, exact = open_box_case(n, 1)
    e_narrow = interior_error(port, x, z, gm.green_box(x, x, z, bz, xs=xs, ys=xs, zs=0.0), exact)
    print("n=%d fov=1: model faces %.4e" % (n, e_narrow))
