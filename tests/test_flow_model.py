"""CPU tests of what the flow tests rest on (flow_model.py): the numpy restatements of ndsm_hip_flow_fit,
ndsm_hip_green_ap_points / _plane and ndsm_hip_flow_flux pass the closed-form checks that test_gpu_flow.py runs with the
library, and their own pieces - the difference quotients, the window's clipping, the slices, the reduction's order -
are what include/ndsm_hip.h says."""
import numpy as np
import pytest

import flow_model as fm


@pytest.mark.parametrize("n,h,r", fm.RECOVERY, ids=lambda v: str(v).replace(" ", ""))
def test_model_recovers_an_affine_flow(n, h, r):
    err = fm.check_recovery(fm.fit_model, n, h, r, fm.recovery_tol(r))
    assert err >= 0.05 * fm.RECOVERY_SEEN[r], "the recorded figure is stale"       # (the tolerance stays ten times it)


def test_model_rank_deficiency():
    fm.check_rank_deficient(fm.fit_model)


def test_model_bad_values():
    fm.check_bad_values(fm.fit_model)


def test_model_single_pixel_vector_potential():
    fm.check_single_pixel(fm.ap_model)


def test_model_gaussian_vector_potential():
    fm.check_gaussian(fm.ap_model)


def test_model_fluxes():
    fm.check_aligned_flow(fm.flux_model)
    fm.check_uniform_totals(fm.flux_model)


def test_quotients_are_centred_inside_and_one_sided_on_the_end_rows():
    rng = np.random.default_rng(3)
    v = rng.uniform(-1.0, 1.0, (5, 6))
    h = 0.37
    dx, dy = fm.ddq2(v, 1, h), fm.ddq2(v, 0, h)
    assert np.allclose(dx[:, 1:-1], (v[:, 2:] - v[:, :-2]) / (2 * h), rtol=1e-14)
    assert np.allclose(dx[:, 0], (-1.5 * v[:, 0] + 2 * v[:, 1] - 0.5 * v[:, 2]) / h, rtol=1e-13)
    assert np.allclose(dy[-1], (1.5 * v[-1] - 2 * v[-2] + 0.5 * v[-3]) / h, rtol=1e-13)
    quad = np.arange(6.0) ** 2
    assert np.allclose(fm.ddq2(quad[None, :].repeat(3, 0), 1, 1.0), 2 * np.arange(6.0)[None, :])   # exact on quadratics


def test_model_windows_are_clipped():
    fm.check_clipping(fm.fit_model)


def test_model_pivot_rule_is_strict():
    fm.check_pivot_rule(fm.fit_model)


def test_model_zero_pivot_is_rank_deficient():
    fm.check_zero_pivot(fm.fit_model)
    # the pivot the check predicts, in the restatement: exactly 0 at the four corners, every G_kk > 0 there
    xs, ys = np.arange(6.0), np.arange(5.0)
    X, Y = np.meshgrid(xs, ys)
    b = np.stack([X, np.zeros_like(X), X + Y + 3.0])
    _p, bad, gpos, piv = fm.flow_fit_core(xs, ys, b, b, 1.0, 1)
    for j, i in ((0, 0), (0, 5), (4, 0), (4, 5)):
        assert gpos[j, i] and not bad[j, i] and piv[3, j, i] == 0.0 and np.all(piv[:3, j, i] > 0.0)


def test_slices_and_reduction_order():
    assert fm.slices_of(4) == [(0, 4)] and fm.slices_of(4096) == [(0, 4096)]
    assert fm.slices_of(4410) == [(0, 2205), (2205, 4410)]
    assert len(fm.slices_of(64 * 4096 + 1)) == 64
    rng = np.random.default_rng(5)
    for shape in ((2, 2), (63, 70), (3, 300), (2100, 3)):
        t = rng.uniform(-1.0, 1.0, shape)
        got = fm.reduce_rows(t)
        assert abs(got - t.sum()) <= 1e-13 * np.abs(t).sum()
    # one row of up to 256 pixels: the tree alone
    t = rng.uniform(-1.0, 1.0, (1, 200))
    lanes = np.zeros(256)
    lanes[:200] = t[0]
    o = 128
    while o:
        lanes[:o] += lanes[o:2 * o]
        o //= 2
    assert fm.reduce_rows(t) == lanes[0]


def test_points_and_plane_restatements_agree_on_the_nodes():
    xs, ys = fm.mesh2((7, 5), (0.5, 0.25))
    bz = fm.white_noise((7, 5), 9, 1)[0]
    plane = fm.green_ap_numpy(xs, ys, bz)
    X, Y = np.meshgrid(xs, ys)
    pts = fm.green_ap_numpy(xs, ys, bz, np.stack([X.ravel(), Y.ravel()], axis=1))
    assert np.array_equal(pts[:, 0].reshape(5, 7), plane[0]) and np.array_equal(pts[:, 1].reshape(5, 7), plane[1])
    # z . curl A_p = B_z and div_h A_p = 0 away from the edge, to the truncation of the quotients and of the edge
    xs2, ys2 = fm.mesh2((41, 41), (0.05, 0.05))
    X2, Y2 = np.meshgrid(xs2, ys2)
    smooth = np.exp(-((X2 - xs2[20]) ** 2 + (Y2 - ys2[20]) ** 2) / 0.08)
    ap = fm.green_ap_numpy(xs2, ys2, smooth)
    curl = fm.ddq2(ap[1], 1, 0.05) - fm.ddq2(ap[0], 0, 0.05)
    div = fm.ddq2(ap[0], 1, 0.05) + fm.ddq2(ap[1], 0, 0.05)
    inner = (slice(8, -8), slice(8, -8))
    bound = 0.05 ** 2 / 0.08                         # h^2 / sigma^2: the second-order truncation on values up to 1
    assert np.abs(curl - smooth)[inner].max() < bound and np.abs(div)[inner].max() < bound
