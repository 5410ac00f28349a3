"""GPU tests of the flow inversion, the plane's vector potential and the boundary fluxes (run with -m gpu on an MI355X):
the eight C entries and flow_fit, plane_vector_potential, plane_vector_potential_points, boundary_fluxes.  The yardsticks
are the numpy restatements of the semantics in include/ndsm_hip.h (flow_model: every output bit for bit, through the
host and the device entry and twice in a row) and closed forms (flow_model's checks, which test_flow_model.py runs with
the restatements): an affine flow under cubic fields recovered, rank deficiency predicted from the degree of the field,
values that are not finite, a single pixel's and a Gaussian's vector potential, the field-aligned flow that carries no
flux, uniform fields' totals."""
import numpy as np
import pytest

import flow_model as fm
from device_arena import Arena, LibTransport, slot

pytestmark = pytest.mark.gpu

FILL = 3.25
IDS = lambda s: "x".join(map(str, s))   # noqa: E731


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def head(xs, ys):
    from ndsm_amd import _lib
    ns = np.array([len(xs), len(ys)], dtype=np.intc)
    xs, ys = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(ys, dtype=np.float64)
    return (ns, xs, ys), (ns.ctypes.data_as(_lib._ip), _lib._d(xs), _lib._d(ys))


def flat(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).copy()


def fit_raw(hip, xs, ys, b0, b1, dt, r, rcond, device):
    """one call of a C entry of the fit on FILL-initialised outputs"""
    L = hip.load_library()
    keep, h = head(xs, ys)
    n = (len(ys), len(xs))
    B0, B1 = flat(b0), flat(b1)
    V, C, S = np.full(3 * B0.size // 3, FILL), np.full(3 * B0.size, FILL), np.full(B0.size // 3, 7, dtype=np.int32)
    if not device:
        rc = L.ndsm_hip_flow_fit(*h, B0.ctypes.data, B1.ctypes.data, dt, r, rcond, V.ctypes.data, C.ctypes.data,
                                 S.ctypes.data)
    else:
        rc = hip._staged(L, [B0, B1, V, C, S],
                         lambda d0, d1, dV, dC, dS: L.ndsm_hip_flow_fit_device(*h, d0, d1, dt, r, rcond, dV, dC, dS))
    assert rc == 0, hip.last_error(L)
    assert np.array_equal(B0, flat(b0)) and np.array_equal(B1, flat(b1), equal_nan=True)
    return V.reshape((3,) + n), C.reshape((9,) + n), S.reshape(n)


def ap_raw(hip, xs, ys, bz, device, pts=None):
    L = hip.load_library()
    keep, h = head(xs, ys)
    S = flat(bz)
    if pts is None:
        A = np.full(2 * S.size, FILL)
        if not device:
            rc = L.ndsm_hip_green_ap_plane(*h, S.ctypes.data, A.ctypes.data)
        else:
            rc = hip._staged(L, [S, A], lambda dS, dA: L.ndsm_hip_green_ap_plane_device(*h, dS, dA))
        assert rc == 0, hip.last_error(L)
        return A.reshape(2, len(ys), len(xs))
    P = flat(pts)
    A = np.full(P.size, FILL)
    if not device:
        rc = L.ndsm_hip_green_ap_points(*h, S.ctypes.data, len(P) // 2, P.ctypes.data, A.ctypes.data)
    else:
        rc = hip._staged(L, [S, P, A], lambda dS, dP, dA: L.ndsm_hip_green_ap_points_device(*h, dS, len(P) // 2, dP, dA))
    assert rc == 0, hip.last_error(L)
    return A.reshape(-1, 2)


def flux_raw(hip, xs, ys, b, v, ap, device):
    L = hip.load_library()
    keep, h = head(xs, ys)
    B, V, A = flat(b), flat(v), flat(ap)
    D, out = np.full(4 * len(xs) * len(ys), FILL), np.full(8, FILL)
    if not device:
        rc = L.ndsm_hip_flow_flux(*h, B.ctypes.data, V.ctypes.data, A.ctypes.data, D.ctypes.data, hip._d(out))
    else:
        rc = hip._staged(L, [B, V, A, D], lambda dB, dV, dA, dD: L.ndsm_hip_flow_flux_device(*h, dB, dV, dA, dD, hip._d(out)))
    assert rc == 0, hip.last_error(L)
    return D.reshape(4, len(ys), len(xs)), out


def same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
            raise AssertionError("%s: output %d differs at %d places, first %s: %r != %r"
                                 % (what, k, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])]))


# ---------------------------------------------------------------------------------------------------------------
# bit for bit against the restatement
# ---------------------------------------------------------------------------------------------------------------
# 3x3: every window clipped on all sides; 4x3; 16x16: one tile; 17x16 and 16x17: a tile of one column or one row;
# 33x18 (with r = 16 the window is wider than the magnetogram in y, and three tiles in x); 70x63: 5 x 4 tiles
FIT_SHAPES = [(3, 3), (4, 3), (16, 16), (17, 16), (16, 17), (33, 18), (70, 63)]


@pytest.mark.parametrize("n", FIT_SHAPES, ids=IDS)
def test_fit_bitwise_white_noise(hip, n):
    xs, ys = fm.mesh2(n, (0.1, 0.13))
    b0, b1 = fm.white_noise(n, 31), fm.white_noise(n, 32)
    seen = set()
    for r in (1, 2, 3, 16):
        for dt in ((-0.37,) if r != 2 else (-0.37, 2.5)):
            core = fm.flow_fit_core(xs, ys, b0, b1, dt, r)
            for rcond in (0.0, 1e-10):
                want = fm.flow_fit_finish(core, rcond)
                seen |= set(np.unique(want[2]))
                for device in (False, True):
                    for again in range(2):
                        same(fit_raw(hip, xs, ys, b0, b1, dt, r, rcond, device), want,
                             "%s r %d dt %g rcond %g device %s call %d" % (n, r, dt, rcond, device, again))
    print(n, "statuses seen", sorted(seen))
    assert 0 in seen or n[0] * n[1] < 16


@pytest.mark.parametrize("deg", [3, 2])
def test_fit_bitwise_closed_form_fields(hip, deg):
    for n, h, r in fm.RECOVERY + [((20, 18), (0.1, 0.13), 1)]:
        xs, ys, b0, b1, dt, _v = fm.affine_case(n, h, deg, seed=11)
        core = fm.flow_fit_core(xs, ys, b0, b1, dt, r)
        for rcond in (0.0, 1e-10):
            want = fm.flow_fit_finish(core, rcond)
            for device in (False, True):
                same(fit_raw(hip, xs, ys, b0, b1, dt, r, rcond, device), want, "deg %d %s r %d rcond %g" % (deg, n, r, rcond))


def test_fit_bitwise_bad_values(hip):
    n, r = (33, 18), 3
    xs, ys = fm.mesh2(n, (0.1, 0.13))
    b0, b1 = fm.white_noise(n, 31), fm.white_noise(n, 32)
    b1[2, 9, 16], b1[0, 0, 0], b0[1, 17, 32] = np.nan, np.inf, -np.inf
    want = fm.flow_fit_numpy(xs, ys, b0, b1, 0.5, r, 1e-10)
    assert set(np.unique(want[2])) == {0, 2}
    for device in (False, True):
        same(fit_raw(hip, xs, ys, b0, b1, 0.5, r, 1e-10, device), want, "bad values, device %s" % device)


# 2x2, 3x2: the smallest sources; 65x4: rows longer than a wave; 70x63: 4410 pixels, two slices
AP_SHAPES = [(2, 2), (3, 2), (65, 4), (70, 63)]


@pytest.mark.parametrize("n", AP_SHAPES, ids=IDS)
def test_ap_bitwise(hip, n):
    xs, ys = fm.mesh2(n, (0.1, 0.13))
    bz = fm.white_noise(n, 41, 1)[0]
    want = fm.green_ap_numpy(xs, ys, bz)
    assert len(fm.slices_of(n[0] * n[1])) == (2 if n == (70, 63) else 1)
    X, Y = np.meshgrid(xs, ys)
    nodes = np.stack([X.ravel(), Y.ravel()], axis=1)
    off = nodes[::3] + np.array([0.031, -0.017])                      # points off the nodes, some outside the mesh
    want_off = fm.green_ap_numpy(xs, ys, bz, off)
    for device in (False, True):
        for again in range(2):
            same([ap_raw(hip, xs, ys, bz, device)], [want], "%s plane device %s call %d" % (n, device, again))
            got = ap_raw(hip, xs, ys, bz, device, nodes)
            same([got[:, 0].reshape(n[1], n[0]), got[:, 1].reshape(n[1], n[0])], [want[0], want[1]],
                 "%s points on the nodes, device %s" % (n, device))
            same([ap_raw(hip, xs, ys, bz, device, off)], [want_off], "%s points off the nodes, device %s" % (n, device))


CHUNK = 262144                             # targets per launch (kChunk of csrc/green.hip)


# 3x2: one slice, every target against the model.  70x63: two slices; the model on the targets from CHUNK - 256 to the
# end and on every 1024th before them - a target's sums depend on nothing but the target and the source, so the subset
# loses nothing, and the full model would take half a minute
@pytest.mark.parametrize("n", [(3, 2), (70, 63)], ids=IDS)
def test_ap_points_past_one_chunk(hip, n):
    """262144 + 300 distinct points through the two-sum path: a second launch whose targets start at 262144, whose count
    (300) is below the first one's and no multiple of the block of 256, and whose slice sums reuse the first launch's
    scratch with two components per slice.  All targets differ, so a target written from the other launch's sums, or
    to the other launch's place, shows"""
    xs, ys = fm.mesh2(n, (0.1, 0.13))
    bz = fm.white_noise(n, 43, 1)[0]
    assert len(fm.slices_of(n[0] * n[1])) == (2 if n == (70, 63) else 1)
    m = CHUNK + 300
    rng = np.random.default_rng(44)
    P = np.stack([rng.uniform(xs[0] - 0.2, xs[-1] + 0.2, m), rng.uniform(ys[0] - 0.2, ys[-1] + 0.2, m)], axis=1)
    X, Y = np.meshgrid(xs, ys)
    P[CHUNK - 3:CHUNK + 3] = np.stack([X.ravel(), Y.ravel()], axis=1)[:6]    # source nodes, both sides of the boundary
    assert len(np.unique(P, axis=0)) == m
    if n == (3, 2):
        pick = np.arange(m)
    else:
        pick = np.concatenate([np.arange(0, CHUNK - 256, 1024), np.arange(CHUNK - 256, m)])
    want = fm.green_ap_numpy(xs, ys, bz, P[pick])
    assert np.isfinite(want).all() and not np.array_equal(want[:300], want[-300:])
    for device in (False, True):
        got = ap_raw(hip, xs, ys, bz, device, P)
        assert got.shape == (m, 2)
        same([got[pick]], [want], "%s points past one chunk, device %s" % (n, device))


@pytest.mark.parametrize("n", AP_SHAPES, ids=IDS)
def test_flux_bitwise(hip, n):
    xs, ys = fm.mesh2(n, (0.1, 0.13))
    b, v, ap = fm.white_noise(n, 51), fm.white_noise(n, 52), fm.white_noise(n, 53, 2)
    want = fm.flow_flux_numpy(xs, ys, b, v, ap)
    for device in (False, True):
        for again in range(2):
            same(flux_raw(hip, xs, ys, b, v, ap, device), want, "%s device %s call %d" % (n, device, again))


def test_flux_bitwise_many_rows_and_long_rows(hip):
    """more rows than blocks (2048) and rows longer than a block's 256 lanes: both strides of the reduction"""
    for n in ((3, 2100), (300, 5)):
        xs, ys = fm.mesh2(n, (0.1, 0.13))
        b, v, ap = fm.white_noise(n, 51), fm.white_noise(n, 52), fm.white_noise(n, 53, 2)
        same(flux_raw(hip, xs, ys, b, v, ap, True), fm.flow_flux_numpy(xs, ys, b, v, ap), str(n))


# ---------------------------------------------------------------------------------------------------------------
# caller arrays at an offset base, guard bands on both sides (device_arena)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [(3, 3), (5, 3), (17, 16), (33, 18)], ids=IDS)
def test_entries_on_offset_arrays(hip, n):
    L = hip.load_library()
    xs, ys = fm.mesh2(n, (0.1, 0.13))
    keep, h = head(xs, ys)
    npix = n[0] * n[1]
    b0, b1 = fm.white_noise(n, 31), fm.white_noise(n, 32)
    for plain in (False, True):
        for r in (1, 16):
            A = Arena(LibTransport(L), [slot("B0", flat(b0), field=True), slot("B1", flat(b1), field=True),
                                        slot("V", np.full(3 * npix, FILL), output=True),
                                        slot("coef", np.full(9 * npix, FILL), output=True),
                                        slot("status", np.full(npix, 7, dtype=np.int32), output=True)], plain=plain)
            out = A.run(lambda d0, d1, dV, dC, dS: L.ndsm_hip_flow_fit_device(*h, d0, d1, -0.37, r, 1e-10, dV, dC, dS))
            assert A.rc == 0, hip.last_error(L)
            want = fm.flow_fit_numpy(xs, ys, b0, b1, -0.37, r, 1e-10)
            same([out[2].reshape(3, n[1], n[0]), out[3].reshape(9, n[1], n[0]), out[4].reshape(n[1], n[0])], want,
                 "fit %s r %d plain %s" % (n, r, plain))
        bz = b0[2]
        A = Arena(LibTransport(L), [slot("bz", flat(bz), field=True), slot("Ap", np.full(2 * npix, FILL), output=True)],
                  plain=plain)
        out = A.run(lambda dS, dA: L.ndsm_hip_green_ap_plane_device(*h, dS, dA))
        assert A.rc == 0, hip.last_error(L)
        ap = fm.green_ap_numpy(xs, ys, bz)
        same([out[1].reshape(2, n[1], n[0])], [ap], "ap plane %s plain %s" % (n, plain))
        pts = np.stack([np.tile(xs, n[1]) + 0.031, np.repeat(ys, n[0]) - 0.017], axis=1)[:7]
        A = Arena(LibTransport(L), [slot("bz", flat(bz), field=True), slot("pts", flat(pts)),
                                    slot("Ap", np.full(2 * len(pts), FILL), output=True)], plain=plain)
        out = A.run(lambda dS, dP, dA: L.ndsm_hip_green_ap_points_device(*h, dS, len(pts), dP, dA))
        assert A.rc == 0, hip.last_error(L)
        same([out[2].reshape(-1, 2)], [fm.green_ap_numpy(xs, ys, bz, pts)], "ap points %s plain %s" % (n, plain))
        out8 = np.full(8, FILL)
        A = Arena(LibTransport(L), [slot("B", flat(b0), field=True), slot("V", flat(b1), field=True),
                                    slot("Ap", flat(ap), field=True), slot("dens", np.full(4 * npix, FILL), output=True)],
                  plain=plain)
        out = A.run(lambda dB, dV, dA, dD: L.ndsm_hip_flow_flux_device(*h, dB, dV, dA, dD, hip._d(out8)))
        assert A.rc == 0, hip.last_error(L)
        same([out[3].reshape(4, n[1], n[0]), out8], fm.flow_flux_numpy(xs, ys, b0, b1, ap), "flux %s plain %s" % (n, plain))


# ---------------------------------------------------------------------------------------------------------------
# closed forms with the library
# ---------------------------------------------------------------------------------------------------------------
def fit_lib(xs, ys, b0, b1, dt, r, rcond):
    import ndsm_amd
    return tuple(ndsm_amd.flow_fit(xs, ys, b0, b1, dt, r=r, rcond=rcond))


def ap_lib(xs, ys, bz):
    import ndsm_amd
    return ndsm_amd.plane_vector_potential(xs, ys, bz)


def flux_lib(xs, ys, b, v, ap):
    import ndsm_amd
    f = ndsm_amd.boundary_fluxes(xs, ys, b, v, ap=ap)
    return f.dens, np.array(f.helicity + f.energy + f.flux)


@pytest.mark.parametrize("n,h,r", fm.RECOVERY, ids=lambda v: str(v).replace(" ", ""))
def test_fit_recovers_an_affine_flow(hip, n, h, r):
    """measured with the restatement on the CPU: 3.2e-8 (r = 2), 1.7e-9 (r = 3), 3.3e-10 (r = 5) on values of order 1;
    the tolerance is ten times that (flow_model.RECOVERY_SEEN)"""
    fm.check_recovery(fit_lib, n, h, r, fm.recovery_tol(r))


def test_fit_rank_deficiency(hip):
    fm.check_rank_deficient(fit_lib)


def test_fit_bad_values(hip):
    fm.check_bad_values(fit_lib)


def test_fit_windows_are_clipped(hip):
    fm.check_clipping(fit_lib)


def test_fit_zero_pivot_is_rank_deficient(hip):
    fm.check_zero_pivot(fit_lib)


def test_fit_pivot_rule_is_strict(hip):
    fm.check_pivot_rule(fit_lib)


def test_ap_single_pixel(hip):
    fm.check_single_pixel(ap_lib)


def test_ap_gaussian(hip):
    fm.check_gaussian(ap_lib)


def test_flux_aligned_flow_and_uniform_totals(hip):
    fm.check_aligned_flow(flux_lib)
    fm.check_uniform_totals(flux_lib)


# ---------------------------------------------------------------------------------------------------------------
# errors and the Python layer
# ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(hip):
    L = hip.load_library()
    n = (5, 4)
    xs, ys = fm.mesh2(n, (0.1, 0.13))
    keep, h = head(xs, ys)
    ns, qx, qy = h
    back = np.ascontiguousarray(xs[::-1])
    flatx = np.zeros(5)
    small = np.array([2, 4], dtype=np.intc)
    one = np.array([1, 4], dtype=np.intc)
    b0, b1, ap, bz, pts = flat(fm.white_noise(n, 1)), flat(fm.white_noise(n, 2)), flat(fm.white_noise(n, 3, 2)), \
        flat(fm.white_noise(n, 4, 1)), np.zeros(8)
    for suffix in ("", "_device"):
        dev = suffix == "_device"

        def staged(arrays, call):
            """the call on host arrays, or on device copies of them (every array comes back)"""
            return call(*[a.ctypes.data for a in arrays]) if not dev else hip._staged(L, arrays, call)
        fit = getattr(L, "ndsm_hip_flow_fit" + suffix)
        ip, dp = hip._ip, hip._d
        cases = [(9004, (small.ctypes.data_as(ip), qx, qy), (1.0, 2, 0.0)), (9004, (ns, dp(back), qy), (1.0, 2, 0.0)),
                 (9004, (ns, qx, dp(flatx[:4])), (1.0, 2, 0.0)), (9004, h, (0.0, 2, 0.0)),
                 (9004, h, (float("nan"), 2, 0.0)), (9004, h, (float("inf"), 2, 0.0)), (9004, h, (1.0, 0, 0.0)),
                 (9004, h, (1.0, 17, 0.0)), (9004, h, (1.0, -1, 0.0)), (9004, h, (1.0, 2, -1e-300)),
                 (9004, h, (1.0, 2, 1.0)), (9004, h, (1.0, 2, float("nan"))), (9002, (None, qx, qy), (1.0, 2, 0.0)),
                 (9002, (ns, None, qy), (1.0, 2, 0.0)), (9002, (ns, qx, None), (1.0, 2, 0.0))]
        for code, hh, (dt, r, rcond) in cases:
            V, C, S = np.full(60, FILL), np.full(180, FILL), np.full(20, 7, dtype=np.int32)
            rc = staged([b0, b1, V, C, S], lambda d0, d1, dV, dC, dS: fit(*hh, d0, d1, dt, r, rcond, dV, dC, dS))
            assert rc == code, (suffix, code, dt, r, rcond, rc)
            assert (V == FILL).all() and (C == FILL).all() and (S == 7).all()
        for miss in range(5):
            V, C, S = np.full(60, FILL), np.full(180, FILL), np.full(20, 7, dtype=np.int32)

            def call(*p):
                p = list(p)
                p[miss] = None
                return fit(*h, p[0], p[1], 1.0, 2, 0.0, p[2], p[3], p[4])
            assert staged([b0, b1, V, C, S], call) == 9002, (suffix, miss)
            assert (V == FILL).all() and (C == FILL).all() and (S == 7).all()
        plane = getattr(L, "ndsm_hip_green_ap_plane" + suffix)
        points = getattr(L, "ndsm_hip_green_ap_points" + suffix)
        flux = getattr(L, "ndsm_hip_flow_flux" + suffix)
        for code, hh in ((9004, (one.ctypes.data_as(ip), qx, qy)), (9004, (ns, dp(back), qy)), (9004, (ns, qx, dp(flatx[:4]))),
                         (9002, (None, qx, qy)), (9002, (ns, None, qy)), (9002, (ns, qx, None))):
            A = np.full(40, FILL)
            assert staged([bz, A], lambda dS, dA: plane(*hh, dS, dA)) == code, (suffix, code)
            assert (A == FILL).all()
            A = np.full(8, FILL)
            assert staged([bz, pts, A], lambda dS, dP, dA: points(*hh, dS, 4, dP, dA)) == code, (suffix, code)
            assert (A == FILL).all()
            D, out = np.full(80, FILL), np.full(8, FILL)
            assert staged([b0, b1, ap, D], lambda dB, dV, dA, dD: flux(*hh, dB, dV, dA, dD, dp(out))) == code, (suffix, code)
            assert (D == FILL).all() and (out == FILL).all()
        A = np.full(40, FILL)
        assert staged([bz, A], lambda dS, dA: plane(*h, None, dA)) == 9002
        assert staged([bz, A], lambda dS, dA: plane(*h, dS, None)) == 9002 and (A == FILL).all()
        A = np.full(8, FILL)
        assert staged([bz, pts, A], lambda dS, dP, dA: points(*h, dS, -1, dP, dA)) == 9004
        assert staged([bz, pts, A], lambda dS, dP, dA: points(*h, None, 4, dP, dA)) == 9002
        assert staged([bz, pts, A], lambda dS, dP, dA: points(*h, dS, 4, None, dA)) == 9002
        assert staged([bz, pts, A], lambda dS, dP, dA: points(*h, dS, 4, dP, None)) == 9002
        assert staged([bz, pts, A], lambda dS, dP, dA: points(*h, dS, 0, None, None)) == 0       # npts == 0 touches nothing
        assert (A == FILL).all()
        for miss in range(5):
            D, out = np.full(80, FILL), np.full(8, FILL)

            def call(*p):
                p = list(p) + [dp(out)]
                p[miss] = None
                return flux(*h, *p)
            assert staged([b0, b1, ap, D], call) == 9002, (suffix, miss)
            assert (D == FILL).all() and (out == FILL).all()


def test_python_layer(hip):
    """the Python names against the raw entries; boundary_fluxes(ap=None) is the explicit composition bit for bit;
    status zeroes V"""
    import ndsm_amd
    n = (33, 18)
    xs, ys = fm.mesh2(n, (0.1, 0.13))
    b0, b1 = fm.white_noise(n, 31), fm.white_noise(n, 32)
    b1[2, 9, 16] = np.nan
    raw = fit_raw(hip, xs, ys, b0, b1, 0.5, 5, 1e-10, False)
    assert (raw[2] == 2).any() and (raw[2] == 0).any() and np.isnan(raw[0]).any()
    for kw in ({}, dict(device=True)):
        got = ndsm_amd.flow_fit(xs, ys, b0, b1, 0.5, **kw)
        same([got.v, got.coef, got.status], raw, "flow_fit %s" % kw)
    ap = ndsm_amd.plane_vector_potential(xs, ys, b0[2])
    same([ap, ndsm_amd.plane_vector_potential(xs, ys, b0[2], device=True)], [ap_raw(hip, xs, ys, b0[2], False)] * 2, "ap")
    X, Y = np.meshgrid(xs, ys)
    nodes = np.stack([X.ravel(), Y.ravel()], axis=1)
    for kw in ({}, dict(device=True)):
        at = ndsm_amd.plane_vector_potential_points(xs, ys, b0[2], nodes, **kw)
        assert at.shape == (n[0] * n[1], 2)
        same([at[:, 0].reshape(n[1], n[0]), at[:, 1].reshape(n[1], n[0])], [ap[0], ap[1]], "points %s" % kw)
    v = raw[0].copy()
    v[:, raw[2] != 0] = 0.0
    dens, out = flux_raw(hip, xs, ys, b0, v, ap, False)
    for kw in (dict(ap=ap), dict(ap=None), dict(ap=ap, device=True)):
        got = ndsm_amd.boundary_fluxes(xs, ys, b0, raw[0], status=raw[2], **kw)
        same([got.dens, np.array(got.helicity + got.energy + got.flux)], [dens, out], "boundary_fluxes %s" % kw)
    assert got.helicity[2] == got.helicity[0] + got.helicity[1] and got.energy[2] == got.energy[0] + got.energy[1]
    assert got.flux[0] >= abs(got.flux[1])
