"""GPU tests of field-line tracing and field-line helicity (run with -m gpu on an MI355X): VecPot.trace,
trace_field_lines, field_line_helicity.  The yardsticks are a numpy restatement of the semantics in
include/ndsm_hip.h (line_model.trace_numpy; bit for bit) and closed-form fields: a uniform field (straight lines,
exact integrals), a linear helical field B = (-eps (y - yc), eps (x - xc), B0) (trilinear interpolation is exact, only
the integrator errs), its B0 = 0 form (closed circles), fields with zeros and NaNs, and the identity
sum over entering feet of flh |B.n| dS = int A.B dV.  Every mesh-dependent test runs on golden_inputs.aniso_mesh
(unequal spacings, no origin at 0) as well as on a uniform mesh, with unequal nx, ny, nz."""
import numpy as np
import pytest

from golden_inputs import aniso_mesh, uniform_mesh
from line_model import (FACES, NULL, OUTSIDE, UNFINISHED, abc, axis_of, box, centre, entering_feet, face_seeds, grids,
                        helical, inner_seeds, trace_numpy, weights1)

pytestmark = pytest.mark.gpu

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def lib_trace(mesh, b, seeds, g=None, step=0.5, max_steps=None, direction="both", device=False):
    import ndsm_amd
    V = ndsm_amd.VecPot(*mesh)
    try:
        return V.trace(b, seeds, g=g, step=step, max_steps=max_steps, direction=direction, device=device)
    finally:
        V.close()


# The sum-rule tests put the axis well outside the box, beyond its lower x-y corner.  (1) With this A, A.B = eps b0 / 2
# (xc (x - xc) + yc (y - yc)), whose volume integral vanishes identically about a centred axis: nothing to compare
# against.  (2) The projected lines are circles about the axis; a circle touches a face x = const only at y = yc and
# a face y = const only at x = xc, and both points lie outside the box, so no line grazes a face inside it.  Then
# flh is a continuous function of the foot (no jump in connectivity or length) and the trapezoid sum over the feet
# is second order; with the axis inside the box, lines graze the side faces, flh jumps there and the sum is first
# order with an erratic coefficient (numpy restatement, axis at 0.4 of the extent, aniso: 2.0e-2, 1.1e-2, 8.5e-3).
# (3) The gap is a sum of O(h^2) terms of either sign (the trilinear A_z, the kinks of flh where the exit face
# changes); the ratio shows the order only where the gap keeps its sign, which the tests assert as well.  With the
# numpy restatement the signed gaps at n = 16, 32, 64 are +3.5e-3, +9.6e-4, +2.3e-4 (aniso) and +3.1e-3, +6.5e-4,
# +1.6e-4 (uniform) for this axis; one at -0.3 of the extent changes sign between n = 32 and 64.
OFF_CENTRE = (-1.5, -1.5)


def volume_sum(mesh, a, b):
    ws = [weights1(q) for q in mesh]
    w = ws[2][:, None, None] * ws[1][None, :, None] * ws[0][None, None, :]
    return float((w * (a * b).sum(axis=0)).sum())


def rel(a, b):
    return np.abs(a - b) / np.abs(b)


# ---------------------------------------------------------------------------------------------------------------
# 1. the numpy restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [0.5, 0.37])
@pytest.mark.parametrize("kind,shape", [("aniso", [33, 22, 27]), ("uniform", [24, 30, 20])])
def test_matches_the_numpy_restatement_bitwise(hip, kind, shape, step):
    """status and step counts equal; ends, length and integral bitwise equal.  fp64 +, -, *, / and sqrt are
    correctly rounded on both sides and the device code is built without contraction."""
    mesh = MESHES[kind](shape)
    b = abc(mesh)
    g = abc(mesh, k=0.7 * np.pi, phase=0.3)
    rng = np.random.default_rng(2115)
    seeds = np.concatenate([inner_seeds(mesh, rng, 200), face_seeds(mesh, rng, 20)])
    max_steps = 300
    got = lib_trace(mesh, b, seeds, g=g, step=step, max_steps=max_steps)
    assert got.ends.shape == (2, len(seeds), 3) and got.status.dtype == np.int32
    seen = set()
    for row, sgn in ((0, 1.0), (1, -1.0)):
        ends, length, integral, status, nsteps = trace_numpy(mesh, b, g, seeds, step, max_steps, sgn)
        dev = [np.abs(got.ends[row] - ends).max(), np.abs(got.length[row] - length).max(),
               np.abs(got.integral[row] - integral).max()]
        print(kind, step, "sgn", sgn, "max deviations (ends, length, integral):", dev,
              "status differs:", int((got.status[row] != status).sum()))
        assert np.array_equal(got.status[row], status)
        assert np.array_equal(got.nsteps[row], nsteps)
        assert np.array_equal(got.ends[row], ends)
        assert np.array_equal(got.length[row], length)
        assert np.array_equal(got.integral[row], integral)
        seen |= set(status.tolist())
    assert np.array_equal(got.flh, got.integral[0] + got.integral[1])
    assert seen >= set(FACES), seen                 # lines left through all six faces


# ---------------------------------------------------------------------------------------------------------------
# 2. uniform field: straight lines, exact integrals
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", [("aniso", [24, 27, 22]), ("uniform", [21, 26, 23])])
def test_uniform_field_is_exact(hip, kind, shape):
    """B = (0.3, -0.2, 0.9), G = (b_y z, b_z x, b_x y): curl G = B and G.b is linear along a line, which RK4
    integrates exactly.  Lengths, end points and integrals to 1e-12 relative (rounding over <= 1e3 steps)."""
    mesh = MESHES[kind](shape)
    X, Y, Z = grids(mesh)
    bv = np.array([0.3, -0.2, 0.9])
    bh = bv / np.sqrt((bv * bv).sum())
    b = np.stack([np.full(X.shape, v) for v in bv])
    g = np.stack([bv[1] * Z, bv[2] * X, bv[0] * Y])

    def gdot(p):
        return (bv[1] * p[:, 2]) * bh[0] + (bv[2] * p[:, 0]) * bh[1] + (bv[0] * p[:, 1]) * bh[2]

    rng = np.random.default_rng(2116)
    seeds = np.concatenate([inner_seeds(mesh, rng, 150), face_seeds(mesh, rng, 10)])
    lo, _h, hi, _n = box(mesh)
    scale = np.abs(np.concatenate([lo, hi])).max()
    for step in (0.5, 0.37):
        fl = lib_trace(mesh, b, seeds, g=g, step=step)
        assert np.all(np.isin(fl.status, list(FACES)))
        for row in (0, 1):
            ax = (fl.status[row] - 1) >> 1
            want = np.where((fl.status[row] - 1) & 1, hi[ax], lo[ax])
            assert np.array_equal(fl.ends[row][np.arange(len(seeds)), ax], want)       # on the face exactly
            assert np.all((fl.ends[row] >= lo) & (fl.ends[row] <= hi))
            chord = np.sqrt(((fl.ends[row] - seeds) ** 2).sum(axis=1))
            err_len = np.abs(fl.length[row] - chord).max() / scale
            mid = 0.5 * (fl.ends[row] + seeds)
            err_int = np.abs(fl.integral[row] - fl.length[row] * gdot(mid)).max() / np.abs(g).max()
            print(kind, step, "row", row, "length err", err_len, "integral err", err_int)
            assert err_len <= 1e-12 and err_int <= 1e-12
        # the whole line through each seed: flh = length * G(midpoint of the two feet) . b
        total = fl.length[0] + fl.length[1]
        chord = np.sqrt(((fl.ends[0] - fl.ends[1]) ** 2).sum(axis=1))
        mid = 0.5 * (fl.ends[0] + fl.ends[1])
        err_len = np.abs(total - chord).max() / scale
        err_flh = np.abs(fl.flh - total * gdot(mid)).max() / (np.abs(g).max() * scale)
        print(kind, step, "whole lines: length err", err_len, "flh err", err_flh)
        assert err_len <= 1e-12 and err_flh <= 1e-12
        assert total.min() > 0.0


# ---------------------------------------------------------------------------------------------------------------
# 3. helical lines: order of accuracy
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", [("aniso", [24, 27, 22]), ("uniform", [24, 27, 22])])
def test_helical_lines_are_fourth_order(hip, kind, shape):
    """lines of B = (-eps (y - yc), eps (x - xc), B0) from the bottom face reach the top face at the helix angle
    phi0 + eps Lz / B0 with length Lz sqrt(1 + (eps rho / B0)^2); the field is linear, so only the integrator errs.
    Errors fall by >= 10 per halving of the step (fourth order with margin) while they are above 1e-12."""
    eps, b0 = 1.5, 1.0
    mesh = MESHES[kind](shape)
    b, _a = helical(mesh, eps, b0)
    lo, _h, hi, _n = box(mesh)
    xc, yc = axis_of(mesh)
    lz = hi[2] - lo[2]
    rho = np.repeat([0.05, 0.15, 0.3], 8)
    phi0 = np.tile(np.arange(8) * (2 * np.pi / 8) + 0.1, 3)
    seeds = np.stack([xc + rho * np.cos(phi0), yc + rho * np.sin(phi0), np.full(len(rho), lo[2])], axis=1)
    phi1 = phi0 + eps * lz / b0
    want_end = np.stack([xc + rho * np.cos(phi1), yc + rho * np.sin(phi1), np.full(len(rho), hi[2])], axis=1)
    want_len = lz * np.sqrt(1.0 + (eps * rho / b0) ** 2)
    e_len, e_end = [], []
    for step in (2.0, 1.0, 0.5, 0.25):
        fl = lib_trace(mesh, b, seeds, step=step, direction="forward")
        assert np.all(fl.status[0] == 6)
        assert np.array_equal(fl.ends[0][:, 2], np.full(len(rho), hi[2]))
        e_len.append(np.abs(fl.length[0] - want_len).max())
        e_end.append(np.sqrt(((fl.ends[0] - want_end) ** 2).sum(axis=1)).max())
    print(kind, "length errors", e_len, "end-point errors", e_end)
    for e in (e_len, e_end):
        for coarse, fine in zip(e[:-1], e[1:]):
            assert fine > 1e-12, "rounding took over: the steps of this test are too fine to show the order"
            assert coarse / fine >= 10.0, e


# ---------------------------------------------------------------------------------------------------------------
# 4. closed lines terminate
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", [("aniso", [24, 27, 22]), ("uniform", [24, 27, 22])])
def test_closed_lines_end_at_max_steps(hip, kind, shape):
    """B0 = 0: every line is a circle around the axis.  One call; each line takes exactly max_steps steps."""
    mesh = MESHES[kind](shape)
    b, a = helical(mesh, 1.5, 0.0)
    lo, h, hi, _n = box(mesh)
    c = centre(mesh)
    rho = np.repeat([0.05, 0.15, 0.3], 4)
    phi = np.tile(np.arange(4) * (np.pi / 2) + 0.2, 3)
    seeds = np.stack([c[0] + rho * np.cos(phi), c[1] + rho * np.sin(phi),
                      lo[2] + (hi[2] - lo[2]) * np.linspace(0.0, 1.0, len(rho))], axis=1)
    fl = lib_trace(mesh, b, seeds, g=a, step=0.5, max_steps=500)
    ds = 0.5 * h.min()
    assert np.all(fl.status == UNFINISHED) and np.all(fl.nsteps == 500)
    assert np.abs(fl.length - 500 * ds).max() <= 1e-12 * 500 * ds
    assert np.all((fl.ends >= lo) & (fl.ends <= hi))
    radius = np.sqrt(((fl.ends[..., :2] - c[:2]) ** 2).sum(axis=-1))
    # still on their circles: RK4 turns by theta = ds / rho per step and shrinks the radius by theta^6 / 144 of
    # itself (its stability polynomial on the imaginary axis); twice that over 500 steps is the bound
    assert np.all(np.abs(radius / rho - 1.0) <= 500 * (ds / rho) ** 6 / 72 + 1e-12)
    # max_steps = 1: one step, no more
    fl = lib_trace(mesh, b, seeds, step=0.5, max_steps=1)
    assert np.all(fl.status == UNFINISHED) and np.all(fl.nsteps == 1) and np.all(fl.length == ds)


# ---------------------------------------------------------------------------------------------------------------
# 5. nulls, NaN, seeds outside
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", [("aniso", [20, 17, 23]), ("uniform", [20, 17, 23])])
def test_nulls_nan_and_outside_seeds(hip, kind, shape):
    mesh = MESHES[kind](shape)
    lo, h, hi, n = box(mesh)
    X, _Y, _Z = grids(mesh)
    up = np.stack([np.zeros(X.shape), np.zeros(X.shape), np.ones(X.shape)])
    g = np.stack([np.zeros(X.shape), np.zeros(X.shape), np.full(X.shape, 2.0)])
    ci, cj, ck = 7, 5, 11                                          # the cell whose eight corners are changed

    def col(i, j, fz=0.25):
        """a seed in the column of cell (i, j), a quarter of the way up the box"""
        return [lo[0] + (i + 0.5) * h[0], lo[1] + (j + 0.5) * h[1], lo[2] + fz * (hi[2] - lo[2])]

    seeds = np.array([col(ci, cj), col(ci + 4, cj + 3), col(2, 2)])
    # (a) a field that is zero at the corners of one cell: the line below it stops there, the others do not
    b = up.copy()
    b[:, ck:ck + 2, cj:cj + 2, ci:ci + 2] = 0.0
    fl = lib_trace(mesh, b, seeds, g=g, direction="forward")
    assert fl.status[0].tolist() == [NULL, 6, 6]
    zc = lo[2] + ck * h[2]
    assert lo[2] + (ck - 1) * h[2] < fl.ends[0][0, 2] <= zc + h[2]       # stopped at the last accepted point
    assert np.array_equal(fl.ends[0][0, :2], seeds[0, :2])
    assert np.all(np.isfinite(fl.ends)) and np.all(np.isfinite(fl.length)) and np.all(np.isfinite(fl.integral))
    assert np.abs(fl.length[0][1:] - (hi[2] - seeds[1:, 2])).max() <= 1e-12
    assert np.abs(fl.integral[0] - 2.0 * fl.length[0]).max() <= 1e-12   # G.b = 2 along what was traced
    # a seed at the null itself: no step at all
    fl0 = lib_trace(mesh, b, np.array([col(ci, cj, 0.0)[:2] + [zc + 0.5 * h[2]]]), g=g)
    assert np.all(fl0.status == NULL) and np.all(fl0.nsteps == 0) and np.all(fl0.length == 0.0)
    # (b) a NaN: off the traced paths it changes nothing, on a path the line stops with the null status
    b = up.copy()
    b[2, ck, cj, ci] = np.nan
    clean = lib_trace(mesh, up, seeds[1:], g=g)
    fl = lib_trace(mesh, b, seeds, g=g)
    for got, want in zip(fl[:5], clean[:5]):
        assert np.array_equal(got[:, 1:], want)                         # the lines away from it: the same bits
    assert np.array_equal(fl.flh[1:], clean.flh)
    assert fl.status[0].tolist() == [NULL, 6, 6] and fl.status[1].tolist() == [5, 5, 5]
    for arr in (fl.ends, fl.length, fl.integral, fl.flh):
        assert np.all(np.isfinite(arr))
    assert fl.ends[0][0, 2] <= zc
    # (c) seeds outside the box, and not finite
    out = np.array([[lo[0] - 1e-9, c_[1], c_[2]] for c_ in [centre(mesh)]] +
                   [[centre(mesh)[0], hi[1] + 0.3, centre(mesh)[2]], [centre(mesh)[0], centre(mesh)[1], np.nan],
                    [np.inf, centre(mesh)[1], centre(mesh)[2]], list(centre(mesh))])
    fl = lib_trace(mesh, up, out, g=g)
    assert np.all(fl.status[:, :4] == OUTSIDE) and np.all(fl.nsteps[:, :4] == 0)
    assert np.all(fl.length[:, :4] == 0.0) and np.all(fl.integral[:, :4] == 0.0)
    for row in (0, 1):
        assert np.array_equal(fl.ends[row][:4], out[:4], equal_nan=True)
    assert fl.status[:, 4].tolist() == [6, 5]


# ---------------------------------------------------------------------------------------------------------------
# 6. the flux-weighted sum of the field-line helicity is the volume helicity
# ---------------------------------------------------------------------------------------------------------------
def sum_rule_gap(mesh, b, a, tracer):
    """(sum over entering feet of flh |B.n| w - sum w A.B) / |sum w A.B|, signed, and the lines"""
    seeds, flux = entering_feet(mesh, b)
    fl = tracer(seeds)
    total = float((fl.flh * flux).sum())
    vol = volume_sum(mesh, a, b)
    return (total - vol) / abs(vol), fl


@pytest.mark.parametrize("kind", ["aniso", "uniform"])
def test_flux_weighted_sum_is_the_volume_helicity(hip, kind):
    """B = (-1.5 (y - yc), 1.5 (x - xc), 1), axis outside the box (OFF_CENTRE), with its analytic A: every line connects boundary to boundary, so
    sum_feet flh |B.n| dS = int A.B dV.  Both sides are second order in h (trapezoid sums; trilinear A): the gap
    falls by >= 3 per doubling of n."""
    gaps = []
    for n in (16, 32, 64):
        mesh = MESHES[kind]([n, n + 3, n - 2])
        b, a = helical(mesh, axis=OFF_CENTRE)
        gap, fl = sum_rule_gap(mesh, b, a, lambda s: lib_trace(mesh, b, s, g=a, step=0.5))
        assert np.all(np.isin(fl.status, list(FACES))), "a line ended at a null or unfinished"
        gaps.append(gap)
    print(kind, "signed gaps at n = 16, 32, 64:", gaps)
    assert np.all(np.sign(gaps) == np.sign(gaps[0])), gaps
    assert gaps[0] / gaps[1] >= 3.0 and gaps[1] / gaps[2] >= 3.0, gaps


# ---------------------------------------------------------------------------------------------------------------
# 7. through the library's own A
# ---------------------------------------------------------------------------------------------------------------
HEL_SCALARS = ("ierr", "H_R", "H_J", "E", "E_p", "E_free", "recon_max", "recon_rms", "divB_max", "divA_max")


@pytest.mark.parametrize("gauge", ["devore", "coulomb"])
def test_field_line_helicity_uses_the_chains_own_potential(hip, gauge):
    import ndsm_amd
    from test_gpu_field import abc_field
    mesh, b = abc_field([33, 30, 35])
    rng = np.random.default_rng(2117)
    seeds = np.concatenate([inner_seeds(mesh, rng, 100), face_seeds(mesh, rng, 5)])
    V = ndsm_amd.VecPot(*mesh)
    try:
        fl, hel = V.field_line_helicity(b, seeds, gauge=gauge, max_steps=200, return_fields=True, vc_tol=1e-12)
        want = V.helicity(b, gauge=gauge, return_fields=True, vc_tol=1e-12)
        for k in HEL_SCALARS:
            assert getattr(hel, k) == getattr(want, k), k
        for k in ("A", "A_p", "B_p"):
            assert np.array_equal(getattr(hel, k), getattr(want, k)), k
        host = V.trace(b, seeds, g=hel.A, max_steps=200)
        dev = V.trace(b, seeds, g=hel.A, max_steps=200, device=True)
        given, none = V.field_line_helicity(b, seeds, a=hel.A, max_steps=200)
        assert none is None
        for other in (host, dev, given):
            for x, y in zip(fl, other):
                assert np.array_equal(x, y)
        assert np.abs(fl.integral).max() > 0.0
    finally:
        V.close()
    # the one-shot form
    fl1, hel1 = ndsm_amd.field_line_helicity(*mesh, b, seeds, gauge=gauge, max_steps=200, vc_tol=1e-12)
    assert np.array_equal(fl1.integral, fl.integral) and hel1.H_R == hel.H_R and hel1.A is None


def test_sum_rule_with_the_devore_potential(hip):
    """the sum rule of the helical field with the library's DeVore-gauge A against the same call's sum w A.B"""
    import ndsm_amd
    gaps = []
    for n in (16, 32, 64):
        mesh = aniso_mesh([n, n + 3, n - 2])
        b, _a = helical(mesh, axis=OFF_CENTRE)
        seeds, flux = entering_feet(mesh, b)
        fl, hel = ndsm_amd.field_line_helicity(*mesh, b, seeds, gauge="devore", return_fields=True)
        assert np.all(np.isin(fl.status, list(FACES)))
        vol = volume_sum(mesh, hel.A, b)
        gaps.append((float((fl.flh * flux).sum()) - vol) / abs(vol))
    print("DeVore-gauge signed gaps at n = 16, 32, 64:", gaps)
    assert np.all(np.sign(gaps) == np.sign(gaps[0])), gaps
    assert gaps[0] / gaps[1] >= 3.0 and gaps[1] / gaps[2] >= 3.0, gaps


# ---------------------------------------------------------------------------------------------------------------
# 8. order independence and options
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", [("aniso", [33, 22, 27])])
def test_lines_do_not_depend_on_each_other(hip, kind, shape):
    mesh = MESHES[kind](shape)
    b = abc(mesh)
    g = abc(mesh, k=0.7 * np.pi, phase=0.3)
    rng = np.random.default_rng(2118)
    seeds = np.concatenate([inner_seeds(mesh, rng, 150), face_seeds(mesh, rng, 5)])
    kw = dict(step=0.37, max_steps=250)
    ref = lib_trace(mesh, b, seeds, g=g, **kw)
    perm = rng.permutation(len(seeds))
    shuffled = lib_trace(mesh, b, seeds[perm], g=g, **kw)
    for x, y in zip(ref, shuffled):
        assert np.array_equal(x[:, perm] if x.ndim > 1 else x[perm], y)
    cut = 67
    first, second = lib_trace(mesh, b, seeds[:cut], g=g, **kw), lib_trace(mesh, b, seeds[cut:], g=g, **kw)
    for x, y, z in zip(ref, first, second):
        assert np.array_equal(x, np.concatenate([y, z], axis=-1 if x.ndim == 1 else 1))
    fwd = lib_trace(mesh, b, seeds, g=g, direction="forward", **kw)
    bwd = lib_trace(mesh, b, seeds, g=g, direction="backward", device=True, **kw)
    assert fwd.flh is None and bwd.flh is None and fwd.ends.shape == (1, len(seeds), 3)
    for k in ("ends", "length", "integral", "status", "nsteps"):
        assert np.array_equal(getattr(ref, k)[0], getattr(fwd, k)[0]), k
        assert np.array_equal(getattr(ref, k)[1], getattr(bwd, k)[0]), k
    bare = lib_trace(mesh, b, seeds, **kw)
    assert np.all(bare.integral == 0.0) and np.all(bare.flh == 0.0)
    for k in ("ends", "length", "status", "nsteps"):
        assert np.array_equal(getattr(ref, k), getattr(bare, k)), k
    # no seeds: empty arrays
    none = lib_trace(mesh, b, np.zeros((0, 3)), g=g)
    assert none.ends.shape == (2, 0, 3) and none.flh.shape == (0,)
    # the default max_steps scales with the box
    import ndsm_amd
    V = ndsm_amd.VecPot(*mesh)
    try:
        assert V.default_max_steps(0.5) == int(np.ceil(4 * sum(shape) / 0.5))
        with pytest.raises(ValueError):
            V.trace(b, seeds, step=0.0)
        with pytest.raises(ValueError):
            V.trace(b, seeds, max_steps=0)
        with pytest.raises(ValueError):
            V.trace(b, seeds, direction="up")
    finally:
        V.close()


def test_c_entries_reject_bad_scalars(hip):
    """9002 for a NULL handle or array, 9004 for a scalar out of range, the host outputs cleared; no seeds: 0"""
    import ndsm_amd
    mesh = aniso_mesh([12, 11, 10])
    b = np.ascontiguousarray(abc(mesh))
    seeds = np.ascontiguousarray(inner_seeds(mesh, np.random.default_rng(1), 4))
    V = ndsm_amd.VecPot(*mesh)
    try:
        L = V.L

        def call(h, bb, ns, step, max_steps, direction):
            out = [np.full((2, 4, 3), 7.0), np.full((2, 4), 7.0), np.full((2, 4), 7.0),
                   np.full((2, 4), 7, dtype=np.int32), np.full((2, 4), 7, dtype=np.int32)]
            rc = L.ndsm_hip_vecpot_trace(h, bb, None, ns, seeds.ctypes.data, step, max_steps, direction,
                                         *[a.ctypes.data for a in out])
            return rc, out
        rc, out = call(V.h, b.ctypes.data, 4, 0.5, 10, 0)
        assert rc == 0 and np.all(out[3] != 7)
        for args in ((V.h, b.ctypes.data, 4, 0.0, 10, 0), (V.h, b.ctypes.data, 4, -1.0, 10, 0),
                     (V.h, b.ctypes.data, 4, 0.5, 0, 0), (V.h, b.ctypes.data, 4, 0.5, 10, 2),
                     (V.h, b.ctypes.data, 4, float("nan"), 10, 1)):
            rc, out = call(*args)
            assert rc == 9004, args
            nl = 8 if args[5] == 0 else 4
            assert all(np.all(a.reshape(-1)[:nl * (3 if a.ndim == 3 else 1)] == 0) for a in out), args
        assert call(V.h, b.ctypes.data, -1, 0.5, 10, 0)[0] == 9004
        assert call(None, b.ctypes.data, 4, 0.5, 10, 0)[0] == 9002
        rc, out = call(V.h, None, 4, 0.5, 10, 0)
        assert rc == 9002 and np.all(out[3] == 0)
        rc, out = call(V.h, None, 0, 0.5, 10, 0)
        assert rc == 0 and np.all(out[3] == 7)                      # nothing is touched
    finally:
        V.close()
