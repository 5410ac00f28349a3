"""GPU tests of the perpendicular squashing factor (run with -m gpu on an MI355X): VecPot.squashing_perp,
perpendicular_squashing and the two C entries.  The yardsticks are squash_perp_model.squash_perp_numpy, the numpy
restatement of the semantics in include/ndsm_hip.h (bit for bit), VecPot.squashing on the same call (q and the line
outputs, bit for bit), and the closed forms of squash_perp_model, which test_squash_perp_model.py runs on the
restatement without a GPU: a uniform field (Q-perp = 2 for every pair of faces, where Q is |B|^2 / |B_a B_c|), the
helical field (2 on every line, and the twist number), a hyperbolic field, finite differences of VecPot.trace, and the
invariance along a line.  Where a bound is a multiple of the restatement's own error, the restatement runs on the CPU
inside the test; the device agrees with it bit for bit by test 1, so the factor is margin for a later change of seeds
only.  Every test runs on golden_inputs.aniso_mesh (unequal spacings, no origin at 0) and on a uniform mesh."""
import ctypes

import numpy as np
import pytest

from device_arena import Arena, LibTransport, slot
from golden_inputs import aniso_mesh, uniform_mesh
from line_model import FACES, abc, face_seeds, inner_seeds
from test_gpu_squash import CONST_SHAPES, FD_SHAPES, along_line_spread, assert_order
from test_gpu_squash import numpy_tracer as forward_tracer
import squash_perp_model as P

pytestmark = pytest.mark.gpu

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
KINDS = ["aniso", "uniform"]
SHAPE = [24, 27, 22]
LINE_FIELDS = ("ends", "length", "integral", "status", "nsteps")


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def lib_trace(mesh, b, seeds, **kw):
    import ndsm_amd
    V = ndsm_amd.VecPot(*mesh)
    try:
        return V.trace(b, seeds, **kw)
    finally:
        V.close()


def lib_run(mesh, b, seeds, **kw):
    import ndsm_amd
    V = ndsm_amd.VecPot(*mesh)
    try:
        return V.squashing_perp(b, seeds, **kw)
    finally:
        V.close()


def lib_squash(mesh, b, seeds, **kw):
    import ndsm_amd
    V = ndsm_amd.VecPot(*mesh)
    try:
        return V.squashing(b, seeds, **kw)
    finally:
        V.close()


def same(x, y):
    return np.array_equal(x, y, equal_nan=(x.dtype.kind == "f"))


# ---------------------------------------------------------------------------------------------------------------
# 1. the numpy restatement, and VecPot.squashing, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["noG", "G0", "G1"])
@pytest.mark.parametrize("kind,shape,step", [("aniso", [33, 22, 27], 0.5), ("uniform", [24, 30, 20], 0.37)])
def test_matches_the_numpy_restatement_bitwise(hip, kind, shape, step, case):
    mesh = MESHES[kind](shape)
    b = abc(mesh)
    g = None if case == "noG" else abc(mesh, k=0.7 * np.pi, phase=0.3)
    integrand = 1 if case == "G1" else 0
    rng = np.random.default_rng(2119)
    seeds = np.concatenate([inner_seeds(mesh, rng, 160), face_seeds(mesh, rng, 12)])
    max_steps = 300
    kw = dict(g=g, integrand=integrand, step=step, max_steps=max_steps)
    got = lib_run(mesh, b, seeds, **kw)
    want = P.squash_perp_numpy(mesh, b, g, seeds, step, max_steps, integrand)
    assert got.q_perp.shape == (len(seeds),) and got.q_perp.dtype == np.float64 and got.twist is None
    names = ("q", "q_perp") + LINE_FIELDS
    have = [getattr(got, k) for k in names]
    for name, x, y in zip(names, have, want):
        print(kind, case, name, "entries that differ:", int((~((x == y) | ((x != x) & (y != y)))).sum()))
    for name, x, y in zip(names, have, want):
        assert x.dtype == y.dtype and same(x, y), name
    assert set(want[5].reshape(-1).tolist()) >= set(FACES)           # lines left through all six faces
    ok = np.isfinite(want[1])
    assert ok.sum() >= len(seeds) // 2 and np.abs(want[1][ok] / want[0][ok] - 1.0).max() > 0.1
    # q and the five line outputs are those of VecPot.squashing on the same call, through the host and the device entry
    for device in (False, True):
        ref = lib_squash(mesh, b, seeds, device=device, **kw)
        both = lib_run(mesh, b, seeds, device=device, **kw)
        for name in ("q",) + LINE_FIELDS:
            assert same(getattr(both, name), getattr(ref, name)), (name, device)
        assert same(both.q_perp, got.q_perp), device


# ---------------------------------------------------------------------------------------------------------------
# 2. uniform field: what the feature is for
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_uniform_field(hip, kind):
    """Q-perp = 2 to 1e-12 for every pair of faces, mixed-axis pairs included, where Q on the same seeds is |B|^2 /
    |B_a B_c| != 2 between faces normal to different axes (restatement: |Q-perp - 2| <= 8.9e-16, Q up to 15.7)"""
    mesh = MESHES[kind](SHAPE)
    P.check_uniform(lib_run, mesh, P.uniform_seeds(mesh))


# ---------------------------------------------------------------------------------------------------------------
# 3. helical field: Q-perp = 2 on every line, and the twist number
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_helical_field_and_twist(hip, kind):
    """restatement, |Q-perp - 2| / 2 at steps 1, 0.5, 0.25: aniso 2.1e-6, 1.2e-8, 4.3e-9; uniform 3.8e-7, 5.6e-8,
    1.7e-9 (the factors per halving are irregular, so the fall is asked for over the two halvings).  T_w against the
    closed form over the line's own z extent, held to the same rule: aniso 1.3e-4, 7.6e-7, 2.7e-7; uniform 4.9e-6,
    9.9e-7, 3.0e-8 (lines that graze a side face, which the bottom-to-top lines of test_gpu_squash.py do not have)"""
    mesh = MESHES[kind](SHAPE)
    mq, mt = P.helical_errors(P.model_run, mesh)
    dq, dt = P.helical_errors(lib_run, mesh)
    print(kind, "helical Q-perp, restatement:", mq, "device:", dq, "T_w, restatement:", mt, "device:", dt)
    assert mq[0] / mq[2] >= 100.0 and mq[2] < 1e-7
    assert mt[0] / mt[2] >= 100.0 and mt[2] < 1e-6
    for m, d in zip(mq + mt, dq + dt):
        assert d <= 2.0 * m, (mq, dq, mt, dt)


# ---------------------------------------------------------------------------------------------------------------
# 4. hyperbolic field
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha_lz", [1.0, 3.0])
@pytest.mark.parametrize("kind", KINDS)
def test_hyperbolic_field(hip, kind, alpha_lz):
    """seeds on and off the axis at random heights; alpha Lz = 1: every line bottom to top, 3: lines reach the x and
    y faces too.  Restatement, steps 2, 1, 0.5, 0.25: alpha Lz = 1 aniso 9.9e-8, 6.4e-9, 4.1e-10, 2.6e-11, uniform
    1.2e-6, 7.8e-8, 5.0e-9, 3.2e-10; alpha Lz = 3 aniso 2.3e-5, 1.6e-6, 1.0e-7, 6.4e-9, uniform 2.5e-4, 1.8e-5, 1.2e-6,
    7.8e-8"""
    mesh = MESHES[kind](SHAPE)
    errs, want, m = P.hyperbolic_errors(lib_run, mesh, alpha_lz)
    assert_order(errs, f"{kind} hyperbolic, alpha Lz = {alpha_lz}, Q-perp")
    ratio = np.nanmax(np.abs(m.q / m.q_perp - 1.0))
    print("Q-perp from", want.min(), "to", want.max(), "max |Q / Q-perp - 1|", ratio)
    if alpha_lz > 1.0:
        assert ratio > 0.5 and want.max() / want.min() > 50.0


# ---------------------------------------------------------------------------------------------------------------
# 5. against finite differences of VecPot.trace
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_against_finite_differences_of_trace(hip, kind):
    """Q-perp against the Q-perp of four neighbour lines of VecPot.trace per seed, traced in both directions.  The
    bound is the restatement's own gap (trace_numpy and squash_perp_numpy on the CPU) at the best of three offsets,
    times two.  On these seeds Q and Q-perp differ by up to 16 %: a Q-perp that returned Q would miss by two orders of
    magnitude"""
    best = []
    for shape in FD_SHAPES[kind]:
        mesh = MESHES[kind](shape)
        table = [P.fd_gap(P.model_run, P.numpy_tracer, mesh, d) for d in P.FD_DELTAS]
        gaps = [row[0] for row in table]
        i = int(np.argmin(gaps))
        assert table[i][1] <= 0.10, "more than 10 % of the patch left out in the restatement"
        gap, left_out, q_perp, q = P.fd_gap(lib_run, lib_trace, mesh, P.FD_DELTAS[i])
        print(kind, shape, "restatement gaps at delta = 1e-3, 1e-4, 1e-5:", gaps, "left out", [r[1] for r in table],
              "device gap", gap, "at delta", P.FD_DELTAS[i], "max |Q / Q-perp - 1|", np.abs(q / q_perp - 1).max())
        assert left_out <= 0.10
        assert gap <= 2.0 * gaps[i]
        assert np.abs(q / q_perp - 1).max() > 50.0 * gap
        best.append(gap)
    assert best[1] < best[0], best


# ---------------------------------------------------------------------------------------------------------------
# 6. Q-perp is constant along a line
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_q_perp_is_constant_along_a_line(hip, kind):
    """the spread of Q-perp over four points of one line at three resolutions: the restatement's falls with h, the
    device's is within 3x the restatement's"""
    model, dev = [], []
    for shape in CONST_SHAPES[kind]:
        mesh = MESHES[kind](shape)
        sm, qm = along_line_spread(P.perp_as_q(P.model_run), forward_tracer, mesh)
        sd, _qd = along_line_spread(P.perp_as_q(lib_run), lib_trace, mesh)
        model.append(sm)
        dev.append(sd)
        assert qm.max() / qm.min() > 1.2, "Q-perp does not vary over the patch: the test shows nothing"
    print(kind, "spread of Q-perp along a line, restatement:", model, "device:", dev)
    assert model[0] > model[1] > model[2], model
    for sm, sd in zip(model, dev):
        assert sd <= 3.0 * sm, (model, dev)


# ---------------------------------------------------------------------------------------------------------------
# 7. failure ends and lane pairing
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_failure_ends(hip, kind):
    P.check_failure_ends(lib_run, lib_trace, MESHES[kind]([20, 17, 23]))


def test_lane_pairing_and_seed_order(hip):
    """1, 31, 32, 33 and 65 seeds: the workgroup of 64 lanes ends after seed 32, and the forward lane reads its
    partner's end by a wave exchange - the last seed's values are those of that seed alone, and the same seeds in
    reversed order give the same bits"""
    import ndsm_amd
    mesh = aniso_mesh([33, 22, 27])
    b = abc(mesh)
    g = abc(mesh, k=0.7 * np.pi, phase=0.3)
    rng = np.random.default_rng(2204)
    seeds = np.concatenate([inner_seeds(mesh, rng, 59), face_seeds(mesh, rng, 1)])
    names = ("q", "q_perp") + LINE_FIELDS
    kw = dict(g=g, integrand=1, step=0.37, max_steps=250)
    V = ndsm_amd.VecPot(*mesh)
    try:
        ref = V.squashing_perp(b, seeds, **kw)
        assert np.isfinite(ref.q_perp).sum() >= 40
        for n in (1, 31, 32, 33, 65):
            S = seeds[:n]
            m = V.squashing_perp(b, S, **kw)
            rev = V.squashing_perp(b, S[::-1], device=True, **kw)
            one = V.squashing_perp(b, S[n - 1:n], **kw)
            for k in names:
                x, r, y, o = getattr(ref, k), getattr(rev, k), getattr(m, k), getattr(one, k)
                if x.ndim == 1:
                    assert same(y, x[:n]) and same(r, y[::-1]) and same(o, y[n - 1:n]), (k, n)
                else:
                    assert same(y, x[:, :n]) and same(r, y[:, ::-1]) and same(o, y[:, n - 1:n]), (k, n)
    finally:
        V.close()
    # the one-shot form, and the twist map against its parts: NaN where q_perp is
    one = ndsm_amd.perpendicular_squashing(*mesh, b, seeds, **kw)
    assert same(one.q_perp, ref.q_perp) and same(one.q, ref.q) and same(one.integral, ref.integral)
    tw = lib_run(mesh, b, seeds, twist=True, step=0.37, max_steps=250)
    assert same(tw.q_perp, ref.q_perp) and np.array_equal(np.isnan(tw.twist), np.isnan(tw.q_perp))
    ok = ~np.isnan(tw.q_perp)
    assert np.array_equal(tw.twist[ok], ((tw.integral[0] + tw.integral[1]) / (4.0 * np.pi))[ok])
    # an oblique cut: seed_cut's seeds go in as they are, the points outside the box come back with OUTSIDE
    lo, _h, hi, _n = P.box(mesh)
    cut = ndsm_amd.seed_cut(*mesh, lo + 0.2 * (hi - lo), [0.9 * (hi[0] - lo[0]), 0.0, 0.3 * (hi[2] - lo[2])],
                            [0.0, 0.7 * (hi[1] - lo[1]), 0.2 * (hi[2] - lo[2])], 6, 5)
    m = lib_run(mesh, b, cut, max_steps=250)
    inside = np.all((cut >= lo) & (cut <= hi), axis=1)
    assert m.q_perp.shape == (30,) and (~inside).sum() >= 3 and inside.sum() >= 15
    assert np.all(m.status[:, ~inside] == P.OUTSIDE) and np.all(m.status[:, inside] != P.OUTSIDE)


@pytest.mark.parametrize("shape,twist", [([4, 5, 4], False), ([4, 4, 4], True)])
@pytest.mark.parametrize("kind", KINDS)
def test_smallest_meshes(hip, kind, shape, twist):
    """the smallest meshes a handle takes (ndsm_hip_vecpot_create asks for four points per axis; the kernel itself
    for two, and three for the curl of twist=True, which no public entry reaches), without G and with twist=True: the
    uniform field, Q-perp = 2 and T_w = 0 (to rounding) at every seed, and the restatement bit for bit"""
    mesh = MESHES[kind](shape)
    b = P.uniform_b(mesh)
    rng = np.random.default_rng(2205)
    seeds = np.concatenate([inner_seeds(mesh, rng, 20), face_seeds(mesh, rng, 2)])
    m = lib_run(mesh, b, seeds, twist=twist)
    assert np.all(np.isin(m.status, list(FACES))) and np.abs(m.q_perp - 2.0).max() <= 1e-12
    if twist:
        # curl_h of a uniform field is rounding alone, a few ulp(|B|) / h per entry (exactly 0 only where the
        # differences' weights cancel exactly): over a line of length <= 3 box widths, / 4 pi, that stays below 1e-14
        assert np.abs(m.twist).max() <= 1e-14
    else:
        want = P.squash_perp_numpy(mesh, b, None, seeds, 0.5, int(np.ceil(4.0 * sum(shape) / 0.5)))
        for name, y in zip(("q", "q_perp") + LINE_FIELDS, want):
            assert same(getattr(m, name), y), name


# ---------------------------------------------------------------------------------------------------------------
# 8. the C entries
# ---------------------------------------------------------------------------------------------------------------
def test_c_entries_reject_bad_scalars(hip):
    """9002 for a NULL handle or array (qperp among them), 9004 for a scalar out of range, the host outputs cleared;
    no seeds: 0, and nothing is touched"""
    import ndsm_amd
    mesh = aniso_mesh([12, 11, 10])
    b = np.ascontiguousarray(abc(mesh))
    seeds = np.ascontiguousarray(inner_seeds(mesh, np.random.default_rng(1), 4))
    V = ndsm_amd.VecPot(*mesh)
    try:
        L = V.L

        def call(h, bb, integrand, ns, step, max_steps, drop=None):
            out = [np.full(4, 7.0), np.full(4, 7.0), np.full((2, 4, 3), 7.0), np.full((2, 4), 7.0),
                   np.full((2, 4), 7.0),
                   np.full((2, 4), 7, dtype=np.int32), np.full((2, 4), 7, dtype=np.int32)]
            ptrs = [None if i == drop else a.ctypes.data for i, a in enumerate(out)]
            rc = L.ndsm_hip_vecpot_squash_perp(h, bb, None, integrand, ns, seeds.ctypes.data, step, max_steps, *ptrs)
            return rc, out
        rc, out = call(V.h, b.ctypes.data, 0, 4, 0.5, 10)
        assert rc == 0 and np.all(out[5] != 7) and np.all(out[1] != 7.0)
        for args in ((V.h, b.ctypes.data, 0, 4, 0.0, 10), (V.h, b.ctypes.data, 0, 4, -1.0, 10),
                     (V.h, b.ctypes.data, 0, 4, 0.5, 0), (V.h, b.ctypes.data, 2, 4, 0.5, 10),
                     (V.h, b.ctypes.data, -1, 4, 0.5, 10), (V.h, b.ctypes.data, 1, 4, float("nan"), 10)):
            rc, out = call(*args)
            assert rc == 9004, args
            assert all(np.all(a == 0) for a in out), args
        assert call(V.h, b.ctypes.data, 0, -1, 0.5, 10)[0] == 9004
        assert call(None, b.ctypes.data, 0, 4, 0.5, 10)[0] == 9002
        rc, out = call(V.h, None, 0, 4, 0.5, 10)
        assert rc == 9002 and np.all(out[5] == 0) and np.all(out[1] == 0)
        # a NULL qperp (and a NULL q) with seeds: 9002, the arrays that are there cleared
        for drop in (1, 0):
            rc, out = call(V.h, b.ctypes.data, 0, 4, 0.5, 10, drop=drop)
            assert rc == 9002, drop
            assert all(np.all(a == 0) for i, a in enumerate(out) if i != drop)
        rc, out = call(V.h, None, 0, 0, 0.5, 10, drop=1)
        assert rc == 0 and all(np.all(a == 7) for a in out)            # no seeds: nothing is looked at or touched
        # the device entry: the same codes
        dev = L.ndsm_hip_vecpot_squash_perp_device
        assert dev(V.h, None, None, 0, 4, None, 0.5, 10, *([None] * 7)) == 9002
        assert dev(V.h, None, None, 0, 0, None, 0.5, 10, *([None] * 7)) == 0
        assert dev(V.h, None, None, 2, 0, None, 0.5, 10, *([None] * 7)) == 9004
    finally:
        V.close()


@pytest.mark.parametrize("ns", ([4, 4, 4], [7, 5, 9]), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mname", KINDS)
def test_device_entry_on_offset_arrays(hip, mname, ns):
    """the device entry on views into one larger allocation (device_arena.Arena: 8 mod 16 for doubles, 4 mod 8 for
    int32, NaN bands beside the fields, guard bytes checked): the restatement bit for bit, for 1, 32, 33 and 65
    seeds"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b, g = abc(mesh), abc(mesh, k=0.7 * np.pi, phase=0.3)
    rng = np.random.default_rng(5)
    seeds = np.concatenate([inner_seeds(mesh, rng, 29), face_seeds(mesh, rng, 2)])
    step, max_steps, fill = 0.37, 300, 7.0
    want = {k: P.squash_perp_numpy(mesh, b, g, seeds, step, max_steps, k) for k in (0, 1)}
    assert np.isfinite(want[0][1]).all()
    V = ndsm_amd.VecPot(*mesh)
    try:
        for count in (1, 32, 33, 65):
            idx = np.arange(count) % len(seeds)
            S = np.ascontiguousarray(seeds[idx])
            nl = 2 * count
            for integrand in (0, 1):
                slots = [slot("B", b.reshape(-1), field=True), slot("G", g.reshape(-1), field=True), slot("seeds", S),
                         slot("q", np.full(count, fill), output=True), slot("qperp", np.full(count, fill), output=True),
                         slot("ends", np.full((nl, 3), fill), output=True),
                         slot("length", np.full(nl, fill), output=True),
                         slot("integral", np.full(nl, fill), output=True),
                         slot("status", np.full(nl, 7, dtype=np.int32), output=True),
                         slot("nsteps", np.full(nl, 7, dtype=np.int32), output=True)]
                A = Arena(LibTransport(V.L), slots)
                out = A.run(lambda dB, dG, dS, *p: V.L.ndsm_hip_vecpot_squash_perp_device(
                    V.h, dB, dG, integrand, count, dS, step, max_steps, *p))
                assert A.rc == 0, hip.last_error(V.L)
                got = out[-7:]
                w = want[integrand]
                assert same(got[0], w[0][idx]) and same(got[1], w[1][idx]), (count, integrand)
                for k in range(2, 7):
                    y = w[k][:, idx]
                    assert same(got[k], y.reshape((nl,) + y.shape[2:])), (count, integrand, k)
    finally:
        V.close()
