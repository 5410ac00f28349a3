"""GPU tests of the ten ndsm_hip_vecpot_*_device entries on caller arrays as a caller has them (run with -m gpu on an
MI355X): views into one larger allocation, aligned as far as their element type asks (doubles and int64 at 8 mod 16,
int32 at 4 mod 8), with guard bands on both sides - NaN beside the input fields - and at the smallest shapes the handle
takes (4 points per axis).  device_arena.Arena lays the arrays out, runs the entry and fails when a byte outside the
declared outputs, or a slot past the records written, has changed (test_device_arena.py tests that it does).  The
yardsticks are the suite's own: null_model.nulls_numpy, line_model.trace_numpy / squash_numpy and
test_gpu_devore.devore_numpy bit for bit, and for the entries with solves the host entry of the same call, bit for bit
(nothing in the library branches on a caller's address).  Every test runs on golden_inputs.uniform_mesh and aniso_mesh.

A stray access lands inside the test's own allocation and shows as a failed comparison, never as a fault: no test aims
an access outside an allocation."""
import ctypes

import numpy as np
import pytest

from device_arena import Arena, LibTransport, slot
from golden_inputs import analytic_case, aniso_mesh, uniform_mesh
from line_model import FACES, abc, face_seeds, inner_seeds, sheared, squash_numpy, trace_numpy
from null_model import nulls_numpy
from test_gpu_devore import assert_reduction, devore_numpy, flux
from test_gpu_nulls import assert_bitwise
from test_gpu_project import case as project_case

pytestmark = pytest.mark.gpu

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
IDS = lambda s: "x".join(map(str, s))   # noqa: E731
VC_TOL = 1e-12
FILL = 7

_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def arena(V, slots, plain=False):
    return Arena(LibTransport(V.L), slots, plain=plain)


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), what


# ---------------------------------------------------------------------------------------------------------------
# a. nulls
# ---------------------------------------------------------------------------------------------------------------
# N = 64: one mask word; 80: a second, partial word; 125, 315, 729: odd, node_code_k's one-node tail and components
# that start at 8 and 0 mod 16 in turn; 512: exactly one node_code_k workgroup; 1340: four Newton workgroups
NULL_SHAPES = ([4, 4, 4], [4, 4, 5], [5, 5, 5], [7, 5, 9], [9, 9, 9], [8, 8, 8], [67, 5, 4], [5, 4, 67])
ODD_N = ([5, 5, 5], [7, 5, 9], [9, 9, 9])
# (candidates, nulls) of nulls_numpy on the noise below, the same on both meshes
NULL_COUNTS = {"4x4x4": (27, 15), "5x5x5": (64, 23), "7x5x9": (191, 60), "9x9x9": (504, 174), "5x4x67": (781, 245),
               "67x5x4": (775, 278)}


def noise(ns):
    """the first draw of default_rng(5): white noise, nearly every cell a candidate and a third of them with a null"""
    return np.random.default_rng(5).uniform(-1.0, 1.0, (3, ns[2], ns[1], ns[0]))


def null_slots(b, cap, fill=FILL):
    m = cap
    return [slot("B", np.ascontiguousarray(b, dtype=np.float64).reshape(-1), field=True),
            slot("cell", np.full(m, fill, dtype=np.int64), output=True),
            slot("pos", np.full((m, 3), float(fill)), output=True),
            slot("jac", np.full((m, 3, 3), float(fill)), output=True),
            slot("det", np.full(m, float(fill)), output=True),
            slot("resid", np.full(m, float(fill)), output=True),
            slot("sign", np.full(m, fill, dtype=np.int32), output=True),
            slot("iters", np.full(m, fill, dtype=np.int32), output=True)]


def nulls_device(hip, V, b, cap, plain=False):
    """one call of ndsm_hip_vecpot_nulls_device with capacity cap on arrays of exactly cap slots: the tuple of
    nulls_numpy's layout, cut to the records written.  The slots past them must come back as they went up (the arena
    checks it); with cap = 0 every record pointer is NULL."""
    counts = np.full(2, FILL, dtype=np.int64)
    slots = null_slots(b, cap) if cap > 0 else null_slots(b, 1)[:1]

    def call(dB, *rec):
        return V.L.ndsm_hip_vecpot_nulls_device(V.h, dB, cap, counts.ctypes.data, *(rec if cap > 0 else [None] * 7))

    def written():
        n = min(max(int(counts[1]), 0), cap)
        return {s.name: n for s in slots[1:]}
    A = arena(V, slots, plain=plain)
    out = A.run(call, written=written)
    assert A.rc == 0, hip.last_error(V.L)
    n = min(int(counts[1]), cap)
    if cap == 0:
        return (counts,)
    return (counts,) + tuple(a[:n] for a in out[1:])


def nulls_host(hip, V, b, cap):
    counts = np.full(2, FILL, dtype=np.int64)
    B = np.ascontiguousarray(b, dtype=np.float64).reshape(-1).copy()
    out = [s.array.copy() for s in null_slots(b, cap)[1:]]
    rc = V.L.ndsm_hip_vecpot_nulls(V.h, B.ctypes.data, cap, counts.ctypes.data, *[a.ctypes.data for a in out])
    assert rc == 0, hip.last_error(V.L)
    n = min(int(counts[1]), cap)
    for a in out:
        assert not np.any(a[n:])                         # the host entry clears the slots past the records
    return (counts,) + tuple(a[:n] for a in out)


@pytest.mark.parametrize("ns", NULL_SHAPES, ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_nulls_on_offset_arrays(hip, mname, ns):
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b = noise(ns)
    want = nulls_numpy(mesh, b, 10 ** 6)
    nc, nf = int(want[0][0]), int(want[0][1])
    print(mname, ns, "candidates", nc, "nulls", nf)
    assert nf >= 2 and nc > nf
    if IDS(ns) in NULL_COUNTS:
        assert (nc, nf) == NULL_COUNTS[IDS(ns)]
    V = ndsm_amd.VecPot(*mesh)
    try:
        for cap in (nf + 3, nf, nf - 1, 1):
            got = nulls_device(hip, V, b, cap)
            cut = (want[0],) + tuple(a[:cap] for a in want[1:])
            assert_bitwise(got, cut, "%s %s capacity %d" % (mname, ns, cap))
            assert len(got[1]) == min(nf, cap) and np.all(np.diff(got[1]) > 0)
        assert np.array_equal(nulls_device(hip, V, b, 0)[0], want[0])
        if ns in ODD_N:
            # arrays in allocations of their own, and the host entry: an odd-N finding and an alignment finding can
            # be told apart
            assert_bitwise(nulls_device(hip, V, b, nf + 3, plain=True), want, "%s %s plain" % (mname, ns))
            assert_bitwise(nulls_host(hip, V, b, nf + 3), want, "%s %s host entry" % (mname, ns))
    finally:
        V.close()


@pytest.mark.parametrize("ns,ncand", (([5, 5, 5], 64), ([5, 5, 17], 256), ([5, 5, 18], 272)), ids=lambda v: IDS(v) if isinstance(v, list) else str(v))
@pytest.mark.parametrize("mname", list(MESHES))
def test_nulls_zero_field_on_offset_arrays(hip, mname, ns, ncand):
    """every cell a candidate - one, exactly four and five mask words of candidates (a Newton workgroup holds four) - and
    no null: the counts, and nothing written"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b = np.zeros((3, ns[2], ns[1], ns[0]))
    want = nulls_numpy(mesh, b, 16)
    assert (int(want[0][0]), int(want[0][1])) == (ncand, 0)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for cap in (4, 1, 0):
            got = nulls_device(hip, V, b, cap)          # (written = 0 records: every slot must be as it went up)
            assert np.array_equal(got[0], want[0]), (cap, got[0])
        got = nulls_device(hip, V, b, 4, plain=True)
        assert np.array_equal(got[0], want[0])
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------
# b. trace and squash
# ---------------------------------------------------------------------------------------------------------------
LINE_SHAPES = ([4, 4, 4], [5, 5, 5], [7, 5, 9], [67, 5, 4], [5, 4, 67])
# one lane; exactly one wave; a wave plus one; two waves (one block of 64 in a single direction, 128 lines in both);
# a block plus one
SEED_COUNTS = (1, 32, 33, 64, 65)
STEP, MAX_STEPS = 0.37, 300
_LINES = {}


def line_case(mname, ns):
    """(mesh, b, g, seeds) and the restatements' results for the 41 seeds, computed once per mesh and shape: every line
    depends on its own seed only, so any seed list made of these has its rows among them.  The seeds come from a FRESH
    default_rng(5) (not the generator after the noise draw of the nulls tests): 29 inside, 2 on each face."""
    key = (mname, IDS(ns))
    if key not in _LINES:
        mesh = MESHES[mname](ns)
        b, g = abc(mesh), abc(mesh, k=0.7 * np.pi, phase=0.3)
        rng = np.random.default_rng(5)
        seeds = np.concatenate([inner_seeds(mesh, rng, 29), face_seeds(mesh, rng, 2)])
        tr = {(sgn, withg): trace_numpy(mesh, b, g if withg else None, seeds, STEP, MAX_STEPS, sgn)
              for sgn in (1.0, -1.0) for withg in (True, False)}
        sq = {k: squash_numpy(mesh, b, g, seeds, STEP, MAX_STEPS, k) for k in (0, 1)}
        # the lines of the two directions together end on all six faces, and Q is finite at every seed
        ends = np.concatenate([tr[(1.0, True)][3], tr[(-1.0, True)][3]])
        assert set(FACES) <= set(ends.tolist()) and len(seeds) == 41
        assert np.isfinite(sq[0][0]).all() and set(FACES) <= set(sq[0][4].reshape(-1).tolist())
        _LINES[key] = (mesh, b, g, seeds, tr, sq)
    return _LINES[key]


def line_slots(b, g, S, nl, q=False):
    f = float(FILL)
    return ([slot("B", b.reshape(-1), field=True)] + ([slot("G", g.reshape(-1), field=True)] if g is not None else []) +
            [slot("seeds", S)] + ([slot("q", np.full(len(S), f), output=True)] if q else []) +
            [slot("ends", np.full((nl, 3), f), output=True), slot("length", np.full(nl, f), output=True),
             slot("integral", np.full(nl, f), output=True), slot("status", np.full(nl, FILL, dtype=np.int32), output=True),
             slot("nsteps", np.full(nl, FILL, dtype=np.int32), output=True)])


@pytest.mark.parametrize("ns", LINE_SHAPES, ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_trace_on_offset_arrays(hip, mname, ns):
    import ndsm_amd
    mesh, b, g, seeds, tr, _sq = line_case(mname, ns)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for count in SEED_COUNTS:
            idx = np.arange(count) % len(seeds)          # the first seeds of the list, repeated
            S = np.ascontiguousarray(seeds[idx])
            for direction in (1, -1, 0):
                nl = count * (2 if direction == 0 else 1)
                sgns = (1.0, -1.0) if direction == 0 else (float(direction),)
                for withg in (True, False):
                    slots = line_slots(b, g if withg else None, S, nl)

                    def call(dB, *p):
                        dG, p = (p[0], p[1:]) if withg else (None, p)
                        return V.L.ndsm_hip_vecpot_trace_device(V.h, dB, dG, count, p[0], STEP, MAX_STEPS, direction,
                                                                *p[1:])
                    A = arena(V, slots)
                    out = A.run(call)
                    assert A.rc == 0, hip.last_error(V.L)
                    got = out[-5:]
                    what = "%s %s %d seeds, direction %d, G %s" % (mname, ns, count, direction, withg)
                    for k, name in enumerate(("ends", "length", "integral", "status", "nsteps")):
                        want = np.concatenate([tr[(sgn, withg)][k][idx] for sgn in sgns])
                        same_bits(got[k], want, what + ": " + name)
                    if not withg:
                        assert not np.any(got[2])
    finally:
        V.close()


@pytest.mark.parametrize("ns", LINE_SHAPES, ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_squash_on_offset_arrays(hip, mname, ns):
    import ndsm_amd
    mesh, b, g, seeds, _tr, sq = line_case(mname, ns)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for count in SEED_COUNTS:
            idx = np.arange(count) % len(seeds)
            S = np.ascontiguousarray(seeds[idx])
            for integrand in (0, 1):
                slots = line_slots(b, g, S, 2 * count, q=True)
                A = arena(V, slots)
                out = A.run(lambda dB, dG, dS, *p: V.L.ndsm_hip_vecpot_squash_device(
                    V.h, dB, dG, integrand, count, dS, STEP, MAX_STEPS, *p))
                assert A.rc == 0, hip.last_error(V.L)
                got = out[-6:]
                what = "%s %s %d seeds, integrand %d" % (mname, ns, count, integrand)
                want = sq[integrand]
                same_bits(got[0], want[0][idx], what + ": q")
                for k, name in ((1, "ends"), (2, "length"), (3, "integral"), (4, "status"), (5, "nsteps")):
                    w = want[k][:, idx]
                    same_bits(got[k], w.reshape((2 * count,) + w.shape[2:]), what + ": " + name)
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------
# c. DeVore
# ---------------------------------------------------------------------------------------------------------------
# 4x4x4: no unrolled block anywhere; 17x5x9: the base scan along x is one block of 16 and no tail, the columns one
# block of 8 up and down and no tail; 18x7x10: a block plus one tail in both; 67x5x4: two base workgroups and two
# column workgroups, the second partial; 5x4x67: eight column blocks plus a tail; 4x67x5: a y scan of 67 points
DEVORE_SHAPES = ([4, 4, 4], [17, 5, 9], [18, 7, 10], [67, 5, 4], [5, 4, 67], [4, 67, 5])


@pytest.mark.parametrize("ns", DEVORE_SHAPES, ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_devore_on_offset_arrays(hip, mname, ns):
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b = flux(mesh)
    bp = b.copy()
    bp[:, 1:-1, 1:-1, 1:-1] *= 0.5
    A, Ap = devore_numpy(b, bp, mesh)
    V = ndsm_amd.VecPot(*mesh)
    try:
        res = {}
        for plain in (False, True):
            out8 = np.full(8, np.nan)
            slots = [slot("B", b.reshape(-1), field=True), slot("Bp", bp.reshape(-1), field=True),
                     slot("A", np.full(b.shape, float(FILL)), output=True),
                     slot("Ap", np.full(b.shape, float(FILL)), output=True)]
            R = arena(V, slots, plain=plain)
            out = R.run(lambda dB, dBp, dA, dAp: V.L.ndsm_hip_vecpot_devore_device(V.h, dB, dBp, dA, dAp,
                                                                                  out8.ctypes.data_as(_dp)))
            assert R.rc == 0, hip.last_error(V.L)
            res[plain] = (out[2], out[3], out8)
    finally:
        V.close()
    for plain, (gA, gAp, out8) in res.items():
        same_bits(gA, A, "%s %s A (plain %s)" % (mname, ns, plain))
        same_bits(gAp, Ap, "%s %s A_p (plain %s)" % (mname, ns, plain))
        assert not np.any(gA[2]) and not np.any(gAp[2])                 # A_z = A_p,z = 0 exactly
        assert np.array_equal(gAp[:, -1], gA[:, -1])                    # the top plane is a copy
    # the reductions are deterministic by shape alone: the same eight scalars from offset and from plain arrays
    assert res[False][2].tobytes() == res[True][2].tobytes(), (res[False][2], res[True][2])
    assert_reduction(hip._helicity_tuple(0, res[False][2], res[False][0], res[False][1], bp), b, mesh)


# ---------------------------------------------------------------------------------------------------------------
# d. the entries with solves: the offset-pointer path against the host entry of the same call
# ---------------------------------------------------------------------------------------------------------------
SOLVE_SHAPES = ([5, 5, 5], [7, 5, 9], [9, 8, 7], [67, 5, 4])


def options(V):
    return V._options(10000, 1024, 1e-13, VC_TOL, 5, False, 0, False)


def same_options(V, dev, host, what):
    """ierr and every option slot but the wall time of the call"""
    (rc_d, io_d, ro_d), (rc_h, io_h, ro_h) = dev, host
    assert rc_d == rc_h and rc_d < 9000, (what, rc_d, rc_h)
    assert np.array_equal(io_d, io_h), (what, io_d, io_h)
    keep = np.arange(16) != V.L.get_ropt_tim()
    assert ro_d[keep].tobytes() == ro_h[keep].tobytes(), (what, ro_d, ro_h)


@pytest.mark.parametrize("ns", SOLVE_SHAPES, ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_solve_entries_on_offset_arrays(hip, mname, ns):
    """ndsm_hip_vecpot_solve_device and ndsm_hip_vecpot_solve_field_device (A, B both in and out): test_gpu_parity's
    analytic field (the values of the uniform mesh of that shape) with unbalanced fluxes and a random guess;
    test_gpu_field's ABC field (line_model.abc with its defaults: the same expression) and guess"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    L = ndsm_amd.load_library()
    _x, _y, _z, _A1, b0 = analytic_case(ns)
    cases = {"solve": (b0 + 0.3 * np.random.default_rng(5).uniform(-1, 1, b0.shape),
                       np.random.default_rng(6).uniform(-1, 1, b0.shape)),
             "solve_field": (abc(mesh), 0.01 * np.cos(abc(mesh)))}
    V = ndsm_amd.VecPot(*mesh)
    try:
        for name, (b, a0) in cases.items():
            host_entry = getattr(L, "ndsm_hip_vecpot_" + name)
            dev_entry = getattr(L, "ndsm_hip_vecpot_" + name + "_device")
            io_h, ro_h = options(V)
            A, B = a0.reshape(-1).copy(), b.reshape(-1).copy()
            rc_h = host_entry(V.h, io_h.ctypes.data_as(_ip), ro_h.ctypes.data_as(_dp), A.ctypes.data_as(_dp),
                              B.ctypes.data_as(_dp))
            for plain in (False, True):
                io_d, ro_d = options(V)
                R = arena(V, [slot("A", a0.reshape(-1), output=True, field=True),
                              slot("B", b.reshape(-1), output=True, field=True)], plain=plain)
                gA, gB = R.run(lambda dA, dB: dev_entry(V.h, io_d.ctypes.data_as(_ip), ro_d.ctypes.data_as(_dp), dA, dB))
                what = "%s %s %s (plain %s)" % (name, mname, ns, plain)
                same_options(V, (R.rc, io_d, ro_d), (rc_h, io_h, ro_h), what)
                same_bits(gA, A, what + ": A")
                same_bits(gB, B, what + ": B")
            assert np.isfinite(A).all() and np.isfinite(B).all() and not np.array_equal(A, a0.reshape(-1))
    finally:
        V.close()


@pytest.mark.parametrize("ns", SOLVE_SHAPES, ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_helicity_on_offset_arrays(hip, mname, ns):
    """ndsm_hip_vecpot_helicity_device: B is the caller's and read only, A, A_p, B_p and the eight scalars come out
    (test_gpu_field's ABC field)"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    L = ndsm_amd.load_library()
    b = abc(mesh)
    V = ndsm_amd.VecPot(*mesh)
    try:
        io_h, ro_h = options(V)
        B = b.reshape(-1).copy()
        host = [np.full(B.size, float(FILL)) for _ in range(3)]
        out_h = np.full(8, np.nan)
        rc_h = L.ndsm_hip_vecpot_helicity(V.h, io_h.ctypes.data_as(_ip), ro_h.ctypes.data_as(_dp), B.ctypes.data_as(_dp),
                                          *[a.ctypes.data_as(_dp) for a in host], out_h.ctypes.data_as(_dp))
        assert np.array_equal(B, b.reshape(-1))
        for plain in (False, True):
            io_d, ro_d = options(V)
            out_d = np.full(8, np.nan)
            slots = [slot("B", B, field=True)] + [slot(k, np.full(B.size, float(FILL)), output=True)
                                                  for k in ("A", "Ap", "Bp")]
            R = arena(V, slots, plain=plain)
            got = R.run(lambda dB, dA, dAp, dBp: L.ndsm_hip_vecpot_helicity_device(
                V.h, io_d.ctypes.data_as(_ip), ro_d.ctypes.data_as(_dp), dB, dA, dAp, dBp, out_d.ctypes.data_as(_dp)))
            what = "helicity %s %s (plain %s)" % (mname, ns, plain)
            same_options(V, (R.rc, io_d, ro_d), (rc_h, io_h, ro_h), what)
            for k, name in enumerate(("A", "A_p", "B_p")):
                same_bits(got[1 + k], host[k], what + ": " + name)
            assert out_d.tobytes() == out_h.tobytes(), (what, out_d, out_h)
        assert np.isfinite(out_h).all() and all(np.isfinite(a).all() for a in host)
    finally:
        V.close()


@pytest.mark.parametrize("ns", SOLVE_SHAPES, ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_project_on_offset_arrays(hip, mname, ns):
    """ndsm_hip_vecpot_project_device (B in and out; phi out, or absent), on test_gpu_project's field"""
    import ndsm_amd
    mesh, b = project_case(ns, meshf=MESHES[mname])
    L = ndsm_amd.load_library()
    V = ndsm_amd.VecPot(*mesh)
    try:
        io_h, ro_h = options(V)
        B = b.reshape(-1).copy()
        phi = np.full(B.size // 3, float(FILL))
        out_h = np.full(4, np.nan)
        rc_h = L.ndsm_hip_vecpot_project(V.h, io_h.ctypes.data_as(_ip), ro_h.ctypes.data_as(_dp), B.ctypes.data_as(_dp),
                                         phi.ctypes.data_as(_dp), out_h.ctypes.data_as(_dp))
        for plain, with_phi in ((False, True), (False, False), (True, True)):
            io_d, ro_d = options(V)
            out_d = np.full(4, np.nan)
            slots = [slot("B", b.reshape(-1), output=True, field=True)]
            if with_phi:
                slots.append(slot("phi", np.full(B.size // 3, float(FILL)), output=True))
            R = arena(V, slots, plain=plain)
            got = R.run(lambda dB, dphi=None: L.ndsm_hip_vecpot_project_device(
                V.h, io_d.ctypes.data_as(_ip), ro_d.ctypes.data_as(_dp), dB, dphi, out_d.ctypes.data_as(_dp)))
            what = "project %s %s (plain %s, phi %s)" % (mname, ns, plain, with_phi)
            same_options(V, (R.rc, io_d, ro_d), (rc_h, io_h, ro_h), what)
            same_bits(got[0], B, what + ": B")
            if with_phi:
                same_bits(got[1], phi, what + ": phi")
            assert out_d.tobytes() == out_h.tobytes(), (what, out_d, out_h)
        assert np.isfinite(out_h).all() and np.isfinite(B).all() and not np.array_equal(B, b.reshape(-1))
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------
# e. the two Grad-Rubin entries: the solve for a prescribed current and the iteration
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", SOLVE_SHAPES, ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_solve_current_on_offset_arrays(hip, mname, ns):
    """ndsm_hip_vecpot_solve_current_device: J is read only, A and B go in and come out (line_model's sheared field for
    B.n, a third of the ABC field as the current, test_gpu_field's guess)"""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    L = ndsm_amd.load_library()
    b, j, a0 = sheared(mesh), 0.3 * abc(mesh), 0.01 * np.cos(abc(mesh))
    V = ndsm_amd.VecPot(*mesh)
    try:
        io_h, ro_h = options(V)
        J, A, B = j.reshape(-1).copy(), a0.reshape(-1).copy(), b.reshape(-1).copy()
        rc_h = L.ndsm_hip_vecpot_solve_current(V.h, io_h.ctypes.data_as(_ip), ro_h.ctypes.data_as(_dp),
                                               J.ctypes.data_as(_dp), A.ctypes.data_as(_dp), B.ctypes.data_as(_dp))
        assert np.array_equal(J, j.reshape(-1))
        for plain in (False, True):
            io_d, ro_d = options(V)
            R = arena(V, [slot("J", j.reshape(-1), field=True), slot("A", a0.reshape(-1), output=True, field=True),
                          slot("B", b.reshape(-1), output=True, field=True)], plain=plain)
            _gJ, gA, gB = R.run(lambda dJ, dA, dB: L.ndsm_hip_vecpot_solve_current_device(
                V.h, io_d.ctypes.data_as(_ip), ro_d.ctypes.data_as(_dp), dJ, dA, dB))
            what = "solve_current %s %s (plain %s)" % (mname, ns, plain)
            same_options(V, (R.rc, io_d, ro_d), (rc_h, io_h, ro_h), what)
            same_bits(gA, A, what + ": A")
            same_bits(gB, B, what + ": B")
        assert np.isfinite(A).all() and np.isfinite(B).all() and not np.array_equal(A, a0.reshape(-1))
    finally:
        V.close()


def nlfff_host(V, b, alpha0, a0, start, passes, max_steps, with_status=True):
    """one call of ndsm_hip_vecpot_nlfff on host arrays: (rc, ioptc, ropt), [B, A, alpha, status], hist, niter"""
    io, ro = options(V)
    B, A, al0 = b.reshape(-1).copy(), a0.reshape(-1).copy(), alpha0.reshape(-1).copy()
    alpha, status = np.full(B.size // 3, float(FILL)), np.full(B.size // 3, FILL, dtype=np.int32)
    hist, niter = np.full((passes, 4), np.nan), ctypes.c_int(FILL)
    rc = V.L.ndsm_hip_vecpot_nlfff(V.h, io.ctypes.data_as(_ip), ro.ctypes.data_as(_dp), B.ctypes.data, al0.ctypes.data,
                                   1, start, passes, 0.0, 0.5, max_steps, A.ctypes.data, alpha.ctypes.data,
                                   status.ctypes.data if with_status else None, hist.ctypes.data_as(_dp),
                                   ctypes.byref(niter))
    assert np.array_equal(al0, alpha0.reshape(-1))
    return (rc, io, ro), [B, A, alpha, status], hist, niter.value


@pytest.mark.parametrize("ns", SOLVE_SHAPES, ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_nlfff_on_offset_arrays(hip, mname, ns):
    """ndsm_hip_vecpot_nlfff_device: B and A go in and come out, alpha0 (a 2-D array, NaN beside it) is read only,
    alpha and status come out; hist and niter_out stay on the host.  The fields B^k and B^{k+1} alternate between the
    caller's B and the handle's own, so the last one lies in the caller's array after an even number of passes and is
    copied there after an odd one: 1, 2 and 3 passes, from the potential start (A is not read) and from the given one
    (the sheared field, boundary_alpha's alpha0, a small guess).  Once without a status array: the count of the
    history is taken in a scratch array, and nothing of the caller's is written in its place."""
    import ndsm_amd
    mesh = MESHES[mname](ns)
    L = ndsm_amd.load_library()
    b, a0 = sheared(mesh), 0.01 * np.cos(abc(mesh))
    alpha0 = ndsm_amd.boundary_alpha(mesh[0], mesh[1], b, 1e-3)
    assert np.abs(alpha0).max() > 0.1
    npts = b.size // 3
    V = ndsm_amd.VecPot(*mesh)
    max_steps = V.default_max_steps(0.5)
    try:
        for start in (0, 1):
            for passes in (1, 2, 3):
                opt_h, host, hist_h, niter_h = nlfff_host(V, b, alpha0, a0, start, passes, max_steps)
                assert niter_h == passes and np.isfinite(hist_h).all() and hist_h[-1, 3] == (host[3] == 5).sum() > 0
                for plain, with_status in ((False, True), (True, True)) + (((False, False),) if passes == 2 else ()):
                    io_d, ro_d = options(V)
                    hist_d, niter_d = np.full((passes, 4), np.nan), ctypes.c_int(FILL)
                    slots = [slot("B", b.reshape(-1), output=True, field=True), slot("alpha0", alpha0, field=True),
                             slot("A", a0.reshape(-1), output=True, field=True),
                             slot("alpha", np.full(npts, float(FILL)), output=True)]
                    if with_status:
                        slots.append(slot("status", np.full(npts, FILL, dtype=np.int32), output=True))
                    R = arena(V, slots, plain=plain)
                    got = R.run(lambda dB, da0, dA, dal, dst=None: L.ndsm_hip_vecpot_nlfff_device(
                        V.h, io_d.ctypes.data_as(_ip), ro_d.ctypes.data_as(_dp), dB, da0, 1, start, passes, 0.0, 0.5,
                        max_steps, dA, dal, dst, hist_d.ctypes.data_as(_dp), ctypes.byref(niter_d)))
                    what = "nlfff %s %s start %d, %d passes (plain %s, status %s)" % (mname, ns, start, passes, plain,
                                                                                     with_status)
                    same_options(V, (R.rc, io_d, ro_d), opt_h, what)
                    same_bits(got[0], host[0], what + ": B")
                    same_bits(got[2], host[1], what + ": A")
                    same_bits(got[3], host[2], what + ": alpha")
                    if with_status:
                        same_bits(got[4], host[3], what + ": status")
                    assert niter_d.value == niter_h and hist_d.tobytes() == hist_h.tobytes(), (what, hist_d, hist_h)
                if passes == 2:
                    # the host entry without a status array: the same fields and history
                    opt_n, none, hist_n, niter_n = nlfff_host(V, b, alpha0, a0, start, passes, max_steps, with_status=False)
                    same_options(V, opt_n, opt_h, "nlfff host entry, status NULL")
                    for k in range(3):
                        same_bits(none[k], host[k], "nlfff host entry, status NULL: array %d" % k)
                    assert niter_n == niter_h and hist_n.tobytes() == hist_h.tobytes()
                    assert np.all(none[3] == FILL)
    finally:
        V.close()
