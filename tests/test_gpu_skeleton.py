"""GPU tests of the skeleton entries (run with -m gpu on an MI355X): ndsm_hip_vecpot_skeleton and
ndsm_hip_vecpot_skeleton_device against the numpy restatement skeleton_model.skeleton_numpy bit for bit, the closed
forms of skeleton_model.py through the device entries, and the chain from the nulls entries.  The C entries run on
device_arena.Arena allocations: element-aligned bases, NaN bands round B, canaries elsewhere, and every slot past the
points written must come back as it went up - a stray write shows as a failed comparison inside the test's own
allocation, never as a fault."""
import ctypes

import numpy as np
import pytest

from device_arena import Arena, LibTransport, slot
from golden_inputs import aniso_mesh, uniform_mesh
from null_model import LINEAR, nulls_numpy
from skeleton_model import (CAPTURED, NAMES, Skel, check_equals_paths, check_linear, check_no_type, check_separator,
                            check_structure, default_ring, model_run, noise_nulls, same_skel, separator_field,
                            skeleton_numpy)

pytestmark = pytest.mark.gpu

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
IDS = lambda s: "x".join(map(str, s))   # noqa: E731
SHAPES = ([4, 4, 4], [5, 5, 5], [7, 5, 9], [67, 5, 4], [5, 4, 67])
NULL_COUNTS = (1, 64, 65)               # one lane of the typing kernel; one workgroup of it; a workgroup plus one
NRINGS = (0, 1, 30, 31)                 # with two nulls: 4, 6, 64 and 66 lanes
EVERYS = (1, 3, 1000)
RADIUS, STEP, MAX_STEPS = 0.5, 0.5, 50  # (50 steps: closed and jittering lines cost nothing)
FILL = 7
_CASE = {}


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def noise_case(mname, ns):
    """white noise U(-1, 1) on the mesh and its nulls (the records of nulls_numpy), once per mesh and shape"""
    key = (mname, IDS(ns))
    if key not in _CASE:
        mesh = MESHES[mname](ns)
        b, pos, jac = noise_nulls(mesh)
        assert len(pos) >= 2, len(pos)
        _CASE[key] = (mesh, b, pos, jac)
    return _CASE[key]


def first_nulls(pos, jac, count):
    """the first `count` nulls, the list repeated where it is shorter"""
    idx = np.arange(count) % len(pos)
    return pos[idx], jac[idx]


def skel_call(hip, V, b, pos, jac, ring, radius, capture, step, max_steps, every, cap, with_bpt=True, device=True,
              plain=False):
    """One call of a C entry with capacity cap on point arrays of exactly max(cap, 1) slots, every output filled with FILL
    first.  device: on an arena (the slots past the points written must come back as they went up, the arena checks it);
    else the host entry on numpy arrays, checked the same way here.  cap = 0 passes both point arrays NULL.  Returns
    (Skel, total): the point arrays cut to the slots written, bpt as zeros when it was not passed."""
    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    jac = np.ascontiguousarray(jac, dtype=np.float64).reshape(-1, 3, 3)
    ring = np.ascontiguousarray(ring, dtype=np.float64).reshape(-1, 2)
    n, nr = len(pos), len(ring)
    nl = n * (2 + nr)
    f = float(FILL)
    total = np.full(1, FILL, dtype=np.int64)
    m = max(cap, 1)
    outs = [("kind", np.full(n, FILL, dtype=np.int32)), ("eig", np.full((n, 3), f)), ("spine", np.full((n, 3), f)),
            ("normal", np.full((n, 3), f)), ("ends", np.full((nl, 3), f)), ("length", np.full(nl, f)),
            ("status", np.full(nl, FILL, dtype=np.int32)), ("nsteps", np.full(nl, FILL, dtype=np.int32)),
            ("hit", np.full(nl, FILL, dtype=np.int32)), ("offsets", np.full(nl + 1, FILL, dtype=np.int64))]
    pts = ([("points", np.full((m, 3), f))] + ([("bpt", np.full((m, 3), f))] if with_bpt else [])) if cap > 0 else []
    passed = [name for name, _a in pts]
    entry = V.L.ndsm_hip_vecpot_skeleton_device if device else V.L.ndsm_hip_vecpot_skeleton

    def call(dB, dpos, djac, dring, *p):
        p = list(p)
        by = dict(zip(passed, p[10:]))
        return entry(V.h, dB, n, dpos, djac, nr, dring, radius, capture, step, max_steps, every, cap, *p[:10],
                     total.ctypes.data, by.get("points"), by.get("bpt"))

    def nwritten():
        return min(max(int(total[0]), 0), cap)

    def written():
        return {name: nwritten() for name in passed}

    if device:
        slots = ([slot("B", b.reshape(-1), field=True), slot("pos", pos), slot("jac", jac)] +
                 ([slot("ring", ring)] if nr else []) + [slot(name, a, output=True) for name, a in outs + pts])
        A = Arena(LibTransport(V.L), slots, plain=plain)
        if nr:
            got = A.run(call, written=written)
        else:
            got = A.run(lambda dB, dpos, djac, *p: call(dB, dpos, djac, None, *p), written=written)
        rc = A.rc
        got = dict(zip([s.name for s in slots], got))
    else:
        B = np.ascontiguousarray(b, dtype=np.float64).reshape(-1).copy()
        ins = [pos.copy(), jac.copy(), ring.copy()]
        got = {name: a.copy() for name, a in outs + pts}
        rc = call(B.ctypes.data, ins[0].ctypes.data, ins[1].ctypes.data, ins[2].ctypes.data if nr else None,
                  *[got[name].ctypes.data for name, _a in outs + pts])
        assert B.tobytes() == b.tobytes() and ins[0].tobytes() == pos.tobytes() and ins[1].tobytes() == jac.tobytes()
        assert ins[2].tobytes() == ring.tobytes()
        for name in passed:
            assert np.all(got[name][nwritten():] == f), "host entry: %s changed past the points written" % name
    assert rc == 0, (rc, hip.last_error(V.L))
    k = nwritten()
    full = {"points": np.zeros((k, 3)), "bpt": np.zeros((k, 3))}
    for name in passed:
        full[name] = got[name][:k]
    assert int(got["offsets"][-1]) == int(total[0])
    return Skel(*[got[name] for name, _a in outs], full["points"], full["bpt"]), int(total[0])


class Runner:
    """skeleton_model's runner on the C entries: a counting call (max_points = 0, both point arrays NULL), then the
    filling call of that size; one handle per mesh, closed at the end"""

    def __init__(self, hip, device=True):
        self.hip, self.device, self.handles = hip, device, {}

    def handle(self, mesh):
        import ndsm_amd
        key = tuple(np.asarray(q).tobytes() for q in mesh)
        if key not in self.handles:
            self.handles[key] = ndsm_amd.VecPot(*mesh)
        return self.handles[key]

    def __call__(self, mesh, b, pos, jac, ring, radius, capture, step, max_steps, every):
        V = self.handle(mesh)
        counted, total = skel_call(self.hip, V, b, pos, jac, ring, radius, capture, step, max_steps, every, 0,
                                   device=self.device)
        sk, total2 = skel_call(self.hip, V, b, pos, jac, ring, radius, capture, step, max_steps, every, total,
                               device=self.device)
        assert total2 == total == int(sk.offsets[-1])
        for k in range(10):
            assert sk[k].tobytes() == counted[k].tobytes(), NAMES[k]
        return sk

    def close(self):
        for V in self.handles.values():
            V.close()


@pytest.fixture()
def runner(hip):
    r = Runner(hip)
    yield r
    r.close()


# ---------------------------------------------------------------------------------------------------------------
# 1. the numpy restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", SHAPES, ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_skeleton_matches_the_restatement_bitwise(hip, runner, mname, ns):
    mesh, b, pos, jac = noise_case(mname, ns)
    V = runner.handle(mesh)
    cases = [(count, 5, 1, capture) for count in NULL_COUNTS for capture in (0.0, 0.5)]
    cases += [(2, nring, 1, capture) for nring in NRINGS for capture in (0.0, 0.5)]
    cases += [(8, 5, every, 0.5) for every in EVERYS]
    seen = set()
    for count, nring, every, capture in cases:
        P, J = first_nulls(pos, jac, count)
        ring = default_ring(nring)
        want = skeleton_numpy(mesh, b, P, J, ring, RADIUS, capture, STEP, MAX_STEPS, every)
        total = int(want.offsets[-1])
        what = "%s %s %d nulls, nring %d, every %d, capture %g" % (mname, ns, count, nring, every, capture)
        got, n = skel_call(hip, V, b, P, J, ring, RADIUS, capture, STEP, MAX_STEPS, every, total)
        assert n == total, what
        same_skel(got, want, what)
        check_structure(got, P, nring, every)
        seen |= set(got.status.tolist())
    assert len(seen) >= 3, seen
    # the host entry, bpt NULL, arrays in allocations of their own, and the counting call
    P, J = first_nulls(pos, jac, 8)
    ring = default_ring(5)
    want = skeleton_numpy(mesh, b, P, J, ring, RADIUS, 0.5, STEP, MAX_STEPS, 3)
    total = int(want.offsets[-1])
    nob = want._replace(bpt=np.zeros_like(want.bpt))
    for device in (True, False):
        for with_bpt in (True, False):
            got, _n = skel_call(hip, V, b, P, J, ring, RADIUS, 0.5, STEP, MAX_STEPS, 3, total, with_bpt=with_bpt,
                                device=device)
            same_skel(got, want if with_bpt else nob, "%s %s device %s bpt %s" % (mname, ns, device, with_bpt))
    got, _n = skel_call(hip, V, b, P, J, ring, RADIUS, 0.5, STEP, MAX_STEPS, 3, total, plain=True)
    same_skel(got, want, "%s %s plain" % (mname, ns))
    same_skel(runner(mesh, b, P, J, ring, RADIUS, 0.5, STEP, MAX_STEPS, 3), want, "%s %s counted first" % (mname, ns))


@pytest.mark.parametrize("mname", list(MESHES))
def test_odd_and_even_counts_on_both_entries(hip, runner, mname):
    """1 and 3 nulls with 0 and 1 ring seeds - 2, 3, 6 and 9 lines, so the 4-byte arrays of the host entry's staging
    buffer hold an odd and an even number of entries in front of 8-byte data -, bpt present and NULL, both entries"""
    mesh, b, pos, jac = noise_case(mname, [5, 5, 5])
    V = runner.handle(mesh)
    for count in (1, 3):
        for nring in (0, 1):
            P, J = first_nulls(pos, jac, count)
            ring = default_ring(nring)
            want = skeleton_numpy(mesh, b, P, J, ring, RADIUS, 0.5, STEP, MAX_STEPS, 1)
            assert len(want.status) == count * (2 + nring)
            total = int(want.offsets[-1])
            nob = want._replace(bpt=np.zeros_like(want.bpt))
            for device in (True, False):
                for with_bpt in (True, False):
                    got, n = skel_call(hip, V, b, P, J, ring, RADIUS, 0.5, STEP, MAX_STEPS, 1, total, with_bpt=with_bpt,
                                       device=device)
                    assert n == total
                    same_skel(got, want if with_bpt else nob,
                              "%s %d nulls, nring %d, device %s bpt %s" % (mname, count, nring, device, with_bpt))


# ---------------------------------------------------------------------------------------------------------------
# 2. capacity
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", ([5, 5, 5], [7, 5, 9]), ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_capacity(hip, runner, mname, ns):
    """offsets and total do not depend on max_points; the slots below it are those of the full result, everything at
    and beyond it is untouched (skel_call's arena and host checks)"""
    mesh, b, pos, jac = noise_case(mname, ns)
    V = runner.handle(mesh)
    P, J = first_nulls(pos, jac, 6)
    ring = default_ring(4)
    for every in (1, 2):
        want = skeleton_numpy(mesh, b, P, J, ring, RADIUS, 0.5, STEP, MAX_STEPS, every)
        total = int(want.offsets[-1])
        for device in (True, False):
            for with_bpt in (True, False):
                w = want if with_bpt else want._replace(bpt=np.zeros_like(want.bpt))
                for cap in (0, 1, total - 1, total, total + 3):
                    got, n = skel_call(hip, V, b, P, J, ring, RADIUS, 0.5, STEP, MAX_STEPS, every, cap, with_bpt=with_bpt,
                                       device=device)
                    assert n == total
                    same_skel(got, w, "%s %s capacity %d device %s" % (mname, ns, cap, device), upto=min(cap, total))
                    assert len(got.points) == min(cap, total)


# ---------------------------------------------------------------------------------------------------------------
# 3. the chain from the nulls entries, and the scratch a larger call left
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", list(MESHES))
def test_chain_from_nulls_device(hip, mname):
    """ndsm_hip_vecpot_nulls_device writes pos and jac into device arrays; ndsm_hip_vecpot_skeleton_device reads those
    very arrays: nothing crosses to the host in between, and the result is the restatement's on nulls_numpy's records"""
    import ndsm_amd
    mesh, b, _pos, _jac = noise_case(mname, [7, 5, 9])
    rec = nulls_numpy(mesh, b, 1 << 20)
    n = int(rec[0][1])
    nring = 6
    L = 2 + nring
    ring = default_ring(nring)
    want = skeleton_numpy(mesh, b, rec[2], rec[3], ring, RADIUS, 0.5, STEP, MAX_STEPS, 1)
    total = int(want.offsets[-1])
    V = ndsm_amd.VecPot(*mesh)
    lib = V.L
    B = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    host = {"cell": np.zeros(n, dtype=np.int64), "pos": np.zeros((n, 3)), "jac": np.zeros((n, 3, 3)), "det": np.zeros(n),
            "resid": np.zeros(n), "sign": np.zeros(n, dtype=np.int32), "iters": np.zeros(n, dtype=np.int32),
            "kind": np.zeros(n, dtype=np.int32), "eig": np.zeros((n, 3)), "spine": np.zeros((n, 3)),
            "normal": np.zeros((n, 3)), "ends": np.zeros((n * L, 3)), "length": np.zeros(n * L),
            "status": np.zeros(n * L, dtype=np.int32), "nsteps": np.zeros(n * L, dtype=np.int32),
            "hit": np.zeros(n * L, dtype=np.int32), "offsets": np.zeros(n * L + 1, dtype=np.int64),
            "points": np.zeros((total, 3)), "bpt": np.zeros((total, 3)), "B": B, "ring": ring}
    d = {}
    try:
        for k, a in host.items():
            d[k] = ctypes.c_void_p()
            assert lib.ndsm_hip_device_alloc(a.nbytes, ctypes.byref(d[k])) == 0
        for k in ("B", "ring"):
            assert lib.ndsm_hip_memcpy_h2d(d[k], host[k].ctypes.data, host[k].nbytes) == 0
        counts = np.zeros(2, dtype=np.int64)
        rc = lib.ndsm_hip_vecpot_nulls_device(V.h, d["B"], n, counts.ctypes.data,
                                              *[d[k] for k in ("cell", "pos", "jac", "det", "resid", "sign", "iters")])
        assert rc == 0 and counts[1] == n, (rc, counts, hip.last_error(lib))
        tot = np.zeros(1, dtype=np.int64)
        rc = lib.ndsm_hip_vecpot_skeleton_device(
            V.h, d["B"], n, d["pos"], d["jac"], nring, d["ring"], RADIUS, 0.5, STEP, MAX_STEPS, 1, total,
            *[d[k] for k in NAMES[:10]], tot.ctypes.data, d["points"], d["bpt"])
        assert rc == 0 and tot[0] == total, (rc, tot, hip.last_error(lib))
        for k in ("pos", "jac") + NAMES:
            assert lib.ndsm_hip_memcpy_d2h(host[k].ctypes.data, d[k], host[k].nbytes) == 0
    finally:
        for p in d.values():
            lib.ndsm_hip_device_free(p)
        V.close()
    assert host["pos"].tobytes() == rec[2].tobytes() and host["jac"].tobytes() == rec[3].tobytes()
    same_skel(Skel(*[host[k] for k in NAMES]), want, "chain " + mname)


@pytest.mark.parametrize("mname", list(MESHES))
def test_small_call_on_the_scratch_of_a_larger_one(hip, runner, mname):
    """130 nulls with 31 ring seeds (4290 lanes: every lane of the 1024-wide scan sums a run of several counts), then one
    null with no ring on the scratch that call left"""
    mesh, b, pos, jac = noise_case(mname, [7, 5, 9])
    P, J = first_nulls(pos, jac, 130)
    ring = default_ring(31)
    want = skeleton_numpy(mesh, b, P, J, ring, RADIUS, 0.5, STEP, 12, 2)
    assert len(set(np.diff(want.offsets).tolist())) >= 3
    same_skel(runner(mesh, b, P, J, ring, RADIUS, 0.5, STEP, 12, 2), want, "130 nulls")
    k = int(np.nonzero(want.kind != 0)[0][0])
    one = skeleton_numpy(mesh, b, P[[k]], J[[k]], default_ring(0), RADIUS, 0.5, STEP, 12, 1)
    same_skel(runner(mesh, b, P[[k]], J[[k]], default_ring(0), RADIUS, 0.5, STEP, 12, 1), one, "one null after")


# ---------------------------------------------------------------------------------------------------------------
# 4. closed forms (skeleton_model.py, as test_skeleton_model.py runs them on the restatement)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", list(MESHES))
@pytest.mark.parametrize("name", list(LINEAR))
def test_linear_nulls(runner, mname, name):
    mesh = MESHES[mname]([13, 11, 12])
    got = check_linear(runner, mesh, name)
    same_skel(got, check_linear(skeleton_numpy, mesh, name), "linear " + name)


@pytest.mark.parametrize("mname,shape", [("uniform", [24, 30, 20]), ("aniso", [33, 22, 27]), ("uniform", [12, 14, 11]),
                                         ("aniso", [12, 14, 11])], ids=lambda v: v if isinstance(v, str) else IDS(v))
def test_separator(hip, runner, mname, shape):
    """each null of the separator field is connected to the other by exactly the four ring seeds that face it; the
    Python layer reports the same connections"""
    import ndsm_amd
    mesh = MESHES[mname](shape)
    b, _rc, _aa = separator_field(mesh)
    for radius in (1.0, 0.5):
        sk, pos, jac, conn = check_separator(runner, mesh, radius)
    V = runner.handle(mesh)
    for device in (False, True):
        S = V.skeleton(b, nulls=(pos, jac), radius=0.5, nring=8, capture=0.5, max_steps=4000, device=device)
        got = ndsm_amd.connections(S)
        assert [(m, o, idx.tolist()) for m, o, idx in got] == [(m, o, idx.tolist()) for m, o, idx in conn]
        assert S.paths.points.tobytes() == sk.points.tobytes() and S.hit.reshape(-1).tobytes() == sk.hit.tobytes()


@pytest.mark.parametrize("mname", list(MESHES))
def test_nulls_without_a_type(runner, mname):
    mesh = MESHES[mname]([13, 11, 12])
    same_skel(check_no_type(runner, mesh), check_no_type(skeleton_numpy, mesh), "no type")


@pytest.mark.parametrize("mname", list(MESHES))
def test_every_line_is_a_path(hip, runner, mname):
    """the header's property on the device result: capture off, every line is the paths entry's line of its seed and
    direction (path_numpy, which ndsm_hip_vecpot_paths matches bit for bit); a captured line is its prefix of at least
    one step, also where the capture radius reaches seeds of other nulls (capture 2)"""
    mesh, b, pos, jac = noise_case(mname, [7, 5, 9])
    ring = default_ring(5)
    for capture in (0.0, 0.5, 2.0):
        sk = runner(mesh, b, pos, jac, ring, RADIUS, capture, STEP, MAX_STEPS, 3)
        check_equals_paths(sk, mesh, b, pos, jac, ring, RADIUS, STEP, MAX_STEPS, 3)
        assert (capture == 0.0) == (not np.any(sk.status == CAPTURED))


# ---------------------------------------------------------------------------------------------------------------
# 5. the Python layer
# ---------------------------------------------------------------------------------------------------------------
def as_skel(S):
    """the skeleton_model.Skel of an ndsm_amd.Skeleton (lane order; an absent b as zeros)"""
    fl = S.paths.lines
    return Skel(S.kind, S.eig, S.spine, S.normal, fl.ends.reshape(-1, 3), fl.length.reshape(-1), fl.status.reshape(-1),
                fl.nsteps.reshape(-1), S.hit.reshape(-1), S.paths.offsets, S.paths.points,
                S.paths.b if S.paths.b is not None else np.zeros((len(S.paths.points), 3)))


@pytest.mark.parametrize("mname", list(MESHES))
def test_python_skeleton(hip, mname):
    import ndsm_amd
    mesh, b, _pos, _jac = noise_case(mname, [5, 5, 5])
    want = model_run(mesh, b, nring=6, max_steps=MAX_STEPS, every=2)
    assert len(want.position) >= 2
    total = int(want.paths.offsets[-1])
    V = ndsm_amd.VecPot(*mesh)
    try:
        # nulls=None: the nulls entry runs first (merged); None: a counting call and one of the exact size; a capacity
        # that is too small: repeated once; a large one
        for device in (False, True):
            for cap in (None, 0, 5, total, total + 100):
                S = V.skeleton(b, nring=6, max_steps=MAX_STEPS, every=2, max_points=cap, device=device)
                assert S.position.tobytes() == want.position.tobytes()
                same_skel(as_skel(S), as_skel(want), "python, max_points %s device %s" % (cap, device))
        nul = V.nulls(b)
        S = V.skeleton(b, nulls=nul, nring=6, max_steps=MAX_STEPS, every=2, values=False)
        assert S.paths.b is None and S.paths.points.tobytes() == want.paths.points.tobytes()
        ring = np.array([[1.0, 0.0], [0.0, -2.0]])
        S = V.skeleton(b, nulls=(nul.position, nul.jacobian), ring=ring, capture=0, max_steps=MAX_STEPS)
        same_skel(as_skel(S), as_skel(model_run(mesh, b, nulls=nul, ring=ring, capture=0, max_steps=MAX_STEPS)), "ring")
        assert ndsm_amd.connections(S) == []
    finally:
        V.close()
    S = ndsm_amd.find_skeleton(*mesh, b, nring=6, max_steps=MAX_STEPS, every=2)
    same_skel(as_skel(S), as_skel(want), "find_skeleton")
    assert len(ndsm_amd.spine_of(S, 0)) == 2 and len(ndsm_amd.fan_of(S, 1)) == 6


# ---------------------------------------------------------------------------------------------------------------
# 6. the C entries reject bad input, and write nothing
# ---------------------------------------------------------------------------------------------------------------
def reject_slots(b, pos, jac, ring, cap):
    n, nl, m, f = len(pos), len(pos) * (2 + len(ring)), max(cap, 1), float(FILL)
    return [slot("B", b.reshape(-1), field=True), slot("pos", pos), slot("jac", jac), slot("ring", ring),
            slot("kind", np.full(n, FILL, dtype=np.int32), output=True), slot("eig", np.full((n, 3), f), output=True),
            slot("spine", np.full((n, 3), f), output=True), slot("normal", np.full((n, 3), f), output=True),
            slot("ends", np.full((nl, 3), f), output=True), slot("length", np.full(nl, f), output=True),
            slot("status", np.full(nl, FILL, dtype=np.int32), output=True),
            slot("nsteps", np.full(nl, FILL, dtype=np.int32), output=True),
            slot("hit", np.full(nl, FILL, dtype=np.int32), output=True),
            slot("offsets", np.full(nl + 1, FILL, dtype=np.int64), output=True),
            slot("points", np.full((m, 3), f), output=True), slot("bpt", np.full((m, 3), f), output=True)]


def reject(hip, V, b, pos, jac, ring, code, device, missing=None, nnulls=None, nring=None, radius=RADIUS, capture=0.5,
           step=STEP, max_steps=MAX_STEPS, every=1, cap=50):
    """the entry returns `code` and clears total; the device entry changes no byte of the allocation, the host entry
    clears its outputs and leaves its inputs alone"""
    total = np.full(1, FILL, dtype=np.int64)
    slots = reject_slots(b, pos, jac, ring, cap + 2 if (not device and cap > 0) else cap)
    names = [s.name for s in slots]
    nn = len(pos) if nnulls is None else nnulls
    nr = len(ring) if nring is None else nring

    def call(*p):
        p = [None if names[i] == missing else q for i, q in enumerate(p)]
        entry = V.L.ndsm_hip_vecpot_skeleton_device if device else V.L.ndsm_hip_vecpot_skeleton
        return entry(V.h, p[0], nn, p[1], p[2], nr, p[3], radius, capture, step, max_steps, every, cap, *p[4:14],
                     None if missing == "total" else total.ctypes.data, p[14], p[15])
    if device:
        A = Arena(LibTransport(V.L), slots)
        A.run(call, written={s.name: 0 for s in slots if s.output})
        rc = A.rc
    else:
        arr = [s.array.copy() for s in slots]
        rc = call(*[a.ctypes.data for a in arr])
        for s, a in zip(slots, arr):
            if not s.output:
                assert a.tobytes() == s.array.tobytes(), s.name
            elif s.name in ("points", "bpt"):
                k = max(cap, 0)
                assert s.name == missing or (not np.any(a[:k]) and np.all(a[k:] == FILL)), s.name
            elif nn == len(pos) and nr == len(ring):
                assert s.name == missing or not np.any(a), s.name
    assert rc == code, (rc, hip.last_error(V.L))
    assert total[0] == (FILL if missing == "total" else 0)


def test_c_entries_reject_bad_input(hip):
    import ndsm_amd
    mesh, b, pos, jac = noise_case("aniso", [5, 5, 5])
    pos, jac = first_nulls(pos, jac, 3)
    ring = default_ring(4)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for device in (True, False):
            for kw in (dict(nnulls=-1), dict(nring=-1), dict(every=0), dict(every=-3), dict(cap=-1), dict(radius=0.0),
                       dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(capture=-0.5),
                       dict(capture=float("nan")), dict(capture=float("inf")), dict(step=0.0), dict(step=float("nan")),
                       dict(max_steps=0)):
                reject(hip, V, b, pos, jac, ring, 9004, device, **kw)
            for missing in ("B", "pos", "jac", "ring", "kind", "eig", "spine", "normal", "ends", "length", "status",
                            "nsteps", "hit", "offsets", "total", "points"):
                reject(hip, V, b, pos, jac, ring, 9002, device, missing=missing)
        # no nulls: success, total 0, nothing else touched
        total = np.full(1, FILL, dtype=np.int64)
        for entry in (V.L.ndsm_hip_vecpot_skeleton, V.L.ndsm_hip_vecpot_skeleton_device):
            total[0] = FILL
            assert entry(V.h, None, 0, None, None, 4, None, RADIUS, 0.5, STEP, MAX_STEPS, 1, 50, *[None] * 10,
                         total.ctypes.data, None, None) == 0
            assert total[0] == 0
    finally:
        V.close()
