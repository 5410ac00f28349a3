"""GPU tests of the field-line path entries (run with -m gpu on an MI355X): ndsm_hip_vecpot_paths and
ndsm_hip_vecpot_paths_device against the numpy restatement path_model.path_numpy bit for bit, the closed forms of
path_checks.py, and what ties the paths to the trace entries.  The C entries run on device_arena.Arena allocations:
element-aligned bases, NaN bands round B and G, canaries elsewhere, and every slot past the points written must come back
as it went up - a stray write shows as a failed comparison inside the test's own allocation, never as a fault."""
import numpy as np
import pytest

import path_checks
from device_arena import Arena, LibTransport, slot
from golden_inputs import aniso_mesh, uniform_mesh
from line_model import abc, face_seeds, inner_seeds
from path_model import Paths, join, npts_of, path_numpy, paths_numpy, take

pytestmark = pytest.mark.gpu

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
IDS = lambda s: "x".join(map(str, s))   # noqa: E731
LINE_SHAPES = ([4, 4, 4], [5, 5, 5], [7, 5, 9], [67, 5, 4], [5, 4, 67])
# one lane; exactly one wave; a wave plus one; two waves; a block plus one (test_gpu_caller_arrays.SEED_COUNTS)
SEED_COUNTS = (1, 32, 33, 64, 65)
EVERYS = (1, 2, 3, 7, 1000)
STEP, MAX_STEPS = 0.37, 300
FILL = 7
NAMES = ("ends", "length", "integral", "status", "nsteps", "offsets", "points", "bpt", "gpt", "ipt")
_REF = {}


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def line_case(mname, ns):
    """test_gpu_caller_arrays.line_case's fields and 41 seeds (a FRESH default_rng(5): 29 inside, 2 on each face), and
    the restatement's paths per (sgn, with G, every), computed once per mesh and shape: every line depends on its own
    seed only, so any seed list made of these has its lines among them"""
    key = (mname, IDS(ns))
    if key not in _REF:
        mesh = MESHES[mname](ns)
        b, g = abc(mesh), abc(mesh, k=0.7 * np.pi, phase=0.3)
        rng = np.random.default_rng(5)
        seeds = np.concatenate([inner_seeds(mesh, rng, 29), face_seeds(mesh, rng, 2)])
        ref = {(sgn, withg, every): path_numpy(mesh, b, g if withg else None, seeds, STEP, MAX_STEPS, sgn, every)
               for sgn in (1.0, -1.0) for withg in (True, False) for every in EVERYS}
        assert len(seeds) == 41
        _REF[key] = (mesh, b, g, seeds, ref)
    return _REF[key]


def expected(ref, idx, direction, withg, every):
    sgns = (1.0, -1.0) if direction == 0 else (float(direction),)
    return join([take(ref[(sgn, withg, every)], idx) for sgn in sgns])


def same_paths(got, want, what, upto=None):
    """bit for bit; upto: the point arrays of `got` hold the first upto slots only"""
    for k, name in enumerate(NAMES):
        w = want[k] if upto is None or k < 6 else want[k][:upto]
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (what, name, got[k].shape, w.shape)
        assert got[k].tobytes() == w.tobytes(), (what, name)


def paths_call(hip, V, b, g, S, step, max_steps, direction, every, cap, arrays=("bpt", "gpt", "ipt"), device=True,
               plain=False):
    """One call of a C entry with capacity cap on point arrays of exactly max(cap, 1) slots, every array filled with
    FILL first.  device: on an arena (the slots past the points written must come back as they went up, the arena
    checks it); else the host entry on numpy arrays, checked the same way here.  arrays: the optional point arrays that
    are passed (the others NULL); cap = 0 passes all four NULL.  Returns (Paths, total): the point arrays cut to the
    slots written, an array that was not passed - or gpt, ipt without G - as zeros."""
    S = np.ascontiguousarray(S, dtype=np.float64)
    ns = len(S)
    nl = ns * (2 if direction == 0 else 1)
    f = float(FILL)
    total = np.full(1, FILL, dtype=np.int64)
    m = max(cap, 1)
    outs = [("ends", np.full((nl, 3), f)), ("length", np.full(nl, f)), ("integral", np.full(nl, f)),
            ("status", np.full(nl, FILL, dtype=np.int32)), ("nsteps", np.full(nl, FILL, dtype=np.int32)),
            ("offsets", np.full(nl + 1, FILL, dtype=np.int64))]
    pts = [(name, np.full((m, 3) if name != "ipt" else m, f)) for name in ("points",) + tuple(arrays)] if cap > 0 else []
    passed = [name for name, _a in pts]
    entry = V.L.ndsm_hip_vecpot_paths_device if device else V.L.ndsm_hip_vecpot_paths

    def call(dB, dG, dS, *p):
        p = list(p)
        head, by = p[:6], dict(zip(passed, p[6:]))
        return entry(V.h, dB, dG, ns, dS, step, max_steps, direction, every, cap, *head, total.ctypes.data,
                     *[by.get(k) for k in ("points", "bpt", "gpt", "ipt")])

    def nwritten():
        return min(max(int(total[0]), 0), cap)

    def written():
        return {name: (nwritten() if name in ("points", "bpt") or g is not None else 0) for name in passed}

    if device:
        slots = ([slot("B", b.reshape(-1), field=True)] + ([slot("G", g.reshape(-1), field=True)] if g is not None else [])
                 + [slot("seeds", S)] + [slot(name, a, output=True) for name, a in outs + pts])
        A = Arena(LibTransport(V.L), slots, plain=plain)
        if g is not None:
            got = A.run(call, written=written)
        else:
            got = A.run(lambda dB, dS, *p: call(dB, None, dS, *p), written=written)
        rc = A.rc
        got = dict(zip([s.name for s in slots], got))
    else:
        B = np.ascontiguousarray(b, dtype=np.float64).reshape(-1).copy()
        G = None if g is None else np.ascontiguousarray(g, dtype=np.float64).reshape(-1).copy()
        got = {name: a.copy() for name, a in outs + pts}
        rc = call(B.ctypes.data, None if G is None else G.ctypes.data, S.ctypes.data,
                  *[got[name].ctypes.data for name, _a in outs + pts])
        assert B.tobytes() == b.tobytes() and (G is None or G.tobytes() == g.tobytes())
        for name, n in written().items():
            if name in passed:
                assert np.all(got[name][n:] == f), "host entry: %s changed past the %d points written" % (name, n)
    assert rc == 0, (rc, hip.last_error(V.L))
    n = nwritten()
    full = {"points": np.zeros((n, 3)), "bpt": np.zeros((n, 3)), "gpt": np.zeros((n, 3)), "ipt": np.zeros(n)}
    for name in passed:
        if name in ("points", "bpt") or g is not None:
            full[name] = got[name][:n]
    assert int(got["offsets"][-1]) == int(total[0])
    return Paths(*[got[name] for name, _a in outs], full["points"], full["bpt"], full["gpt"], full["ipt"]), int(total[0])


class Runner:
    """path_checks' runner on the C entries: a counting call (max_points = 0, the four point arrays NULL), then the
    filling call of that size; one handle per mesh, closed at the end"""

    def __init__(self, hip, device=True):
        self.hip, self.device, self.handles = hip, device, {}

    def handle(self, mesh):
        import ndsm_amd
        key = tuple(np.asarray(q).tobytes() for q in mesh)
        if key not in self.handles:
            self.handles[key] = ndsm_amd.VecPot(*mesh)
        return self.handles[key]

    def __call__(self, mesh, b, g, seeds, step, max_steps, direction, every):
        V = self.handle(mesh)
        counted, total = paths_call(self.hip, V, b, g, seeds, step, max_steps, direction, every, 0, device=self.device)
        assert total == int(npts_of(counted.nsteps, every).sum())
        p, total2 = paths_call(self.hip, V, b, g, seeds, step, max_steps, direction, every, total, device=self.device)
        assert total2 == total
        for k in range(6):
            assert p[k].tobytes() == counted[k].tobytes(), NAMES[k]
        return p

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
@pytest.mark.parametrize("ns", LINE_SHAPES, ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_paths_match_the_restatement_bitwise(hip, mname, ns):
    import ndsm_amd
    mesh, b, g, seeds, ref = line_case(mname, ns)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for count in SEED_COUNTS:
            idx = np.arange(count) % len(seeds)
            S = seeds[idx]
            for direction in (1, -1, 0):
                for withg in (True, False):
                    for every in EVERYS:
                        want = expected(ref, idx, direction, withg, every)
                        total = int(want.offsets[-1])
                        got, n = paths_call(hip, V, b, g if withg else None, S, STEP, MAX_STEPS, direction, every, total)
                        what = "%s %s %d seeds, direction %d, G %s, every %d" % (mname, ns, count, direction, withg, every)
                        assert n == total, what
                        same_paths(got, want, what)
                        if every > 1:
                            path_checks.check_stride(expected(ref, idx, direction, withg, 1), got, every)
        # each optional point array present and NULL, the host entry, and arrays in allocations of their own
        idx = np.arange(33) % len(seeds)
        for direction in (0, -1):
            for withg in (True, False):
                want = expected(ref, idx, direction, withg, 2)
                total = int(want.offsets[-1])
                for arrays in ((), ("bpt",), ("gpt",), ("ipt",), ("gpt", "ipt"), ("bpt", "gpt", "ipt")):
                    zeroed = want._replace(**{k: np.zeros_like(getattr(want, k)) for k in ("bpt", "gpt", "ipt")
                                              if k not in arrays})
                    for device in (True, False):
                        got, _n = paths_call(hip, V, b, g if withg else None, seeds[idx], STEP, MAX_STEPS, direction, 2,
                                             total, arrays=arrays, device=device)
                        same_paths(got, zeroed, "%s %s arrays %s device %s G %s" % (mname, ns, arrays, device, withg))
                got, _n = paths_call(hip, V, b, g if withg else None, seeds[idx], STEP, MAX_STEPS, direction, 2, total,
                                     plain=True)
                same_paths(got, want, "%s %s plain" % (mname, ns))
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. capacity
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", ([5, 5, 5], [7, 5, 9]), ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_capacity(hip, mname, ns):
    """offsets and total do not depend on max_points; the slots below it are those of the full result, everything at
    and beyond it is untouched (paths_call's arena and host checks)"""
    import ndsm_amd
    mesh, b, g, seeds, ref = line_case(mname, ns)
    idx = np.arange(33) % len(seeds)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for direction, every in ((0, 2), (1, 1)):
            want = expected(ref, idx, direction, True, every)
            total = int(want.offsets[-1])
            for device in (True, False):
                for cap in (0, 1, total - 1, total, total + 3):
                    got, n = paths_call(hip, V, b, g, seeds[idx], STEP, MAX_STEPS, direction, every, cap, device=device)
                    assert n == total
                    same_paths(got, want, "%s %s capacity %d device %s" % (mname, ns, cap, device), upto=min(cap, total))
                    assert len(got.points) == min(cap, total)
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. consistency with the trace entries
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", list(MESHES))
def test_consistent_with_trace(hip, runner, mname):
    ns = [7, 5, 9]
    mesh, b, g, seeds, _ref = line_case(mname, ns)
    V = runner.handle(mesh)
    for every in (1, 3):
        p = runner(mesh, b, g, seeds, STEP, MAX_STEPS, 0, every)
        path_checks.check_structure(p, seeds, 0, every)
        fl = V.trace(b, seeds, g=g, step=STEP, max_steps=MAX_STEPS, direction="both", device=True)
        for k, a in enumerate((fl.ends, fl.length, fl.integral, fl.status, fl.nsteps)):
            assert p[k].tobytes() == a.tobytes(), NAMES[k]
    # point j of a line is where the trace entry ends after j steps
    p = runner(mesh, b, g, seeds, STEP, MAX_STEPS, 0, 1)
    lines = np.argsort(p.nsteps[:len(seeds)])[-4:]               # forward lines of the most steps
    assert p.nsteps[lines].min() >= 4
    for l in lines:
        n = int(p.nsteps[l])
        for j in (1, 2, n - 1):
            fl = V.trace(b, seeds[[l]], g=g, step=STEP, max_steps=j, direction="both", device=True)
            for row, lane in ((0, l), (1, len(seeds) + l)):
                if j < p.nsteps[lane]:
                    k = int(p.offsets[lane]) + j
                    assert p.points[k].tobytes() == fl.ends[row, 0].tobytes(), (l, j, row)
                    assert p.ipt[k].tobytes() == fl.integral[row, 0].tobytes(), (l, j, row)


# ---------------------------------------------------------------------------------------------------------------
# 4. many lanes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", list(MESHES))
def test_many_lanes_then_one(hip, runner, mname):
    """4200 lanes: every lane of the 1024-wide scan sums a run of several counts; then one seed on whatever scratch
    the large call left"""
    mesh = MESHES[mname]([5, 5, 5])
    b, g = abc(mesh), abc(mesh, k=0.7 * np.pi, phase=0.3)
    rng = np.random.default_rng(7)
    seeds = np.concatenate([inner_seeds(mesh, rng, 2088), face_seeds(mesh, rng, 2)])
    assert len(seeds) == 2100
    for every in (1, 3):
        want = paths_numpy(mesh, b, g, seeds, STEP, 8, 0, every)
        assert len(set(np.diff(want.offsets).tolist())) >= 3
        same_paths(runner(mesh, b, g, seeds, STEP, 8, 0, every), want, "%s 2100 seeds, every %d" % (mname, every))
    one = seeds[[1234]]
    same_paths(runner(mesh, b, g, one, STEP, 8, 0, 1), paths_numpy(mesh, b, g, one, STEP, 8, 0, 1), "one seed after")


# ---------------------------------------------------------------------------------------------------------------
# 5. other ends, closed forms (path_checks.py, as test_paths_model.py runs them on the restatement)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", list(MESHES))
def test_other_ends(runner, mname):
    path_checks.check_other_ends(runner, MESHES[mname]([12, 11, 10]))


@pytest.mark.parametrize("mname", list(MESHES))
def test_other_ends_match_the_restatement(runner, mname):
    """the same calls through a runner that also compares every result with the restatement bit for bit"""
    def both(mesh, b, g, seeds, step, max_steps, direction, every):
        got = runner(mesh, b, g, seeds, step, max_steps, direction, every)
        same_paths(got, paths_numpy(mesh, b, g, seeds, step, max_steps, direction, every), "other ends")
        return got
    path_checks.check_other_ends(both, MESHES[mname]([12, 11, 10]))


@pytest.mark.parametrize("mname", list(MESHES))
def test_uniform_field(runner, mname):
    path_checks.check_uniform(runner, MESHES[mname]([9, 8, 10]))


@pytest.mark.parametrize("mname", list(MESHES))
def test_helical_field(runner, mname):
    """the device equals the restatement bit for bit, so its errors are the restatement's (DESIGN.md has them)"""
    mesh = MESHES[mname]([12, 14, 11])
    got = path_checks.check_helical(runner, mesh)
    model = path_checks.check_helical(paths_numpy, mesh)
    assert got == model


# ---------------------------------------------------------------------------------------------------------------
# 6. independence
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", list(MESHES))
def test_a_path_depends_on_its_own_seed_only(hip, mname):
    import ndsm_amd
    mesh, b, g, seeds, _ref = line_case(mname, [7, 5, 9])
    V = ndsm_amd.VecPot(*mesh)
    try:
        def one(S, i, direction, device):
            """line i (forward) of the call, as a Paths of one line"""
            p, _n = paths_call(hip, V, b, g, S, STEP, MAX_STEPS, direction, 2, 10 ** 4, device=device)
            return take(p, [i])
        alone = one(seeds[[5]], 0, 1, True)
        order = np.random.default_rng(3).permutation(len(seeds))
        for what, got in (("in a batch", one(seeds, 5, 1, True)),
                          ("in another order", one(seeds[order], int(np.nonzero(order == 5)[0][0]), 1, True)),
                          ("with both directions", one(seeds, 5, 0, True)),
                          ("host entry", one(seeds, 5, 1, False)),
                          ("host entry, alone", one(seeds[[5]], 0, 0, False))):
            same_paths(got, alone, what)
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. the Python layer
# ---------------------------------------------------------------------------------------------------------------
def as_paths(fp, with_g):
    """the path_model.Paths of an ndsm_amd.FieldPaths (lane order; absent arrays as zeros)"""
    n = len(fp.points)
    fl = fp.lines
    return Paths(fl.ends.reshape(-1, 3), fl.length.reshape(-1), fl.integral.reshape(-1), fl.status.reshape(-1),
                 fl.nsteps.reshape(-1), fp.offsets, fp.points, fp.b if fp.b is not None else np.zeros((n, 3)),
                 fp.g if with_g and fp.g is not None else np.zeros((n, 3)),
                 fp.integral if with_g and fp.integral is not None else np.zeros(n))


@pytest.mark.parametrize("mname", list(MESHES))
def test_python_paths(hip, mname):
    import ndsm_amd
    mesh, b, g, seeds, ref = line_case(mname, [5, 5, 5])
    idx = np.arange(len(seeds))
    want = expected(ref, idx, 0, True, 2)
    total = int(want.offsets[-1])
    V = ndsm_amd.VecPot(*mesh)
    try:
        # None: a counting call and one of the exact size; a capacity that is too small: repeated once; a large one
        for device in (False, True):
            for cap in (None, 0, 5, total, total + 100):
                fp = V.paths(b, seeds, g=g, step=STEP, max_steps=MAX_STEPS, every=2, max_points=cap, device=device)
                same_paths(as_paths(fp, True), want, "python, max_points %s device %s" % (cap, device))
                assert np.array_equal(fp.lines.flh, fp.lines.integral[0] + fp.lines.integral[1])
        fp = V.paths(b, seeds, step=STEP, max_steps=MAX_STEPS, direction="backward", every=7)
        assert fp.g is None and fp.integral is None and fp.lines.flh is None
        same_paths(as_paths(fp, False), expected(ref, idx, -1, False, 7), "python, no g")
        fp = V.paths(b, seeds, g=g, step=STEP, max_steps=MAX_STEPS, direction="forward", values=False)
        assert fp.b is None and fp.g is None and fp.integral is None
        assert fp.points.tobytes() == expected(ref, idx, 1, True, 1).points.tobytes()
    finally:
        V.close()
    fp = ndsm_amd.trace_paths(*mesh, b, seeds, g=g, step=STEP, max_steps=MAX_STEPS, every=2)
    same_paths(as_paths(fp, True), want, "trace_paths")


@pytest.mark.parametrize("mname", list(MESHES))
def test_whole_line(hip, mname):
    import ndsm_amd

    def run(mesh, b, g, seeds, step, max_steps, direction, every):
        assert direction == 0
        fp = ndsm_amd.trace_paths(*mesh, b, seeds, g=g, step=step, max_steps=max_steps, every=every)
        return as_paths(fp, True)
    path_checks.check_whole_line(run, MESHES[mname]([9, 8, 10]))


# ---------------------------------------------------------------------------------------------------------------
# 8. the C entries reject bad input, and write nothing
# ---------------------------------------------------------------------------------------------------------------
def test_c_entries_reject_bad_input(hip):
    import ndsm_amd
    mesh, b, g, seeds, _ref = line_case("aniso", [5, 5, 5])
    V = ndsm_amd.VecPot(*mesh)
    try:
        for every, cap in ((0, 50), (-3, 50), (1, -1)):
            reject_device(hip, V, b, g, seeds, every, cap, 9004)
            reject_host(hip, V, b, g, seeds, every, cap, 9004)
        for missing in ("offsets", "total", "points"):
            reject_device(hip, V, b, g, seeds, 1, 50, 9002, missing=missing)
            reject_host(hip, V, b, g, seeds, 1, 50, 9002, missing=missing)
        # no seeds: success, total 0, nothing else touched
        total = np.full(1, FILL, dtype=np.int64)
        for entry in (V.L.ndsm_hip_vecpot_paths, V.L.ndsm_hip_vecpot_paths_device):
            total[0] = FILL
            assert entry(V.h, None, None, 0, None, STEP, MAX_STEPS, 0, 1, 50, *[None] * 6, total.ctypes.data,
                         *[None] * 4) == 0
            assert total[0] == 0
    finally:
        V.close()


def reject_slots(b, g, seeds, cap):
    nl, m, f = 2 * len(seeds), max(cap, 1), float(FILL)
    return [slot("B", b.reshape(-1), field=True), slot("G", g.reshape(-1), field=True), slot("seeds", seeds),
            slot("ends", np.full((nl, 3), f), output=True), slot("length", np.full(nl, f), output=True),
            slot("integral", np.full(nl, f), output=True), slot("status", np.full(nl, FILL, dtype=np.int32), output=True),
            slot("nsteps", np.full(nl, FILL, dtype=np.int32), output=True),
            slot("offsets", np.full(nl + 1, FILL, dtype=np.int64), output=True),
            slot("points", np.full((m, 3), f), output=True), slot("bpt", np.full((m, 3), f), output=True),
            slot("gpt", np.full((m, 3), f), output=True), slot("ipt", np.full(m, f), output=True)]


def reject_device(hip, V, b, g, seeds, every, cap, code, missing=None):
    """the device entry returns `code`, clears total and changes no byte of the allocation"""
    total = np.full(1, FILL, dtype=np.int64)
    slots = reject_slots(b, g, seeds, cap)

    def call(dB, dG, dS, *p):
        p = list(p)
        if missing == "offsets":
            p[5] = None
        if missing == "points":
            p[6] = None
        return V.L.ndsm_hip_vecpot_paths_device(V.h, dB, dG, len(seeds), dS, STEP, MAX_STEPS, 0, every, cap, *p[:6],
                                                None if missing == "total" else total.ctypes.data, *p[6:])
    A = Arena(LibTransport(V.L), slots)
    A.run(call, written={s.name: 0 for s in slots if s.output})
    assert A.rc == code, (A.rc, hip.last_error(V.L))
    assert total[0] == (FILL if missing == "total" else 0)


def reject_host(hip, V, b, g, seeds, every, cap, code, missing=None):
    """the host entry returns `code`, clears total, the lines' outputs, offsets and max_points slots of the point arrays,
    and leaves its inputs alone"""
    total = np.full(1, FILL, dtype=np.int64)
    arr = [s.array.copy() for s in reject_slots(b, g, seeds, cap + 2 if cap > 0 else 2)]
    p = [a.ctypes.data for a in arr]
    if missing == "offsets":
        p[8] = None
    if missing == "points":
        p[9] = None
    rc = V.L.ndsm_hip_vecpot_paths(V.h, p[0], p[1], len(seeds), p[2], STEP, MAX_STEPS, 0, every, cap, *p[3:9],
                                   None if missing == "total" else total.ctypes.data, *p[9:])
    assert rc == code, (rc, hip.last_error(V.L))
    assert total[0] == (FILL if missing == "total" else 0)
    assert arr[0].tobytes() == b.tobytes() and arr[1].tobytes() == g.tobytes() and arr[2].tobytes() == seeds.tobytes()
    for k in range(3, 9):
        if not (missing == "offsets" and k == 8):
            assert not np.any(arr[k]), k
    n = max(cap, 0)
    for k in range(9, 13):
        if missing == "points" and k == 9:
            continue
        assert not np.any(arr[k][:n]) and np.all(arr[k][n:] == FILL), k
