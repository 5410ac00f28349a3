"""GPU tests of the separator entries (run with -m gpu on an MI355X): ndsm_hip_vecpot_separators and
ndsm_hip_vecpot_separators_device against the numpy restatement separator_model.separators_numpy bit for bit, the
closed forms of separator_model.py through the device entries, the property that ties a bracket's line to the skeleton
entry, and the chain from the skeleton entries.  The C entries run on device_arena.Arena allocations: element-aligned
bases, NaN bands round B, canaries elsewhere, and every slot past the points written must come back as it went up - a
stray write shows as a failed comparison inside the test's own allocation, never as a fault."""
import ctypes

import numpy as np
import pytest

from device_arena import Arena, LibTransport, slot
from golden_inputs import aniso_mesh, uniform_mesh
from separator_model import (CROSS_OPT, FOUND, NAMES, NPER, UNRESOLVED, Sep, check_crossing, check_property,
                             check_structure, crossing_case, opposite_pairs, ring_brackets, ring_of, same_sep,
                             separators_numpy)
from skeleton_model import Skel, default_ring, noise_nulls, skeleton_numpy, type_numpy
from skeleton_model import NAMES as SKEL_NAMES

pytestmark = pytest.mark.gpu

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v)   # noqa: E731
NOISE_OPT = dict(radius=0.5, capture=0.5, step=0.5, max_steps=50, rounds=10, tol=1e-12, every=1)
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


@pytest.fixture()
def handles():
    import ndsm_amd
    made = {}

    def handle(mesh):
        key = tuple(np.asarray(q).tobytes() for q in mesh)
        if key not in made:
            made[key] = ndsm_amd.VecPot(*mesh)
        return made[key]
    yield handle
    for V in made.values():
        V.close()


def noise_case(mname, ns, narcs):
    """white noise on the mesh, its nulls typed as the skeleton types them, the brackets of all opposite-sign pairs (the
    first narcs arcs of a 4-seed ring each) and the restatement's result with NOISE_OPT, once per case"""
    key = (mname, IDS(ns), narcs)
    if key not in _CASE:
        mesh = MESHES[mname](ns)
        b, pos, jac = noise_nulls(mesh)
        _ok, _s, kind, _eig, _v, normal, _e1, _e2 = type_numpy(jac)
        pair, arc = ring_brackets(ring_of(4), opposite_pairs(kind), narcs)
        want = separators_numpy(mesh, b, pos, kind, normal, pair, arc, **NOISE_OPT)
        _CASE[key] = (mesh, b, pos, jac, kind.astype(np.int32), normal, pair, arc, want)
    return _CASE[key]


def out_slots(nbr, cap, with_bpt=True):
    f, m = float(FILL), max(cap, 1)
    i32 = np.int32
    outs = [("state", np.full(nbr, FILL, dtype=i32)), ("nrounds", np.full(nbr, FILL, dtype=i32)),
            ("coef", np.full((nbr, 4), f)), ("width", np.full(nbr, f)), ("side", np.full(nbr, FILL, dtype=i32)),
            ("dmin", np.full((nbr, 2), f)), ("ends", np.full((nbr, 3), f)), ("length", np.full(nbr, f)),
            ("status", np.full(nbr, FILL, dtype=i32)), ("nsteps", np.full(nbr, FILL, dtype=i32)),
            ("offsets", np.full(nbr + 1, FILL, dtype=np.int64))]
    pts = ([("points", np.full((m, 3), f))] + ([("bpt", np.full((m, 3), f))] if with_bpt else [])) if cap > 0 else []
    return outs, pts


def sep_call(hip, V, b, pos, kind, normal, pair, arc, opt, cap, with_bpt=True, device=True, plain=False):
    """One call of a C entry with capacity cap on point arrays of exactly max(cap, 1) slots, every output filled with
    FILL first.  device: on an arena (the slots past the points written must come back as they went up, the arena
    checks it); else the host entry on numpy arrays, checked the same way here.  cap = 0 passes both point arrays NULL.
    Returns (Sep, total): the point arrays cut to the slots written, bpt as zeros when it was not passed."""
    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    kind = np.ascontiguousarray(kind, dtype=np.int32).reshape(-1)
    normal = np.ascontiguousarray(normal, dtype=np.float64).reshape(-1, 3)
    pair = np.ascontiguousarray(pair, dtype=np.int32).reshape(-1, 2)
    arc = np.ascontiguousarray(arc, dtype=np.float64).reshape(-1, 4)
    n, nbr = len(pos), len(pair)
    total = np.full(1, FILL, dtype=np.int64)
    outs, pts = out_slots(nbr, cap, with_bpt)
    passed = [name for name, _a in pts]
    entry = V.L.ndsm_hip_vecpot_separators_device if device else V.L.ndsm_hip_vecpot_separators
    head = (opt["radius"], opt["capture"], opt["step"], opt["max_steps"], opt["rounds"], opt["tol"], opt["every"], cap)

    def call(dB, dpos, dkind, dnormal, dpair, darc, *p):
        p = list(p)
        by = dict(zip(passed, p[11:]))
        return entry(V.h, dB, n, dpos, dkind, dnormal, nbr, dpair, darc, *head, *p[:11], total.ctypes.data,
                     by.get("points"), by.get("bpt"))

    def nwritten():
        return min(max(int(total[0]), 0), cap)

    ins = [("B", np.ascontiguousarray(b, dtype=np.float64).reshape(-1)), ("pos", pos), ("kind", kind),
           ("normal", normal), ("pair", pair), ("arc", arc)]
    if device:
        slots = ([slot("B", ins[0][1], field=True)] + [slot(name, a) for name, a in ins[1:]] +
                 [slot(name, a, output=True) for name, a in outs + pts])
        A = Arena(LibTransport(V.L), slots, plain=plain)
        got = A.run(call, written=lambda: {name: nwritten() for name in passed})
        rc = A.rc
        got = dict(zip([s.name for s in slots], got))
    else:
        held = [a.copy() for _name, a in ins]
        got = {name: a.copy() for name, a in outs + pts}
        rc = call(*[a.ctypes.data for a in held], *[got[name].ctypes.data for name, _a in outs + pts])
        for a, (name, orig) in zip(held, ins):
            assert a.tobytes() == orig.tobytes(), name
        for name in passed:
            assert np.all(got[name][nwritten():] == float(FILL)), "host entry: %s changed past the points written" % name
    assert rc == 0, (rc, hip.last_error(V.L))
    k = nwritten()
    full = {"points": np.zeros((k, 3)), "bpt": np.zeros((k, 3))}
    for name in passed:
        full[name] = got[name][:k]
    assert int(got["offsets"][-1]) == int(total[0])
    return Sep(*[got[name] for name, _a in outs], full["points"], full["bpt"]), int(total[0])


class Runner:
    """separator_model's runner on the C entries: a counting call (max_points = 0, both point arrays NULL), then the
    filling call of that size"""

    def __init__(self, hip, handle, device=True):
        self.hip, self.handle, self.device = hip, handle, device

    def __call__(self, mesh, b, pos, kind, normal, pair, arc, **opt):
        V = self.handle(mesh)
        counted, total = sep_call(self.hip, V, b, pos, kind, normal, pair, arc, opt, 0, device=self.device)
        sp, total2 = sep_call(self.hip, V, b, pos, kind, normal, pair, arc, opt, total, device=self.device)
        assert total2 == total == int(sp.offsets[-1])
        for k in range(NPER + 1):
            assert sp[k].tobytes() == counted[k].tobytes(), NAMES[k]
        return sp


def device_skeleton(hip, handle):
    """skeleton_model's runner on ndsm_hip_vecpot_skeleton_device (plain allocations)"""
    def run(mesh, b, pos, jac, ring, radius, capture, step, max_steps, every):
        V = handle(mesh)
        S = V.skeleton(b, nulls=(pos, jac), radius=radius, ring=ring, capture=capture, step=step, max_steps=max_steps,
                       every=every, device=True)
        fl = S.paths.lines
        return Skel(S.kind, S.eig, S.spine, S.normal, fl.ends.reshape(-1, 3), fl.length.reshape(-1),
                    fl.status.reshape(-1), fl.nsteps.reshape(-1), S.hit.reshape(-1), S.paths.offsets, S.paths.points,
                    S.paths.b)
    return run


# ---------------------------------------------------------------------------------------------------------------
# 1. the crossing field: the restatement bit for bit, the closed forms, the property through the device skeleton entry
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,shape", [("uniform", [12, 14, 11]), ("aniso", [33, 22, 27])], ids=IDS)
def test_crossing_field(hip, handles, mname, shape):
    mesh = MESHES[mname](shape)
    b, _rc, pos, kind, normal, jac = crossing_case(mesh)
    for rot in (0.0, 0.3):
        got, pair, arc = check_crossing(Runner(hip, handles), mesh, rot)
        want = separators_numpy(mesh, b, pos, kind, normal, pair, arc, **CROSS_OPT)
        same_sep(got, want, "crossing %s %s rot %g" % (mname, shape, rot))
    assert check_property(got, device_skeleton(hip, handles), mesh, b, pos, jac, pair, CROSS_OPT["radius"],
                          CROSS_OPT["capture"], CROSS_OPT["step"], CROSS_OPT["max_steps"], 1) == 4
    host, _n = sep_call(hip, handles(mesh), b, pos, kind, normal, pair, arc, CROSS_OPT, int(want.offsets[-1]),
                        device=False)
    same_sep(host, want, "crossing, host entry")


# ---------------------------------------------------------------------------------------------------------------
# 2. the nulls of white noise, all opposite-sign pairs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,narcs", [([5, 5, 5], 4), ([7, 5, 9], 1)], ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_noise_nulls_match_the_restatement_bitwise(hip, handles, mname, ns, narcs):
    mesh, b, pos, jac, kind, normal, pair, arc, want = noise_case(mname, ns, narcs)
    assert len(set(want.state.tolist())) >= 4, np.bincount(want.state, minlength=6)
    V = handles(mesh)
    total = int(want.offsets[-1])
    nob = want._replace(bpt=np.zeros_like(want.bpt))
    for device in (True, False):
        for with_bpt in (True, False):
            got, n = sep_call(hip, V, b, pos, kind, normal, pair, arc, NOISE_OPT, total, with_bpt=with_bpt,
                              device=device)
            assert n == total
            same_sep(got, want if with_bpt else nob, "%s %s device %s bpt %s" % (mname, ns, device, with_bpt))
    check_structure(got, pos, pair, 1)
    got, _n = sep_call(hip, V, b, pos, kind, normal, pair, arc, NOISE_OPT, total, plain=True)
    same_sep(got, want, "%s %s plain" % (mname, ns))
    if narcs == 4:
        assert check_property(got, device_skeleton(hip, handles), mesh, b, pos, jac, pair, 0.5, 0.5, 0.5, 50, 1,
                              limit=3) >= 6


@pytest.mark.parametrize("mname", list(MESHES))
def test_bracket_counts_rounds_tol_every(hip, handles, mname):
    """1, 2, 64 and 65 brackets (one lane of the line kernel; one workgroup of it; a workgroup plus one), rounds 1 and
    10, tol 0 and 1e-12, every 1, 3 and 1000; 1, 2 and 65 brackets through the host entry as well; 3 nulls"""
    mesh, b, pos, _jac, kind, normal, pair, arc, want = noise_case(mname, [5, 5, 5], 4)
    # brackets that carry a line first, so that the small calls trace something
    order = np.argsort(~np.isin(want.state, (1, 2, 5)), kind="stable")
    V = handles(mesh)
    seen = set()
    cases = [(nbr, 10, 1e-12, 1) for nbr in (1, 2, 64, 65)]
    cases += [(65, rounds, tol, 1) for rounds in (1, 10) for tol in (0.0, 1e-12)]
    cases += [(65, 10, 1e-12, every) for every in (3, 1000)]
    for nbr, rounds, tol, every in cases:
        idx = order[:nbr]
        opt = dict(NOISE_OPT, rounds=rounds, tol=tol, every=every)
        w = separators_numpy(mesh, b, pos, kind, normal, pair[idx], arc[idx], **opt)
        got, n = sep_call(hip, V, b, pos, kind, normal, pair[idx], arc[idx], opt, int(w.offsets[-1]))
        same_sep(got, w, "%s nbr %d rounds %d tol %g every %d" % (mname, nbr, rounds, tol, every))
        check_structure(got, pos, pair[idx], every)
        seen |= set(got.state.tolist())
        if tol == 0.0 or rounds == 1:
            assert not np.any(np.isin(got.state, (1, 2))) and UNRESOLVED in got.state
        if (rounds, tol, every) == (10, 1e-12, 1) and nbr in (1, 2, 65):
            # the host entry: an odd and an even number of 4-byte entries in front of 8-byte data in its staging buffer
            host, n = sep_call(hip, V, b, pos, kind, normal, pair[idx], arc[idx], opt, int(w.offsets[-1]), device=False)
            same_sep(host, w, "%s nbr %d, host entry" % (mname, nbr))
    assert FOUND in seen
    # an odd number of nulls (the 4-byte kind in front of 8-byte data): the arrays of the nulls cut to 3, the brackets
    # among them, the restatement on the same cut arrays
    idx = np.nonzero(np.all(pair < 3, axis=1))[0]
    assert len(pos) > 3 and len(idx) >= 1
    w = separators_numpy(mesh, b, pos[:3], kind[:3], normal[:3], pair[idx], arc[idx], **NOISE_OPT)
    for device in (True, False):
        got, n = sep_call(hip, V, b, pos[:3], kind[:3], normal[:3], pair[idx], arc[idx], NOISE_OPT, int(w.offsets[-1]),
                          device=device)
        assert n == int(w.offsets[-1])
        same_sep(got, w, "%s 3 nulls, %d brackets, device %s" % (mname, len(idx), device))


# ---------------------------------------------------------------------------------------------------------------
# 3. capacity
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", list(MESHES))
def test_capacity(hip, handles, mname):
    """offsets and total do not depend on max_points; the slots below it are those of the full result, everything at
    and beyond it is untouched (sep_call's arena and host checks)"""
    mesh, b, pos, _jac, kind, normal, pair, arc, full = noise_case(mname, [5, 5, 5], 4)
    order = np.argsort(~np.isin(full.state, (1, 2, 5)), kind="stable")[:40]
    V = handles(mesh)
    for every in (1, 2):
        opt = dict(NOISE_OPT, every=every)
        want = separators_numpy(mesh, b, pos, kind, normal, pair[order], arc[order], **opt)
        total = int(want.offsets[-1])
        assert total > 45
        for device in (True, False):
            for with_bpt in (True, False):
                w = want if with_bpt else want._replace(bpt=np.zeros_like(want.bpt))
                for cap in (0, 1, total - 1, total, total + 3):
                    got, n = sep_call(hip, V, b, pos, kind, normal, pair[order], arc[order], opt, cap, with_bpt=with_bpt,
                                      device=device)
                    assert n == total
                    same_sep(got, w, "%s capacity %d device %s" % (mname, cap, device), upto=min(cap, total))
                    assert len(got.points) == min(cap, total)


# ---------------------------------------------------------------------------------------------------------------
# 4. the scratch a larger call left, and the chain from the skeleton entry
# ---------------------------------------------------------------------------------------------------------------
def test_small_call_on_the_scratch_of_a_larger_one(hip, handles):
    mesh, b, pos, _jac, kind, normal, pair, arc, want = noise_case("aniso", [7, 5, 9], 1)
    run = Runner(hip, handles)
    same_sep(run(mesh, b, pos, kind, normal, pair, arc, **NOISE_OPT), want, "%d brackets" % len(pair))
    k = int(np.nonzero(want.state == FOUND)[0][0])
    one = separators_numpy(mesh, b, pos, kind, normal, pair[[k]], arc[[k]], **NOISE_OPT)
    for name in NAMES[:NPER]:
        assert getattr(one, name)[0].tobytes() == getattr(want, name)[k].tobytes(), name
    same_sep(run(mesh, b, pos, kind, normal, pair[[k]], arc[[k]], **NOISE_OPT), one, "one bracket after")


@pytest.mark.parametrize("mname", list(MESHES))
def test_chain_from_skeleton_device(hip, mname):
    """ndsm_hip_vecpot_skeleton_device writes kind and normal into device arrays; ndsm_hip_vecpot_separators_device
    reads those very arrays, and pos: nothing crosses to the host in between"""
    import ndsm_amd
    mesh, b, pos, jac, kind, normal, pair, arc, want = noise_case(mname, [5, 5, 5], 4)
    n, nbr, nring = len(pos), len(pair), 4
    L = 2 + nring
    ring = default_ring(nring)
    sk = skeleton_numpy(mesh, b, pos, jac, ring, 0.5, 0.5, 0.5, 50, 1)
    assert sk.kind.tobytes() == kind.tobytes() and sk.normal.tobytes() == normal.tobytes()
    stot, total = int(sk.offsets[-1]), int(want.offsets[-1])
    V = ndsm_amd.VecPot(*mesh)
    lib = V.L
    i32 = np.int32
    host = {"B": np.ascontiguousarray(b, dtype=np.float64).reshape(-1), "pos": pos.copy(), "jac": jac.copy(), "ring": ring,
            "kind": np.zeros(n, dtype=i32), "eig": np.zeros((n, 3)), "spine": np.zeros((n, 3)), "normal": np.zeros((n, 3)),
            "ends": np.zeros((n * L, 3)), "length": np.zeros(n * L), "status": np.zeros(n * L, dtype=i32),
            "nsteps": np.zeros(n * L, dtype=i32), "hit": np.zeros(n * L, dtype=i32),
            "offsets": np.zeros(n * L + 1, dtype=np.int64), "points": np.zeros((stot, 3)), "bpt": np.zeros((stot, 3)),
            "pair": pair, "arc": arc}
    sep = {"state": np.zeros(nbr, dtype=i32), "nrounds": np.zeros(nbr, dtype=i32), "coef": np.zeros((nbr, 4)),
           "width": np.zeros(nbr), "side": np.zeros(nbr, dtype=i32), "dmin": np.zeros((nbr, 2)),
           "ends": np.zeros((nbr, 3)), "length": np.zeros(nbr), "status": np.zeros(nbr, dtype=i32),
           "nsteps": np.zeros(nbr, dtype=i32), "offsets": np.zeros(nbr + 1, dtype=np.int64),
           "points": np.zeros((total, 3)), "bpt": np.zeros((total, 3))}
    d, ds = {}, {}
    try:
        for where, arrays in ((d, host), (ds, sep)):
            for k, a in arrays.items():
                where[k] = ctypes.c_void_p()
                assert lib.ndsm_hip_device_alloc(a.nbytes, ctypes.byref(where[k])) == 0
        for k in ("B", "pos", "jac", "ring", "pair", "arc"):
            assert lib.ndsm_hip_memcpy_h2d(d[k], host[k].ctypes.data, host[k].nbytes) == 0
        tot = np.zeros(1, dtype=np.int64)
        rc = lib.ndsm_hip_vecpot_skeleton_device(
            V.h, d["B"], n, d["pos"], d["jac"], nring, d["ring"], 0.5, 0.5, 0.5, 50, 1, stot,
            *[d[k] for k in SKEL_NAMES[:10]], tot.ctypes.data, d["points"], d["bpt"])
        assert rc == 0 and tot[0] == stot, (rc, tot, hip.last_error(lib))
        rc = lib.ndsm_hip_vecpot_separators_device(
            V.h, d["B"], n, d["pos"], d["kind"], d["normal"], nbr, d["pair"], d["arc"], 0.5, 0.5, 0.5, 50, 10, 1e-12, 1,
            total, *[ds[k] for k in NAMES[:NPER + 1]], tot.ctypes.data, ds["points"], ds["bpt"])
        assert rc == 0 and tot[0] == total, (rc, tot, hip.last_error(lib))
        for k in NAMES:
            assert lib.ndsm_hip_memcpy_d2h(sep[k].ctypes.data, ds[k], sep[k].nbytes) == 0
    finally:
        for p in list(d.values()) + list(ds.values()):
            lib.ndsm_hip_device_free(p)
        V.close()
    same_sep(Sep(*[sep[k] for k in NAMES]), want, "chain " + mname)


# ---------------------------------------------------------------------------------------------------------------
# 5. the Python layer
# ---------------------------------------------------------------------------------------------------------------
def as_sep(S, nrounds):
    fl = S.paths.lines
    return Sep(S.state, nrounds, S.coef, S.width, S.side, S.dmin, fl.ends, fl.length, fl.status, fl.nsteps,
               S.paths.offsets, S.paths.points, S.paths.b if S.paths.b is not None else np.zeros((len(S.paths.points), 3)))


def test_python_separators(hip):
    import ndsm_amd
    mesh = uniform_mesh([12, 14, 11])
    b, _rc, pos, kind, normal, jac = crossing_case(mesh)
    pair, arc = ring_brackets(ring_of(8), [(0, 1), (1, 0)])
    opt = dict(CROSS_OPT)
    want = separators_numpy(mesh, b, pos, kind, normal, pair, arc, **opt)
    kw = dict(radius=1.0, capture=0.5, max_steps=400)
    V = ndsm_amd.VecPot(*mesh)
    try:
        sk = V.skeleton(b, nulls=(pos, jac), nring=8, **kw)
        assert sk.kind.tolist() == kind.tolist() and sk.normal.tobytes() == normal.tobytes()
        for device in (False, True):
            S = V.separators(b, skeleton=sk, device=device, **kw)
            assert S.pair.tolist() == pair.tolist()
            same_sep(as_sep(S, want.nrounds), want, "python, device %s" % device)
        S = V.separators(b, skeleton=sk, pairs=[(1, 0)], values=False, **kw)
        assert S.paths.b is None and S.state.tolist() == want.state[8:].tolist()
        S = V.separators(b, skeleton=sk, brackets=(pair[[5]], arc[[5]]), every=3, **kw)
        w5 = separators_numpy(mesh, b, pos, kind, normal, pair[[5]], arc[[5]], **dict(opt, every=3))
        same_sep(as_sep(S, w5.nrounds), w5, "python, one bracket")
        # skeleton=None: the nulls and the skeleton entries run first (two nulls, x order is cell order here)
        S = V.separators(b, **kw)
        assert np.bincount(S.state, minlength=6).tolist() == [0, 2, 2, 28, 0, 0]
    finally:
        V.close()
    S = ndsm_amd.find_separators(*mesh, b, skeleton=sk, **kw)
    same_sep(as_sep(S, want.nrounds), want, "find_separators")
    lines = ndsm_amd.separator_of(S, 0, 1)
    f = int(np.nonzero(want.state[:8] == FOUND)[0][0])
    assert len(lines) == 1 and lines[0][0].tobytes() == want.points[want.offsets[f]:want.offsets[f + 1]].tobytes()
    assert len(ndsm_amd.separator_of(S, 1, 0)) == 1 and ndsm_amd.separator_of(S, 0, 0) == []


# ---------------------------------------------------------------------------------------------------------------
# 6. the C entries reject bad input, and write nothing
# ---------------------------------------------------------------------------------------------------------------
def reject(hip, V, b, pos, kind, normal, pair, arc, code, device, missing=None, nnulls=None, nbr=None, cap=50,
           **over):
    """the entry returns `code` and clears total; the device entry changes no byte of the allocation, the host entry
    clears its outputs and leaves its inputs alone"""
    opt = dict(NOISE_OPT, **over)
    total = np.full(1, FILL, dtype=np.int64)
    outs, pts = out_slots(len(pair), cap + 2 if (not device and cap > 0) else max(cap, 1))
    slots = ([slot("B", b.reshape(-1), field=True), slot("pos", pos), slot("kind", kind), slot("normal", normal),
              slot("pair", pair), slot("arc", arc)] + [slot(name, a, output=True) for name, a in outs + pts])
    names = [s.name for s in slots]
    nn = len(pos) if nnulls is None else nnulls
    nb = len(pair) if nbr is None else nbr
    entry = V.L.ndsm_hip_vecpot_separators_device if device else V.L.ndsm_hip_vecpot_separators

    def call(*p):
        p = [None if names[i] == missing else q for i, q in enumerate(p)]
        return entry(V.h, p[0], nn, p[1], p[2], p[3], nb, p[4], p[5], opt["radius"], opt["capture"], opt["step"],
                     opt["max_steps"], opt["rounds"], opt["tol"], opt["every"], cap, *p[6:17],
                     None if missing == "total" else total.ctypes.data, p[17], p[18])
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
            elif nb == len(pair):
                assert s.name == missing or not np.any(a), s.name
    assert rc == code, (rc, hip.last_error(V.L))
    assert total[0] == (FILL if missing == "total" else 0)


def test_c_entries_reject_bad_input(hip):
    import ndsm_amd
    mesh, b, pos, _jac, kind, normal, pair, arc, _want = noise_case("aniso", [5, 5, 5], 4)
    pair, arc = pair[:6], arc[:6]
    V = ndsm_amd.VecPot(*mesh)
    try:
        for device in (True, False):
            for kw in (dict(nnulls=-1), dict(nnulls=0), dict(nbr=-1), dict(every=0), dict(every=-3), dict(cap=-1),
                       dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
                       dict(capture=0.0), dict(capture=-0.5), dict(capture=float("nan")), dict(capture=float("inf")),
                       dict(step=0.0), dict(step=float("nan")), dict(max_steps=0), dict(rounds=0), dict(rounds=-2),
                       dict(tol=-1e-12), dict(tol=float("nan")), dict(tol=float("inf"))):
                reject(hip, V, b, pos, kind, normal, pair, arc, 9004, device, **kw)
            # a pair index out of range, in the first and in the last bracket: nothing is written
            for at, bad in (((0, 0), -1), ((5, 1), len(pos)), ((3, 0), 2 ** 31 - 1)):
                p = pair.copy()
                p[at] = bad
                reject(hip, V, b, pos, kind, normal, p, arc, 9004, device)
            reject(hip, V, b, pos, kind, normal, pair, arc, 9004, device, nnulls=int(pair.max()))
            for missing in ("B", "pos", "kind", "normal", "pair", "arc", "state", "nrounds", "coef", "width", "side",
                            "dmin", "ends", "length", "status", "nsteps", "offsets", "total", "points"):
                reject(hip, V, b, pos, kind, normal, pair, arc, 9002, device, missing=missing)
        # no brackets: success, total 0, nothing else touched
        total = np.full(1, FILL, dtype=np.int64)
        for entry in (V.L.ndsm_hip_vecpot_separators, V.L.ndsm_hip_vecpot_separators_device):
            total[0] = FILL
            assert entry(V.h, None, 4, None, None, None, 0, None, None, 0.5, 0.5, 0.5, 50, 10, 1e-12, 1, 50,
                         *[None] * 11, total.ctypes.data, None, None) == 0
            assert total[0] == 0
    finally:
        V.close()
