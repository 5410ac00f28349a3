"""CPU tests of the separator semantics: the closed-form checks of test_gpu_separators.py run on the numpy restatement
(separator_model.separators_numpy) - the crossing field of DESIGN.md, whose separator is a segment of a mesh axis -, the
property that ties a bracket's line to the skeleton entry (skeleton_model.skeleton_numpy, bit for bit), and the states
a bracket can end in.  Every state 0 .. 5 must occur over the file."""
import numpy as np
import pytest

from golden_inputs import aniso_mesh, uniform_mesh
from skeleton_model import CAPTURED, NONE, noise_nulls, skeleton_numpy, type_numpy
from separator_model import (CROSS_OPT, FAR, FOUND, GAP, NO_CROSSING, OFF_AXIS, SEP_NONE, UNRESOLVED, check_crossing,
                             check_property, check_structure, crossing_case, opposite_pairs, ring_brackets, ring_of,
                             separators_numpy)

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
CROSSING_CASES = [("uniform", [24, 30, 20]), ("uniform", [12, 14, 11]), ("aniso", [33, 22, 27])]
CASE_ID = lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v)   # noqa: E731
SEEN = set()


@pytest.mark.parametrize("rot", (0.0, 0.3))
@pytest.mark.parametrize("mname,shape", CROSSING_CASES, ids=CASE_ID)
def test_model_crossing_field(mname, shape, rot):
    """two changes of side per ring, the one facing the other null FOUND within 8 rounds and on the axis, the other
    FAR; with the ring rotated by 0.3 rad the change does not sit in the middle of its arc; and the header's property"""
    mesh = MESHES[mname](shape)
    history = []
    sp, pair, _arc = check_crossing(lambda *a, **k: separators_numpy(*a, history=history, **k), mesh, rot)
    SEEN.update(sp.state.tolist())
    assert check_crossing.worst <= OFF_AXIS
    b, _rc, pos, _kind, _normal, jac = crossing_case(mesh)
    n = check_property(sp, skeleton_numpy, mesh, b, pos, jac, pair, CROSS_OPT["radius"], CROSS_OPT["capture"],
                       CROSS_OPT["step"], CROSS_OPT["max_steps"], CROSS_OPT["every"])
    assert n == 4
    # round 1 of a FOUND bracket: i* = 32 for the symmetric ring, another lane for the rotated one; from round 3 on
    # both sides of the change are captured, after 6 to 32 steps
    for l in np.nonzero(sp.state == FOUND)[0]:
        rounds = [(cls[list(idx).index(l)], cap[list(idx).index(l)], nst[list(idx).index(l)])
                  for idx, cls, cap, nst in history if l in idx]
        first = int(np.nonzero(rounds[0][0] != rounds[0][0][0])[0][0])
        assert (first == 32) == (rot == 0.0), first
        assert len(rounds) == sp.nrounds[l]
        for cls, cap, nst in rounds[2:]:
            k = int(np.nonzero(cls != cls[0])[0][0])
            assert cap[k - 1] and cap[k] and 6 <= nst[k - 1] <= 32 and 6 <= nst[k] <= 32, (cap, nst)


def test_model_every_and_tol():
    """every changes the stored points alone; tol = 0 never converges (the two sides of a change differ)"""
    mesh = uniform_mesh([12, 14, 11])
    b, _rc, pos, kind, normal, jac = crossing_case(mesh)
    pair, arc = ring_brackets(ring_of(8), [(0, 1)])
    base = separators_numpy(mesh, b, pos, kind, normal, pair, arc, **CROSS_OPT)
    for every in (3, 1000):
        sp = separators_numpy(mesh, b, pos, kind, normal, pair, arc, **dict(CROSS_OPT, every=every))
        check_structure(sp, pos, pair, every)
        for k in range(10):
            assert sp[k].tobytes() == base[k].tobytes()
        assert check_property(sp, skeleton_numpy, mesh, b, pos, jac, pair, 1.0, 0.5, 0.5, 400, every) == 2
    sp = separators_numpy(mesh, b, pos, kind, normal, pair, arc, **dict(CROSS_OPT, tol=0.0, rounds=12))
    assert sorted(set(sp.state.tolist())) == [NO_CROSSING, UNRESOLVED]
    assert np.all(sp.nrounds[sp.state == UNRESOLVED] == 12) and np.all(sp.width[sp.state == UNRESOLVED] > 0.0)
    SEEN.update(sp.state.tolist())


def test_model_special_cases():
    mesh = uniform_mesh([12, 14, 11])
    b, _rc, pos, kind, normal, jac = crossing_case(mesh)
    pair, arc = ring_brackets(ring_of(8), [(0, 1)])
    full = separators_numpy(mesh, b, pos, kind, normal, pair, arc, **CROSS_OPT)
    f = int(np.nonzero(full.state == FOUND)[0][0])
    # rounds = 1: the brackets with a change are UNRESOLVED, 1/63 of their arc wide, and still carry their a-side line
    one = separators_numpy(mesh, b, pos, kind, normal, pair, arc, **dict(CROSS_OPT, rounds=1))
    check_structure(one, pos, pair, 1)
    assert np.array_equal(one.state == UNRESOLVED, np.isin(full.state, (FOUND, FAR)))
    assert np.array_equal(one.state == NO_CROSSING, full.state == NO_CROSSING) and np.all(one.nrounds == 1)
    w0 = np.hypot(*(arc[f, :2] - arc[f, 2:]))
    assert 0.9 * w0 / 63.0 <= one.width[f] <= 1.1 * w0 / 63.0
    assert one.status[f] != NONE and one.nsteps[f] >= 1
    assert check_property(one, skeleton_numpy, mesh, b, pos, jac, pair, 1.0, 0.5, 0.5, 400, 1) == 2
    # same-sign, equal and untyped pairs: NONE - one point with pos(m)'s bits, the input arc, zeros elsewhere
    pos3 = np.concatenate([pos, pos[[0]] + 0.01])
    kind3 = np.array([1, -1, 0], dtype=np.int32)
    normal3 = np.concatenate([normal, np.zeros((1, 3))])
    pair3 = np.array([[0, 0], [1, 1], [0, 2], [2, 1], [0, 1]], dtype=np.int32)
    arc3 = np.tile(arc[f], (5, 1))
    sp = separators_numpy(mesh, b, pos3, kind3, normal3, pair3, arc3, **CROSS_OPT)
    check_structure(sp, pos3, pair3, 1)
    assert sp.state.tolist() == [SEP_NONE] * 4 + [FOUND]
    assert sp.coef[:4].tobytes() == arc3[:4].tobytes() and not np.any(sp.width[:4]) and not np.any(sp.dmin[:4])
    assert not np.any(sp.side[:4]) and not np.any(sp.nrounds[:4]) and np.all(np.diff(sp.offsets)[:4] == 1)
    same = separators_numpy(mesh, b, pos3, np.array([1, 2, 0], dtype=np.int32), normal3, pair3[[4]], arc3[[4]],
                            **CROSS_OPT)
    assert same.state.tolist() == [SEP_NONE]
    # the bits of a bracket do not depend on the others
    for k in range(10):
        assert sp[k][4].tobytes() == full[k][f].tobytes()
    # an arc without a change of side: NO_CROSSING after one round
    assert NO_CROSSING in full.state and np.all(full.nrounds[full.state == NO_CROSSING] == 1)
    # an antipodal arc across the separator has no interior: its lanes fall on a and on b alone (up to rounding), so a
    # round leaves the change as wide as the arc - never FOUND in one round, and no lane is without a side (g = 0 counts
    # as the + side).  (Narrowing it further would interpolate between two opposite vectors: rounding noise.)
    anti = np.array([[np.cos(0.3), np.sin(0.3), -np.cos(0.3), -np.sin(0.3)]])
    sp = separators_numpy(mesh, b, pos, kind, normal, pair[[0]], anti, **dict(CROSS_OPT, rounds=1))
    assert sp.state.tolist() == [UNRESOLVED] and sp.nrounds[0] == 1, (sp.state, sp.nrounds)
    assert abs(sp.width[0] - 2.0) <= 1e-15
    # an arc one end of which lies outside the box has no side there: GAP, in lane 0 and in lane i* = 63
    for bad in (np.array([[1e6, 0.0, arc[f, 2], arc[f, 3]]]), np.array([[arc[f, 2], arc[f, 3], 1e6, 0.0]]),
                np.array([[np.nan, 0.0, arc[f, 2], arc[f, 3]]])):
        sp = separators_numpy(mesh, b, pos, kind, normal, pair[[0]], bad, **CROSS_OPT)
        check_structure(sp, pos, pair[[0]], 1)
        assert sp.state.tolist() == [GAP] and sp.nrounds[0] == 1 and sp.coef.tobytes() == bad.tobytes()
    SEEN.update([SEP_NONE, GAP])
    SEEN.update(one.state.tolist())
    # no brackets
    sp = separators_numpy(mesh, b, pos, kind, normal, pair[:0], arc[:0], **CROSS_OPT)
    check_structure(sp, pos, pair[:0], 1)
    assert sp.offsets.tolist() == [0]


@pytest.mark.parametrize("mname", list(MESHES))
@pytest.mark.parametrize("ns,narcs", (([5, 5, 5], 4), ([7, 5, 9], 1)), ids=CASE_ID)
def test_model_noise_nulls(mname, ns, narcs):
    """all opposite-sign pairs of the nulls of white noise (the four arcs of a 4-seed ring each, or the first of them),
    50 steps: lines of every end, at least four states, and the property on six lines of each state"""
    mesh = MESHES[mname](ns)
    b, pos, jac = noise_nulls(mesh)
    _ok, _s, kind, _eig, _v, normal, _e1, _e2 = type_numpy(jac)
    pair, arc = ring_brackets(ring_of(4), opposite_pairs(kind), narcs)
    assert len(pair) >= 8
    sp = separators_numpy(mesh, b, pos, kind, normal, pair, arc, 0.5, 0.5, 0.5, 50, 10, 1e-12, 1)
    check_structure(sp, pos, pair, 1)
    print(mname, ns, "brackets", len(pair), "states", np.bincount(sp.state, minlength=6), "status",
          np.bincount(sp.status, minlength=12))
    assert len(set(sp.state.tolist())) >= 4, np.bincount(sp.state, minlength=6)
    assert check_property(sp, skeleton_numpy, mesh, b, pos, jac, pair, 0.5, 0.5, 0.5, 50, 1, limit=6) >= 12
    SEEN.update(sp.state.tolist())


def test_model_zz_every_state_occurred():
    assert SEEN == set(range(6)), SEEN
    assert CAPTURED == 10 and NONE == 11
