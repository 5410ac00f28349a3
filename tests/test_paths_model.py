"""CPU tests of the numpy restatement of the path semantics (path_model.path_numpy): its trace outputs are
line_model.trace_numpy's bit for bit, every stored point is the end of a shorter trace - which ties it to the model the
device is already pinned to -, and the closed forms of path_checks.py hold for it.  The GPU tests compare the device with
this restatement bit for bit (test_gpu_paths.py)."""
import numpy as np
import pytest

import path_checks
from golden_inputs import aniso_mesh, uniform_mesh
from line_model import FACES, NULL, UNFINISHED, abc, face_seeds, inner_seeds, trace_numpy
from path_model import join, npts_of, path_numpy, paths_numpy, take

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
STEP, MAX_STEPS = 0.37, 300
EVERYS = (1, 2, 3, 7, 1000)


def line_case(mname, ns):
    """test_gpu_caller_arrays.line_case's fields and 41 seeds (that module needs a GPU library to import)"""
    mesh = MESHES[mname](ns)
    b, g = abc(mesh), abc(mesh, k=0.7 * np.pi, phase=0.3)
    rng = np.random.default_rng(5)
    seeds = np.concatenate([inner_seeds(mesh, rng, 29), face_seeds(mesh, rng, 2)])
    return mesh, b, g, seeds


def model_runner(mesh, b, g, seeds, step, max_steps, direction, every):
    return paths_numpy(mesh, b, g, seeds, step, max_steps, direction, every)


def test_npts_formula():
    assert npts_of([0, 1, 2, 3, 4, 5, 6, 7], 1).tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
    assert npts_of([0, 1, 2, 3, 4, 5, 6, 7], 3).tolist() == [1, 2, 2, 2, 3, 3, 3, 4]
    assert npts_of([0, 1, 50, 300], 1000).tolist() == [1, 2, 2, 2]


@pytest.mark.parametrize("ns", ([4, 4, 4], [5, 4, 67]), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mname", list(MESHES))
def test_trace_outputs_and_prefix_property(mname, ns):
    """the five trace outputs are trace_numpy's; point j every of a line and its running integral are ends and integral
    of trace_numpy called with max_steps = j every, for all j; B and G at a point are those of a one-point path from
    it"""
    mesh, b, g, seeds = line_case(mname, ns)
    longest, statuses = 0, set()
    for sgn in (1.0, -1.0):
        for withg in (True, False):
            want = trace_numpy(mesh, b, g if withg else None, seeds, STEP, MAX_STEPS, sgn)
            by_every = {}
            for every in EVERYS:
                p = path_numpy(mesh, b, g if withg else None, seeds, STEP, MAX_STEPS, sgn, every)
                for k in range(5):
                    assert p[k].tobytes() == want[k].tobytes(), (sgn, withg, every, k)
                path_checks.check_structure(p, seeds, int(sgn), every)
                if not withg:
                    assert not np.any(p.gpt) and not np.any(p.ipt)
                by_every[every] = p
            for every in EVERYS[1:]:
                path_checks.check_stride(by_every[1], by_every[every], every)
            p = by_every[1]
            assert not np.any(np.isin(p.status, (NULL, UNFINISHED)))
            longest = max(longest, int(p.nsteps.max()))
            statuses |= set(p.status.tolist())
            if not withg:
                continue
            # the prefix property, for every j at once: the trace cut at j steps ends at point j of each line that
            # takes more than j steps
            for j in range(1, int(p.nsteps.max())):
                cut = trace_numpy(mesh, b, g, seeds, STEP, j, sgn)
                has = np.nonzero(p.nsteps > j)[0]
                rows = p.offsets[has] + j
                assert p.points[rows].tobytes() == cut[0][has].tobytes(), (sgn, j)
                assert p.ipt[rows].tobytes() == cut[2][has].tobytes(), (sgn, j)
            # B and G at the points: the first point of a path seeded there
            at = path_numpy(mesh, b, g, p.points, STEP, 1, sgn, 1)
            first = at.offsets[:-1]
            assert at.bpt[first].tobytes() == p.bpt.tobytes() and at.gpt[first].tobytes() == p.gpt.tobytes()
    total = {e: sum(int(paths_numpy(mesh, b, g, seeds, STEP, MAX_STEPS, 0, e).offsets[-1]) for _ in (0,))
             for e in (1, 1000)}
    print(mname, ns, "longest line", longest, "steps; total points", total)
    assert statuses >= set(FACES)
    assert 12 <= longest <= 27 and 403 <= total[1] <= 821 and total[1000] == 164


def test_join_and_take():
    mesh, b, g, seeds = line_case("aniso", [5, 5, 5])
    both = paths_numpy(mesh, b, g, seeds, STEP, MAX_STEPS, 0, 2)
    fwd = path_numpy(mesh, b, g, seeds, STEP, MAX_STEPS, 1.0, 2)
    bwd = path_numpy(mesh, b, g, seeds, STEP, MAX_STEPS, -1.0, 2)
    idx = np.array([3, 0, 3, 40])
    sub = path_numpy(mesh, b, g, seeds[idx], STEP, MAX_STEPS, 1.0, 2)
    for k in range(10):
        assert both[k].tobytes() == join([fwd, bwd])[k].tobytes()
        assert take(fwd, idx)[k].tobytes() == sub[k].tobytes()           # a line depends on its own seed only


@pytest.mark.parametrize("mname", list(MESHES))
def test_uniform_field(mname):
    path_checks.check_uniform(model_runner, MESHES[mname]([9, 8, 10]))


@pytest.mark.parametrize("mname", list(MESHES))
def test_helical_field(mname):
    path_checks.check_helical(model_runner, MESHES[mname]([12, 14, 11]))


@pytest.mark.parametrize("mname", list(MESHES))
def test_other_ends(mname):
    path_checks.check_other_ends(model_runner, MESHES[mname]([12, 11, 10]))


@pytest.mark.parametrize("mname", list(MESHES))
def test_whole_line(mname):
    path_checks.check_whole_line(model_runner, MESHES[mname]([9, 8, 10]))
