"""CPU tests of the null-point semantics: the closed-form checks of test_gpu_nulls.py run with the numpy restatement
(null_model.nulls_numpy) behind the library's own Python layer, and the screen is checked against running the Newton
stage on EVERY cell: it must lose no null."""
import numpy as np
import pytest

from golden_inputs import aniso_mesh, uniform_mesh
from line_model import abc
from null_model import (LINEAR, PLACES, check_failure_ends, check_linear, check_near_plane, check_no_nulls, check_null_pair,
                        check_second_start, linear_field, model_run, null_pair, nulls_numpy, numpy_tracer, place,
                        same_records, second_start_cell, smooth_noise, spine_approach)

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
SHAPE = [13, 11, 12]


@pytest.mark.parametrize("mname", list(MESHES))
@pytest.mark.parametrize("where", list(PLACES))
@pytest.mark.parametrize("name", list(LINEAR))
def test_model_linear_nulls(mname, name, where):
    raw = check_linear(model_run, MESHES[mname](SHAPE), name, where)
    assert np.all(raw.residual >= 0.0)


@pytest.mark.parametrize("mname", list(MESHES))
def test_model_null_pair(mname):
    for n in (16, 32):
        check_null_pair(model_run, MESHES[mname], n)


@pytest.mark.parametrize("mname", list(MESHES))
def test_model_no_nulls_and_failure_ends(mname):
    mesh = MESHES[mname](SHAPE)
    check_no_nulls(model_run, mesh)
    check_failure_ends(model_run, mesh)
    check_near_plane(model_run, mesh)


@pytest.mark.parametrize("mname", list(MESHES))
def test_model_second_start(mname):
    """the constructed cell needs a start other than the centre; with the centre start alone the null is missed"""
    mesh = MESHES[mname](SHAPE)
    raw = check_second_start(model_run, mesh)
    cell = 5 + SHAPE[0] * (4 + SHAPE[1] * 6)
    b, _r0 = second_start_cell(mesh)
    out = nulls_numpy(mesh, b, 4096)
    assert out[7][out[1].tolist().index(cell)] // 32 >= 1
    assert cell not in nulls_numpy(mesh, b, 4096, nstarts=1)[1].tolist()
    assert len(raw.cell) >= 1


@pytest.mark.parametrize("mname", list(MESHES))
def test_model_screen_loses_no_null(mname):
    """Newton on every cell, with no screen, accepts exactly the cells it accepts behind the screen, with the same
    records: on the ABC field, on it plus smooth noise, on linear nulls at every placement and on the null pair"""
    mesh = MESHES[mname]([14, 12, 13])
    fields = [abc(mesh, k=2.0 * np.pi), abc(mesh, k=2.0 * np.pi) + smooth_noise(mesh, 7, 0.4), null_pair(mesh)[0]]
    fields += [linear_field(mesh, LINEAR[name][0], place(mesh, where)) for name in LINEAR for where in PLACES]
    total = 0
    for b in fields:
        a = nulls_numpy(mesh, b, 10 ** 6)
        e = nulls_numpy(mesh, b, 10 ** 6, screen=False)
        assert same_records(a, e)
        assert a[0][1] <= a[0][0]
        total += int(a[0][1])
    assert total >= len(LINEAR) * 15


@pytest.mark.parametrize("mname", list(MESHES))
def test_model_order_truncation_and_counts(mname):
    mesh = MESHES[mname]([14, 12, 13])
    b = abc(mesh, k=2.0 * np.pi)
    full = nulls_numpy(mesh, b, 10 ** 6)
    nf = int(full[0][1])
    assert nf >= 3 and np.all(np.diff(full[1]) > 0)
    cut = nulls_numpy(mesh, b, 2)
    assert np.array_equal(cut[0], full[0]) and all(len(a) == 2 for a in cut[1:])
    assert same_records(cut[1:], [a[:2] for a in full[1:]])
    none = nulls_numpy(mesh, b, 0)
    assert np.array_equal(none[0], full[0]) and all(len(a) == 0 for a in none[1:])
    # iters: the start number times 32 plus 1 .. 20 iterations
    assert np.all((full[7] % 32 >= 1) & (full[7] % 32 <= 20) & (full[7] // 32 <= 8))
    # the records hold nulls of the interpolant: |B| there is at rounding level
    assert np.all(full[5] <= 1e-10)
    assert np.all(full[6] == -np.sign(full[4]).astype(np.int32))


def test_model_spine_approach():
    for mname in MESHES:
        d = spine_approach(model_run, numpy_tracer, MESHES[mname](SHAPE))
        assert d[1] < d[0]
