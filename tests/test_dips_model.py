"""CPU tests of the dip semantics (include/ndsm_hip.h, ndsm_hip_vecpot_dips) on their numpy restatement
(dips_model.dips_numpy) behind the library's own Python layer: the closed forms that test_gpu_dips.py runs with the
device - all linear, so that the difference quotient and the edge interpolation reproduce them to rounding -, on a
uniform mesh and on golden_inputs.aniso_mesh (unequal spacings, no origin at 0, unequal nx, ny, nz)."""
import numpy as np
import pytest

from dips_model import (bad_value_fields, bald_subset, bitwise_fields, check_bad_values, check_on_node_plane, check_rope,
                        check_tilted, dips_numpy, model_run, rope, same_records, white_noise, inside)
from golden_inputs import aniso_mesh, uniform_mesh

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
SHAPES = {"uniform": [24, 30, 20], "aniso": [33, 22, 27]}


@pytest.mark.parametrize("mname", list(MESHES))
def test_dips_rope_along_y(mname):
    check_rope(model_run, MESHES[mname](SHAPES[mname]), "y")


@pytest.mark.parametrize("mname", list(MESHES))
def test_dips_rope_along_x(mname):
    check_rope(model_run, MESHES[mname](SHAPES[mname]), "x")


@pytest.mark.parametrize("mname", list(MESHES))
def test_dips_tilted_zero_surface(mname):
    check_tilted(model_run, MESHES[mname](SHAPES[mname]))


@pytest.mark.parametrize("mname", list(MESHES))
def test_dips_zero_on_a_node_plane(mname):
    check_on_node_plane(model_run, MESHES[mname](SHAPES[mname]))


@pytest.mark.parametrize("mname", list(MESHES))
def test_dips_plane_only_is_the_bald_subset(mname):
    """(e): the records of plane_only are, bit for bit, the records of the full call with flag bit 0, and
    counts[1] == counts[2]"""
    mesh = MESHES[mname](SHAPES[mname])
    lo, hi = mesh[2][0], mesh[2][-1]
    fields = list(bitwise_fields(mesh)) + [("rope", rope(mesh, 1.3, 0.225 * (hi - lo), 0.7, inside(mesh, 0, 4),
                                                         inside(mesh, 2, len(mesh[2]) // 2, 0.41))),
                                           ("white noise", white_noise(SHAPES[mname]))]
    for name, b in fields:
        full, plane = dips_numpy(mesh, b), dips_numpy(mesh, b, plane_only=True)
        print(mname, name, "full", full[0], "plane", plane[0])
        assert plane[0][1] == plane[0][2] == full[0][2] > 0, name
        assert plane[0][0] <= full[0][0]
        assert same_records(plane[1:], bald_subset(full)[1:]), name
        assert np.all(plane[6] == 1)
        # and the capacity only truncates
        cut = dips_numpy(mesh, b, max_dips=5)
        assert np.array_equal(cut[0], full[0]) and same_records(cut[1:], tuple(a[:5] for a in full[1:]))


@pytest.mark.parametrize("mname", list(MESHES))
def test_dips_bad_values(mname):
    """(f): NaN and Inf blocks over the zero surface and an all-zero field give no dip, and nothing that is written
    is non-finite"""
    mesh = MESHES[mname](SHAPES[mname])
    for name, b, _ncross in check_bad_values(model_run, mesh):
        out = dips_numpy(mesh, b)
        for a in out[1:]:
            assert len(a) == 0, name
        assert out[0][1] == out[0][2] == 0
    # zero and NaN blocks in a field with dips: every value that enters t or curv is finite in every record (grad_z
    # does not enter them, and is NaN in the records next to the NaN block); a lone Inf is the caller's to mask
    for name, b in bitwise_fields(mesh):
        out = dips_numpy(mesh, b)
        assert out[0][1] > 0
        if "Inf" not in name:
            for a in (out[2], out[3], out[4][:, :2], out[5]):
                assert np.all(np.isfinite(a)), name


def test_dips_white_noise_density():
    """about a quarter of all edges are dips: half of them are crossings, half of those have curv > 0"""
    shape = [40, 36, 44]
    out = dips_numpy(uniform_mesh(shape), white_noise(shape))
    nx, ny, nz = shape
    nedges = (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1)
    print("white noise: edges", nedges, "counts", out[0])
    assert 0.45 < out[0][0] / nedges < 0.55 and 0.2 < out[0][1] / nedges < 0.3
    assert np.all(np.diff(out[1]) > 0)
