"""GPU tests of null-point detection (run with -m gpu on an MI355X): VecPot.nulls, find_nulls and the two C entries.
The yardsticks are the numpy restatement of the semantics in include/ndsm_hip.h (null_model.nulls_numpy; counts and
every record field bit for bit) and closed forms (null_model's checks, which test_nulls_model.py runs with the
restatement): linear fields B = M (r - r0), which the interpolant reproduces, with r0 in a cell, on a face, an edge
and a node; a null pair with a derived position bound; fields without nulls; the ends where the iteration must fail;
and VecPot.trace running into a null that was found.  Every test runs on golden_inputs.aniso_mesh (unequal spacings, no
origin at 0) and on a uniform mesh, with unequal nx, ny, nz."""
import ctypes

import numpy as np
import pytest

from golden_inputs import aniso_mesh, uniform_mesh
from line_model import abc
from null_model import (LINEAR, PLACES, check_failure_ends, check_linear, check_near_plane, check_no_nulls,
                        check_null_pair, check_second_start, failure_fields, linear_field, nulls_numpy, place,
                        smooth_noise, spine_approach)

pytestmark = pytest.mark.gpu

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
SHAPES = {"uniform": [24, 30, 20], "aniso": [33, 22, 27]}
NAMES = ("counts", "cell", "pos", "jac", "det", "resid", "sign", "iters")


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def lib_run(mesh, b, **kw):
    import ndsm_amd
    V = ndsm_amd.VecPot(*mesh)
    try:
        return V.nulls(b, **kw)
    finally:
        V.close()


def lib_tracer(mesh, b, seeds, step, max_steps, sgn):
    import ndsm_amd
    V = ndsm_amd.VecPot(*mesh)
    try:
        return V.trace(b, seeds, step=step, max_steps=max_steps, direction="forward" if sgn > 0 else "backward").ends[0][0]
    finally:
        V.close()


def raw_call(hip, V, b, max_nulls, device=False, fill=0):
    """one call of a C entry on `fill`-initialised arrays of max_nulls slots: the tuple of nulls_numpy's layout, cut to
    the records written, and the arrays themselves"""
    L = V.L
    B = np.ascontiguousarray(b, dtype=np.float64).reshape(-1).copy()
    m = max(max_nulls, 1)
    counts = np.full(2, fill, dtype=np.int64)
    out = [np.full(m, fill, dtype=np.int64), np.full((m, 3), float(fill)), np.full((m, 3, 3), float(fill)),
           np.full(m, float(fill)), np.full(m, float(fill)), np.full(m, fill, dtype=np.int32),
           np.full(m, fill, dtype=np.int32)]
    if not device:
        rc = L.ndsm_hip_vecpot_nulls(V.h, B.ctypes.data, max_nulls, counts.ctypes.data, *[a.ctypes.data for a in out])
    else:
        rc = V._on_device([B] + out, lambda dB, *p: L.ndsm_hip_vecpot_nulls_device(V.h, dB, max_nulls,
                                                                                  counts.ctypes.data, *p))
    assert rc == 0, hip.last_error(L)
    n = min(int(counts[1]), max_nulls)
    return (counts,) + tuple(a[:n] for a in out), out


def assert_bitwise(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), (what, name)


def bitwise_fields(mesh):
    """(name, field): several nulls; smooth noise and an offset, fewer nulls among about as many candidates; a zero
    block and a NaN block (candidate-rich fields: test_nulls_bitwise_many_candidates_many_workgroups)"""
    b = abc(mesh, k=2.0 * np.pi)
    yield "abc", b
    yield "abc+noise", b + smooth_noise(mesh, 7, 0.4) + np.array([0.9, 0.0, 0.0])[:, None, None, None]
    c = b.copy()
    c[:, 3:8, 4:9, 5:10] = 0.0
    c[:, 11:15, 10:14, 12:16] = np.nan
    yield "abc, zero and NaN blocks", c


@pytest.mark.parametrize("mname", list(MESHES))
def test_nulls_bitwise_against_the_restatement(hip, mname):
    import ndsm_amd
    mesh = MESHES[mname](SHAPES[mname])
    V = ndsm_amd.VecPot(*mesh)
    try:
        for what, b in bitwise_fields(mesh):
            want = nulls_numpy(mesh, b, 4096)
            nc, nf = int(want[0][0]), int(want[0][1])
            print(mname, what, "candidates", nc, "nulls", nf)
            assert nf >= 2 and nc > nf
            got, _arrays = raw_call(hip, V, b, 4096)
            assert_bitwise(got, want, what)
            assert np.all(np.diff(got[1]) > 0)
            # the device entry, and the same call again
            dev, arrays = raw_call(hip, V, b, 4096, device=True, fill=7)
            assert_bitwise(dev, want, what + " (device entry)")
            for a in arrays:                                  # slots past the records are not touched
                assert np.all(a[nf:] == 7)
            again, _arrays = raw_call(hip, V, b, 4096)
            assert_bitwise(again, got, what + " (second call)")
            # a capacity that truncates: the first records in cell order, the same counts; and counting only
            cut, arrays = raw_call(hip, V, b, nf - 1, fill=7)
            assert_bitwise(cut, nulls_numpy(mesh, b, nf - 1), what + " (truncated)")
            assert_bitwise(cut[1:], tuple(a[:nf - 1] for a in want[1:]), what + " (truncated)")
            none, arrays = raw_call(hip, V, b, 0, fill=7)
            assert np.array_equal(none[0], want[0])
            for a in arrays:
                assert np.all(a == 7)
            none, arrays = raw_call(hip, V, b, 0, device=True, fill=7)
            assert np.array_equal(none[0], want[0])
        # the Python layer repeats a call whose capacity was too small, once
        b = abc(mesh, k=2.0 * np.pi)
        full, small = V.nulls(b, merge=None), V.nulls(b, max_nulls=1, merge=None)
        assert len(small.cell) == small.nfound == full.nfound >= 2
        assert np.array_equal(small.position, full.position) and np.array_equal(small.cell, full.cell)
        assert np.array_equal(V.nulls(b, device=True, merge=None).position, full.position)
        count = V.nulls(b, max_nulls=0)
        assert (count.ncandidates, count.nfound, len(count.cell)) == (full.ncandidates, full.nfound, 0)
        assert np.array_equal(ndsm_amd.find_nulls(*mesh, b, merge=None).position, full.position)
    finally:
        V.close()


# white noise: nearly every cell is a candidate and a third of them hold a null, found from every one of the nine
# starts - tens of thousands of records over hundreds of Newton workgroups; the last mesh has more than 2^20 nodes
# and more than 2^18 candidates, so that both scans give every lane a run of several counts
MANY = {"uniform": (uniform_mesh, [40, 36, 44]), "aniso": (aniso_mesh, [41, 38, 35]), "large": (aniso_mesh, [112, 100, 96])}


@pytest.mark.parametrize("mname", list(MANY))
def test_nulls_bitwise_many_candidates_many_workgroups(hip, mname):
    """counts and records equal the restatement's where the candidate list, the accepted mask and both exclusive
    sums span many workgroups, with capacities that cut inside a later workgroup"""
    import ndsm_amd
    meshf, shape = MANY[mname]
    mesh = meshf(shape)
    b = np.random.default_rng(3).uniform(-1.0, 1.0, (3, shape[2], shape[1], shape[0]))
    want = nulls_numpy(mesh, b, 10 ** 7)
    nc, nf = int(want[0][0]), int(want[0][1])
    print(mname, "candidates", nc, "nulls", nf, "starts used", np.bincount(want[7] // 32, minlength=9))
    assert nc > 40000 and nf > 10000 and np.all(np.bincount(want[7] // 32, minlength=9) > 0)
    if mname == "large":
        assert np.prod(shape) > 2 ** 20 and nc > 2 ** 18
    V = ndsm_amd.VecPot(*mesh)
    try:
        got, _arrays = raw_call(hip, V, b, nf + 5)
        assert_bitwise(got, want, mname)
        assert np.all(np.diff(got[1]) > 0)
        dev, arrays = raw_call(hip, V, b, nf + 5, device=True, fill=7)
        assert_bitwise(dev, want, mname + " (device entry)")
        for a in arrays:
            assert np.all(a[nf:] == 7)
        for cap in (nf // 2 + 3, 257, 1):
            cut, _arrays = raw_call(hip, V, b, cap, fill=7)
            assert np.array_equal(cut[0], want[0])
            assert_bitwise(cut[1:], tuple(a[:cap] for a in want[1:]), "%s (capacity %d)" % (mname, cap))
        none, _arrays = raw_call(hip, V, b, 0)
        assert np.array_equal(none[0], want[0])
        # and a field with few candidates afterwards, on the scratch the large call left behind
        small = b.copy()
        small[0] = np.abs(small[0]) + 0.1
        small[0, 5:20, 5:20, 5:20] = b[0, 5:20, 5:20, 5:20]
        got, _arrays = raw_call(hip, V, small, 4096)
        assert_bitwise(got, nulls_numpy(mesh, small, 4096), mname + " (small after large)")
        assert 0 < got[0][1] < nf
    finally:
        V.close()


@pytest.mark.parametrize("mname", list(MESHES))
def test_nulls_bitwise_on_closed_form_fields(hip, mname):
    """the records of the linear nulls at every placement, bit for bit (shared faces, edges and nodes included)"""
    import ndsm_amd
    mesh = MESHES[mname](SHAPES[mname])
    V = ndsm_amd.VecPot(*mesh)
    try:
        for name in LINEAR:
            for where in PLACES:
                b = linear_field(mesh, LINEAR[name][0], place(mesh, where))
                got, _arrays = raw_call(hip, V, b, 64)
                assert_bitwise(got, nulls_numpy(mesh, b, 64), name + " " + where)
    finally:
        V.close()


@pytest.mark.parametrize("mname", list(MESHES))
@pytest.mark.parametrize("where", list(PLACES))
@pytest.mark.parametrize("name", list(LINEAR))
def test_nulls_linear_fields(hip, mname, name, where):
    check_linear(lib_run, MESHES[mname](SHAPES[mname]), name, where)


@pytest.mark.parametrize("mname", list(MESHES))
def test_nulls_null_pair(hip, mname):
    """exactly two nulls at n = 16, 32, 64, |dx| <= 1.1 h_x^2 / (8 a), y and z exact to 1e-12.  Measured, the device
    and the restatement alike (|dx| of the two nulls against the bound, both meshes): n = 16: 4.4e-3, 2.9e-3 <= 6.1e-3; n = 32: 7.4e-4,
    2.7e-5 <= 1.4e-3; n = 64: 3.4e-5, 3.0e-4 <= 3.5e-4."""
    for n in (16, 32, 64):
        check_null_pair(lib_run, MESHES[mname], n)


@pytest.mark.parametrize("mname", list(MESHES))
def test_nulls_none_and_failure_ends(hip, mname):
    mesh = MESHES[mname](SHAPES[mname])
    check_no_nulls(lib_run, mesh)
    check_failure_ends(lib_run, mesh)


@pytest.mark.parametrize("mname", list(MESHES))
def test_nulls_failure_ends_raw_outputs(hip, mname):
    """on the fields where every iteration fails both C entries return 0 (raw_call asserts it), report no null and
    leave nothing that is not finite: the host entry's owned slots are all zero, the device entry's untouched"""
    import ndsm_amd
    mesh = MESHES[mname](SHAPES[mname])
    V = ndsm_amd.VecPot(*mesh)
    try:
        for name, b, ncand in failure_fields(mesh):
            for device, fill, left in ((False, 7, 0), (True, 7, 7)):
                got, arrays = raw_call(hip, V, b, 16, device=device, fill=fill)
                assert got[0][1] == 0 and (ncand is None or got[0][0] == ncand), name
                for a in arrays:
                    assert np.all(np.isfinite(a)) and np.all(a == left), (name, device)
    finally:
        V.close()


@pytest.mark.parametrize("mname", list(MESHES))
def test_nulls_acceptance_tolerance(hip, mname):
    check_near_plane(lib_run, MESHES[mname](SHAPES[mname]))


@pytest.mark.parametrize("mname", list(MESHES))
def test_nulls_second_start(hip, mname):
    check_second_start(lib_run, MESHES[mname](SHAPES[mname]))


@pytest.mark.parametrize("mname", list(MESHES))
def test_nulls_consistent_with_trace(hip, mname):
    """a line started on the spine of a found null and traced towards it ends nearer to it with step 0.25 than with
    step 1"""
    d = spine_approach(lib_run, lib_tracer, MESHES[mname](SHAPES[mname]))
    assert d[1] < d[0]


def test_nulls_argument_errors(hip):
    import ndsm_amd
    mesh = uniform_mesh([9, 8, 7])
    V = ndsm_amd.VecPot(*mesh)
    try:
        L = V.L
        b = np.ascontiguousarray(abc(mesh)).reshape(-1)
        counts = np.full(2, 7, dtype=np.int64)
        out = [np.full(4, 7, dtype=np.int64), np.full(12, 7.0), np.full(36, 7.0), np.full(4, 7.0), np.full(4, 7.0),
               np.full(4, 7, dtype=np.int32), np.full(4, 7, dtype=np.int32)]
        ptr = [a.ctypes.data for a in out]
        assert L.ndsm_hip_vecpot_nulls(V.h, b.ctypes.data, -1, counts.ctypes.data, *ptr) == 9004
        assert np.all(counts == 0) and np.all(out[0] == 7)
        assert L.ndsm_hip_vecpot_nulls(None, b.ctypes.data, 4, counts.ctypes.data, *ptr) == 9002
        assert all(np.all(a == 0) for a in out)
        assert L.ndsm_hip_vecpot_nulls(V.h, None, 4, counts.ctypes.data, *ptr) == 9002
        assert L.ndsm_hip_vecpot_nulls(V.h, b.ctypes.data, 4, None, *ptr) == 9002
        assert L.ndsm_hip_vecpot_nulls(V.h, b.ctypes.data, 4, counts.ctypes.data, *ptr[:6], None) == 9002
        assert L.ndsm_hip_vecpot_nulls_device(V.h, None, 4, counts.ctypes.data, *ptr) == 9002
        # counting needs no record array
        assert L.ndsm_hip_vecpot_nulls(V.h, b.ctypes.data, 0, counts.ctypes.data, *[None] * 7) == 0
        assert counts[0] > 0
        assert ctypes.sizeof(ctypes.c_int) == 4
    finally:
        V.close()
