"""GPU tests of the dips and bald patches (run with -m gpu on an MI355X): VecPot.dips, find_dips, bald_patches,
VecPot.bald_patch_lines and the two C entries.  The yardsticks are the numpy restatement of the semantics in
include/ndsm_hip.h (dips_model.dips_numpy; the counts and every record field bit for bit, through the host and the
device entry and twice in a row) and closed forms (dips_model's checks, which test_dips_model.py runs with the
restatement): flux ropes about an axis along y and along x, a tilted zero surface, a zero surface on a node plane, fields
with NaN, Inf and zero blocks.  Every test runs on golden_inputs.aniso_mesh (unequal spacings, no origin at 0) and on a
uniform mesh, with unequal nx, ny, nz.

The handle takes no mesh with fewer than 4 points on an axis (its 2-D face hierarchies need them;
test_dips_no_handle_under_four_points pins it), so the smallest shapes here are 4 x 4 x 4 and 65 x 4 x 4 - the shapes
with 3 points on an axis cannot be run through the entries -, and the entries' 9004 for a mesh with fewer than 3 nodes
on an axis is out of reach of a caller."""
import ctypes

import numpy as np
import pytest

from device_arena import Arena, LibTransport, slot
from dips_model import (NAMES, bad_value_fields, bald_subset, bitwise_fields, check_bad_values, check_on_node_plane,
                        check_rope, check_tilted, dips_numpy, inside, rope, tilted, white_noise)
from golden_inputs import aniso_mesh, uniform_mesh
from line_model import uniform_b

pytestmark = pytest.mark.gpu

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
SHAPES = {"uniform": [24, 30, 20], "aniso": [33, 22, 27]}
IDS = lambda s: "x".join(map(str, s))   # noqa: E731
FILL = 7


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
        return V.dips(b, **kw)
    finally:
        V.close()


def raw_call(hip, V, b, max_dips, plane_only=0, device=False, fill=0):
    """one call of a C entry on `fill`-initialised arrays of max_dips slots: the tuple of dips_numpy's layout, cut to
    the records written, and the arrays themselves"""
    L = V.L
    B = np.ascontiguousarray(b, dtype=np.float64).reshape(-1).copy()
    m = max(max_dips, 1)
    counts = np.full(3, fill, dtype=np.int64)
    out = [np.full(m, fill, dtype=np.int64), np.full((m, 3), float(fill)), np.full((m, 3), float(fill)),
           np.full((m, 3), float(fill)), np.full(m, float(fill)), np.full(m, fill, dtype=np.int32)]
    if not device:
        rc = L.ndsm_hip_vecpot_dips(V.h, B.ctypes.data, plane_only, max_dips, counts.ctypes.data,
                                    *[a.ctypes.data for a in out])
    else:
        rc = V._on_device([B] + out, lambda dB, *p: L.ndsm_hip_vecpot_dips_device(V.h, dB, plane_only, max_dips,
                                                                                 counts.ctypes.data, *p))
    assert rc == 0, hip.last_error(L)
    n = min(int(counts[1]), max_dips)
    return (counts,) + tuple(a[:n] for a in out), out


def assert_bitwise(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), (what, name)


def cut_to(want, cap):
    return (want[0],) + tuple(a[:cap] for a in want[1:])


def closed_form_fields(mesh):
    """the fields of the closed-form checks, for the bitwise comparison"""
    lo, hi = mesh[2][0], mesh[2][-1]
    nx, nz = len(mesh[0]), len(mesh[2])
    ext = hi - lo
    xc, zc = inside(mesh, 0, 4), inside(mesh, 2, nz // 2, 0.41)
    yield "rope along y", rope(mesh, 1.3, 0.225 * ext, 0.7, xc, zc)
    yield "rope along x", rope(mesh, 1.3, 0.225 * ext, 0.7, inside(mesh, 1, 4), zc, "x")
    yield "rope, curv 0 on a node plane", rope(mesh, 1.3, 0.0, 0.0, xc, mesh[2][nz // 2])
    yield "rope, zero on a node plane", rope(mesh, -1.1, -5.0 * ext, 0.3, mesh[0][nx // 2], lo)
    s = 1.7
    r = 0.6 * s * (mesh[0][-1] - mesh[0][0]) / ext
    yield "tilted", tilted(mesh, 0.8, s, r, inside(mesh, 0, nx // 2, 0.23), inside(mesh, 2, nz // 2, 0.57), 0.9 * r / ext)


def check_all_entries(hip, V, mesh, b, what, want=None, caps=()):
    """counts and records of both entries, twice, against the restatement; the plane_only call of both entries against
    the subset of the full call with flag bit 0; the capacities `caps`, and counting only"""
    want = dips_numpy(mesh, b) if want is None else want
    nd = int(want[0][1])
    got, _arrays = raw_call(hip, V, b, nd + 5)
    assert_bitwise(got, want, what)
    assert np.all(np.diff(got[1]) > 0)
    dev, arrays = raw_call(hip, V, b, nd + 5, device=True, fill=FILL)
    assert_bitwise(dev, want, what + " (device entry)")
    for a in arrays:                                  # slots past the records are not touched
        assert np.all(a[nd:] == FILL)
    again, arrays = raw_call(hip, V, b, nd + 5, fill=FILL)
    assert_bitwise(again, want, what + " (second call)")
    for a in arrays:                                  # the host entry clears its slots past the records
        assert not np.any(a[nd:])
    # plane_only: the records with flag bit 0, bit for bit, and counts[1] == counts[2]
    sub = bald_subset(want)
    nb = int(want[0][2])
    for device in (False, True):
        plane, _arrays = raw_call(hip, V, b, nb + 5, plane_only=1, device=device, fill=FILL)
        assert plane[0][1] == plane[0][2] == nb and 0 <= plane[0][0] <= want[0][0], (what, plane[0])
        assert_bitwise(plane, sub, what + " (plane_only)")
    assert np.array_equal(plane[0], dips_numpy(mesh, b, plane_only=True)[0])
    for cap in caps:
        cut, arrays = raw_call(hip, V, b, cap, fill=FILL)
        assert_bitwise(cut, cut_to(want, cap), "%s (capacity %d)" % (what, cap))
        dcut, arrays = raw_call(hip, V, b, cap, device=True, fill=FILL)
        assert_bitwise(dcut, cut_to(want, cap), "%s (capacity %d, device entry)" % (what, cap))
        for a in arrays:
            assert np.all(a[min(cap, nd):] == FILL)
    for device in (False, True):
        none, arrays = raw_call(hip, V, b, 0, device=device, fill=FILL)
        assert np.array_equal(none[0], want[0])
        for a in arrays:
            assert np.all(a == FILL)
    return want


@pytest.mark.parametrize("mname", list(MESHES))
def test_dips_bitwise_against_the_restatement(hip, mname):
    import ndsm_amd
    mesh = MESHES[mname](SHAPES[mname])
    V = ndsm_amd.VecPot(*mesh)
    try:
        for what, b in list(closed_form_fields(mesh)) + list(bitwise_fields(mesh)):
            want = dips_numpy(mesh, b)
            print(mname, what, "crossings, dips, bald patches", want[0])
            assert want[0][1] >= 2 and want[0][0] >= want[0][1] > want[0][2] > 0
            check_all_entries(hip, V, mesh, b, what, want, caps=(int(want[0][1]) - 1, 1))
    finally:
        V.close()


# white noise U(-1, 1): half of all edges are crossings and about a quarter are dips.  4 x 4 x 4: one mask word per
# family; 65 x 4 x 4: rows of 65 nodes, so that the ballot words straddle rows; 40 x 36 x 44 and 41 x 38 x 35: tens of
# workgroups; 112 x 100 x 96: more than 2^20 nodes and more than 1024 workgroups, so that the scan gives every lane a
# run of several counts
MANY = {"4x4x4": (aniso_mesh, [4, 4, 4]), "65x4x4": (uniform_mesh, [65, 4, 4]), "uniform": (uniform_mesh, [40, 36, 44]),
        "aniso": (aniso_mesh, [41, 38, 35]), "large": (aniso_mesh, [112, 100, 96])}


@pytest.mark.parametrize("mname", list(MANY))
def test_dips_bitwise_white_noise_many_workgroups(hip, mname):
    """counts and records equal the restatement's where the mask and the exclusive sums span many workgroups, with
    capacities that cut inside a later workgroup; then a sparse field on the scratch the call left behind"""
    import ndsm_amd
    meshf, shape = MANY[mname]
    mesh = meshf(shape)
    b = white_noise(shape)
    want = dips_numpy(mesh, b)
    nc, nd, nb = (int(v) for v in want[0])
    nx, ny, nz = shape
    nedges = (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1)
    print(mname, "edges", nedges, "crossings", nc, "dips", nd, "bald patches", nb)
    assert 0.4 * nedges < nc < 0.6 * nedges and 0.15 * nedges < nd < 0.35 * nedges and nb > 0
    if mname == "large":
        assert np.prod(shape) > 2 ** 20 and np.prod(shape) > 1024 * 1024
    V = ndsm_amd.VecPot(*mesh)
    try:
        check_all_entries(hip, V, mesh, b, mname, want, caps=(nd // 2 + 3, 257, 1))
        # a field with few dips afterwards, on the scratch the large call left behind
        lo, hi = mesh[2][0], mesh[2][-1]
        sparse = rope(mesh, 1.3, 0.225 * (hi - lo), 0.7, inside(mesh, 0, 1), inside(mesh, 2, nz // 2, 0.41))
        got, _arrays = raw_call(hip, V, sparse, 4096)
        assert_bitwise(got, dips_numpy(mesh, sparse, max_dips=4096), mname + " (sparse after dense)")
        assert 0 < got[0][1] < nd
        none, _arrays = raw_call(hip, V, uniform_b(mesh), 16, fill=FILL)
        assert np.all(none[0] == 0)
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------
# caller arrays at an offset base, guard bands on both sides (device_arena)
# ---------------------------------------------------------------------------------------------------------------
# N = 64: one mask word per family; 125, 315: odd, the components start at 8 and 0 mod 16 in turn; 1340: a second
# workgroup
ARENA_SHAPES = ([4, 4, 4], [5, 5, 5], [7, 5, 9], [67, 5, 4])


def dip_slots(b, cap):
    return [slot("B", np.ascontiguousarray(b, dtype=np.float64).reshape(-1), field=True),
            slot("edge", np.full(cap, FILL, dtype=np.int64), output=True),
            slot("pos", np.full((cap, 3), float(FILL)), output=True),
            slot("bpt", np.full((cap, 3), float(FILL)), output=True),
            slot("grad", np.full((cap, 3), float(FILL)), output=True),
            slot("curv", np.full(cap, float(FILL)), output=True),
            slot("flag", np.full(cap, FILL, dtype=np.int32), output=True)]


def dips_device(hip, V, b, cap, plane_only=0, plain=False):
    """one call of ndsm_hip_vecpot_dips_device with capacity cap on arrays of exactly cap slots in an arena; the slots
    past the records must come back as they went up (the arena checks it); with cap = 0 every record pointer is NULL"""
    counts = np.full(3, FILL, dtype=np.int64)
    slots = dip_slots(b, cap) if cap > 0 else dip_slots(b, 1)[:1]

    def call(dB, *rec):
        return V.L.ndsm_hip_vecpot_dips_device(V.h, dB, plane_only, cap, counts.ctypes.data,
                                               *(rec if cap > 0 else [None] * 6))

    def written():
        n = min(max(int(counts[1]), 0), cap)
        return {s.name: n for s in slots[1:]}
    A = Arena(LibTransport(V.L), slots, plain=plain)
    out = A.run(call, written=written)
    assert A.rc == 0, hip.last_error(V.L)
    n = min(int(counts[1]), cap)
    if cap == 0:
        return (counts,)
    return (counts,) + tuple(a[:n] for a in out[1:])


@pytest.mark.parametrize("ns", ARENA_SHAPES, ids=IDS)
@pytest.mark.parametrize("mname", list(MESHES))
def test_dips_on_offset_arrays(hip, mname, ns):
    import ndsm_amd
    mesh = MESHES[mname](ns)
    b = white_noise(ns, seed=5)
    want = dips_numpy(mesh, b)
    nd, nb = int(want[0][1]), int(want[0][2])
    print(mname, ns, "counts", want[0])
    assert nd >= 4 and nb >= 2
    sub = bald_subset(want)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for cap in (nd + 3, nd, nd - 1, 1):
            got = dips_device(hip, V, b, cap)
            assert_bitwise(got, cut_to(want, cap), "%s %s capacity %d" % (mname, ns, cap))
            assert len(got[1]) == min(nd, cap) and np.all(np.diff(got[1]) > 0)
        assert np.array_equal(dips_device(hip, V, b, 0)[0], want[0])
        for cap in (nb + 3, nb - 1):
            plane = dips_device(hip, V, b, cap, plane_only=1)
            assert plane[0][1] == plane[0][2] == nb
            assert_bitwise(plane, (None,) + tuple(a[:cap] for a in sub[1:]), "%s %s plane_only %d" % (mname, ns, cap))
        assert_bitwise(dips_device(hip, V, b, nd + 3, plain=True), want, "%s %s plain" % (mname, ns))
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------
# closed forms with the library
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", list(MESHES))
@pytest.mark.parametrize("along", ["y", "x"])
def test_dips_rope(hip, mname, along):
    check_rope(lib_run, MESHES[mname](SHAPES[mname]), along)


@pytest.mark.parametrize("mname", list(MESHES))
def test_dips_tilted_zero_surface(hip, mname):
    check_tilted(lib_run, MESHES[mname](SHAPES[mname]))


@pytest.mark.parametrize("mname", list(MESHES))
def test_dips_zero_on_a_node_plane(hip, mname):
    check_on_node_plane(lib_run, MESHES[mname](SHAPES[mname]))


@pytest.mark.parametrize("mname", list(MESHES))
def test_dips_bad_values(hip, mname):
    """no dip on the fields with NaN, Inf and zero blocks over the zero surface; both C entries return 0, and leave
    nothing that is not finite: the host entry's owned slots are all zero, the device entry's untouched"""
    import ndsm_amd
    mesh = MESHES[mname](SHAPES[mname])
    check_bad_values(lib_run, mesh)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for name, b, _ncross in bad_value_fields(mesh):
            want = dips_numpy(mesh, b)
            for plane_only in (0, 1):
                for device, left in ((False, 0), (True, FILL)):
                    got, arrays = raw_call(hip, V, b, 16, plane_only=plane_only, device=device, fill=FILL)
                    assert got[0][1] == 0 and got[0][2] == 0, name
                    assert plane_only or np.array_equal(got[0], want[0]), (name, got[0], want[0])
                    for a in arrays:
                        assert np.all(np.isfinite(a)) and np.all(a == left), (name, device)
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------
# errors and the Python layer
# ---------------------------------------------------------------------------------------------------------------
def test_dips_argument_errors(hip):
    import ndsm_amd
    mesh = uniform_mesh([9, 8, 7])
    V = ndsm_amd.VecPot(*mesh)
    try:
        L = V.L
        b = np.ascontiguousarray(white_noise([9, 8, 7])).reshape(-1)

        def fresh():
            counts = np.full(3, FILL, dtype=np.int64)
            out = [np.full(4, FILL, dtype=np.int64), np.full(12, 7.0), np.full(12, 7.0), np.full(12, 7.0),
                   np.full(4, 7.0), np.full(4, FILL, dtype=np.int32)]
            return counts, out, [a.ctypes.data for a in out]
        for entry in (L.ndsm_hip_vecpot_dips, L.ndsm_hip_vecpot_dips_device):
            host = entry is L.ndsm_hip_vecpot_dips
            # 9004: max_dips < 0, plane_only not 0 or 1 (nothing is staged, no record array is touched)
            for plane_only, cap in ((0, -1), (1, -5), (2, 4), (-1, 4), (2, 0)):
                counts, out, ptr = fresh()
                assert entry(V.h, b.ctypes.data, plane_only, cap, counts.ctypes.data, *ptr) == 9004, (plane_only, cap)
                assert np.all(counts == 0)
                assert all(np.all(a == (0 if host and cap > 0 else FILL)) for a in out)
            # 9002: a NULL handle, B, counts, or with max_dips > 0 a record array
            counts, out, ptr = fresh()
            assert entry(None, b.ctypes.data, 0, 4, counts.ctypes.data, *ptr) == 9002
            assert np.all(counts == 0) and all(np.all(a == (0 if host else FILL)) for a in out)
            counts, out, ptr = fresh()
            assert entry(V.h, None, 0, 4, counts.ctypes.data, *ptr) == 9002
            assert np.all(counts == 0)
            assert entry(V.h, b.ctypes.data, 0, 4, None, *ptr) == 9002
            for miss in range(6):
                counts, out, ptr = fresh()
                ptr[miss] = None
                assert entry(V.h, b.ctypes.data, 1, 4, counts.ctypes.data, *ptr) == 9002, miss
                assert np.all(counts == 0)
        # counting needs no record array
        counts = np.full(3, FILL, dtype=np.int64)
        assert L.ndsm_hip_vecpot_dips(V.h, b.ctypes.data, 0, 0, counts.ctypes.data, *[None] * 6) == 0
        assert counts[0] > counts[1] > counts[2] > 0
        assert ctypes.sizeof(ctypes.c_int) == 4
    finally:
        V.close()


def test_dips_no_handle_under_four_points(hip):
    """what keeps 3 x 3 x 3 and the 9004 of a mesh with fewer than 3 nodes on an axis out of reach: the handle's 2-D face
    hierarchies need 4 points on every axis"""
    import ndsm_amd
    for ns in ([3, 3, 3], [65, 3, 4], [4, 4, 3]):
        with pytest.raises(ndsm_amd.NdsmHipError):
            ndsm_amd.VecPot(*uniform_mesh(ns))
        with pytest.raises(ndsm_amd.NdsmHipError):
            ndsm_amd.find_dips(*uniform_mesh(ns), np.zeros((3, ns[2], ns[1], ns[0])))


def test_dips_python_layer(hip):
    """VecPot.dips against the raw entry; the counting call and the retry when a capacity was too small; the one-shot
    forms"""
    import ndsm_amd
    mesh = aniso_mesh(SHAPES["aniso"])
    b = next(iter(bitwise_fields(mesh)))[1]
    want = dips_numpy(mesh, b)
    nd = int(want[0][1])
    V = ndsm_amd.VecPot(*mesh)
    try:
        raw, _arrays = raw_call(hip, V, b, nd)
        assert_bitwise(raw, want, "raw")
        for kw in ({}, dict(max_dips=1), dict(max_dips=nd), dict(max_dips=nd + 100), dict(device=True),
                   dict(device=True, max_dips=3)):
            got = V.dips(b, **kw)
            assert (got.ncrossings, got.ndips, got.nbald) == tuple(int(v) for v in raw[0]), kw
            assert len(got.edge) == nd
            for g, w in zip((got.edge, got.position, got.b, got.grad, got.curv), raw[1:6]):
                assert np.array_equal(g, w), kw
            assert np.array_equal(got.bald, raw[6] == 1) and np.array_equal(got.axis, raw[1] % 3)
            assert np.array_equal(got.kappa, raw[5] / (raw[3][:, 0] * raw[3][:, 0] + raw[3][:, 1] * raw[3][:, 1]))
            nx, ny = len(mesh[0]), len(mesh[1])
            assert np.array_equal(got.node[:, 0] + nx * (got.node[:, 1] + ny * got.node[:, 2]), raw[1] // 3)
        count = V.dips(b, max_dips=0)
        assert (count.ncrossings, count.ndips, count.nbald, len(count.edge)) == (raw[0][0], nd, raw[0][2], 0)
        plane = V.dips(b, plane_only=True)
        assert plane.ndips == plane.nbald == raw[0][2] == len(plane.edge) and np.all(plane.bald)
        assert np.array_equal(plane.position, got.position[got.bald])
        one = ndsm_amd.find_dips(*mesh, b)
        assert np.array_equal(one.position, got.position) and np.array_equal(one.curv, got.curv)
        bald = ndsm_amd.bald_patches(*mesh, b)
        assert np.array_equal(bald.position, plane.position) and np.array_equal(bald.edge, plane.edge)
    finally:
        V.close()


@pytest.mark.parametrize("mname", list(MESHES))
def test_bald_patch_lines(hip, mname):
    """bald_patch_lines is, bit for bit, VecPot.paths on the seeds position + (0, 0, lift h_z) of the records with
    bald, traced in both directions; on the rope about y every stored point stays at or above the lower face"""
    import ndsm_amd
    mesh = MESHES[mname](SHAPES[mname])
    lo, hi = mesh[2][0], mesh[2][-1]
    b = rope(mesh, 1.3, 0.225 * (hi - lo), 0.7, inside(mesh, 0, len(mesh[0]) // 2), inside(mesh, 2, len(mesh[2]) // 2, 0.41))
    V = ndsm_amd.VecPot(*mesh)
    try:
        dips = V.dips(b)
        assert dips.nbald == len(mesh[1]) and dips.ndips > dips.nbald
        for lift, kw in ((1e-3, {}), (0.25, dict(step=0.3, every=3, values=False))):
            got = V.bald_patch_lines(b, dips, lift=lift, **kw)
            seeds = dips.position[dips.bald] + np.array([0.0, 0.0, lift * (mesh[2][1] - mesh[2][0])])
            want = V.paths(b, seeds, direction="both", **kw)
            assert len(got.offsets) == 2 * dips.nbald + 1 and got.offsets[-1] == len(got.points) > 2 * dips.nbald
            assert np.array_equal(got.offsets, want.offsets) and np.array_equal(got.points, want.points)
            assert np.array_equal(got.lines.ends, want.lines.ends) and np.array_equal(got.lines.status, want.lines.status)
            assert (got.b is None) == (want.b is None) and (got.b is None or np.array_equal(got.b, want.b))
            assert np.all(got.points[:, 2] >= lo)
        plane = V.dips(b, plane_only=True)
        again = V.bald_patch_lines(b, plane)
        first = V.bald_patch_lines(b, dips)
        assert np.array_equal(again.points, first.points)
        # no bald patch: no line
        none = V.bald_patch_lines(b, V.dips(uniform_b(mesh)))
        assert len(none.offsets) == 1 and none.points.shape == (0, 3)
    finally:
        V.close()


def test_dips_of_a_linear_force_free_field(hip):
    """the intended chain: find_dips on a linear_force_free_field box runs and returns finite records - the model's
    bits, no value asserted beyond them"""
    import ndsm_amd
    n = [24, 20, 12]
    x, y = np.linspace(-1.0, 1.0, n[0]), np.linspace(-0.8, 0.8, n[1])
    z = np.arange(n[2]) * (x[1] - x[0])
    X, Y = np.meshgrid(x, y)
    bz = np.exp(-((X - 0.35) ** 2 + Y ** 2) / 0.05) - np.exp(-((X + 0.35) ** 2 + (Y - 0.1) ** 2) / 0.05)
    b = ndsm_amd.linear_force_free_field(x, y, z, bz, 1.5)
    got = ndsm_amd.find_dips(x, y, z, b)
    want = dips_numpy([x, y, z], b)
    print("lfff box: crossings, dips, bald patches", want[0])
    assert (got.ncrossings, got.ndips, got.nbald) == tuple(int(v) for v in want[0]) and got.ncrossings > 0
    for g, w in zip((got.edge, got.position, got.b, got.grad, got.curv), want[1:6]):
        assert np.array_equal(g, w) and np.all(np.isfinite(g))
    assert np.array_equal(got.bald, want[6] == 1)
