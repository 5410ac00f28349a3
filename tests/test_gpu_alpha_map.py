"""GPU tests of the alpha map (run with -m gpu on an MI355X): VecPot.alpha_map, map_alpha and the two C entries.  The
yardsticks are the numpy restatement of the semantics in include/ndsm_hip.h (alpha_model.alpha_map_numpy on top of
line_model.trace_numpy; bit for bit) and the public trace on the node seeds (no model involved).  Every mesh-dependent
test runs on golden_inputs.aniso_mesh (unequal spacings, no origin at 0) as well as on a uniform mesh."""
import numpy as np
import pytest

from alpha_model import ZLO, alpha_map_numpy, alpha_of_ends, node_seeds
from device_arena import Arena, LibTransport, slot
from golden_inputs import aniso_mesh, uniform_mesh
from line_model import NULL, UNFINISHED, abc, grids, helical, sheared, uniform_b

pytestmark = pytest.mark.gpu

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
# ndsm_hip_vecpot_create takes no mesh under four points per axis, so no public entry reaches 2x2x2 or
# 5x7x3 (105 lanes), which the numpy restatement itself is tested on (test_alpha_model.py).  The smallest meshes a handle
# exists for, with the same edges: (4,4,4): 64 lanes, exactly one wave; (5,5,4): 100 lanes, a partial second wave;
# (5,7,4): the unequal nx, ny of 5x7x3, 140 lanes; (33,22,27): 307 waves
SHAPES = [(4, 4, 4), (5, 5, 4), (5, 7, 4), (33, 22, 27)]
MAX_STEPS = 100          # enough for most lines of the largest box at step 0.5; the rest end UNFINISHED, bit for bit too


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


_HANDLES = {}


def handle(kind, shape):
    """one VecPot per mesh for the module"""
    import ndsm_amd
    key = (kind, tuple(shape))
    if key not in _HANDLES:
        mesh = MESHES[kind](shape)
        _HANDLES[key] = (mesh, ndsm_amd.VecPot(*mesh))
    return _HANDLES[key]


def abc_hole(mesh):
    """the ABC field with a block of zeros (where there is room for one): lines that run into it end NULL"""
    b = abc(mesh)
    nz, ny, nx = b.shape[1:]
    if min(nx, ny, nz) >= 5:
        b[:, nz // 2 - 1:nz // 2 + 2, ny // 2 - 1:ny // 2 + 2, nx // 2 - 1:nx // 2 + 2] = 0.0
    return b


FIELDS = {
    "uniform_b": (lambda mesh: uniform_b(mesh), MAX_STEPS),
    "helical": (lambda mesh: helical(mesh)[0], MAX_STEPS),
    "sheared": (lambda mesh: sheared(mesh), MAX_STEPS),
    "abc": (abc_hole, MAX_STEPS),
    "helical_short": (lambda mesh: helical(mesh)[0], 7),          # UNFINISHED ends
}


def alpha0_of(mesh, seed=2131):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, (len(mesh[1]), len(mesh[0])))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the numpy restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [0.5, 0.25])
@pytest.mark.parametrize("polarity", [1, -1])
@pytest.mark.parametrize("field", sorted(FIELDS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", sorted(MESHES))
def test_matches_the_numpy_restatement_bitwise(hip, kind, shape, field, polarity, step):
    """alpha as uint64 and the status equal the model's: fp64 +, -, *, / and sqrt are correctly rounded on both sides
    and the device code is built without contraction"""
    mesh, V = handle(kind, shape)
    make, max_steps = FIELDS[field]
    b = make(mesh)
    alpha0 = alpha0_of(mesh)
    got, gst = V.alpha_map(b, alpha0, polarity=polarity, step=step, max_steps=max_steps)
    want, wst = alpha_map_numpy(mesh, b, alpha0, polarity, step, max_steps)
    assert got.shape == want.shape == tuple(shape[::-1]) and gst.dtype == np.int32
    print(kind, shape, field, polarity, step, "status differs:", int((gst != wst).sum()),
          "max |alpha - model|:", np.abs(got - want).max(), "statuses:", sorted(set(wst.reshape(-1).tolist())))
    assert np.array_equal(gst, wst)
    assert np.array_equal(bits(got), bits(want))
    seen = set(wst.reshape(-1).tolist())
    if field in ("uniform_b", "helical", "sheared") and polarity == 1:
        assert ZLO in seen                                 # B_z > 0: against B the lines come down to the lower face
        assert np.any(got != 0.0)
    if field == "helical_short" and max(shape) > 8:
        assert UNFINISHED in seen
    if field == "abc" and min(shape) >= 5:
        assert NULL in seen


# ---------------------------------------------------------------------------------------------------------------------
# 2. the public trace on the node seeds: no model involved
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("polarity", [1, -1])
@pytest.mark.parametrize("field", ["sheared", "abc"])
@pytest.mark.parametrize("kind", sorted(MESHES))
def test_matches_the_public_trace(hip, kind, field, polarity):
    """the status of every node is trace()'s for the node as the seed with direction -polarity, and alpha is the numpy
    bilinear interpolant of trace()'s end points, bit for bit"""
    mesh, V = handle(kind, (17, 12, 9))
    b = FIELDS[field][0](mesh)
    alpha0 = alpha0_of(mesh, 2132)
    alpha, status = V.alpha_map(b, alpha0, polarity=polarity, step=0.5, max_steps=MAX_STEPS)
    fl = V.trace(b, node_seeds(mesh), step=0.5, max_steps=MAX_STEPS,
                 direction="backward" if polarity == 1 else "forward")
    assert np.array_equal(status.reshape(-1), fl.status[0])
    want = alpha_of_ends(mesh, alpha0, fl.ends[0], fl.status[0])
    assert np.array_equal(bits(alpha.reshape(-1)), bits(want))
    if polarity == 1 or field == "abc":                    # (sheared has B_z > 0: along B no line comes back down)
        assert (status == ZLO).any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. host entry against device entry, caller arrays inside a larger allocation, status = NULL
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", [("aniso", (5, 5, 4)), ("uniform", (17, 12, 9))])
def test_host_and_device_entries_agree(hip, kind, shape):
    """the device entry on views into one larger allocation at an offset base (8-byte data at 8 mod 16, 4-byte data at
    4 mod 8), NaN bands beside the inputs and canaries beside the outputs intact, gives the host entry's bits; so does
    device=True of the Python layer, and status = NULL leaves alpha as it is"""
    mesh, V = handle(kind, shape)
    L = V.L
    b = sheared(mesh)
    alpha0 = alpha0_of(mesh, 2133)
    n = int(np.prod(shape))
    host_a, host_s = V.alpha_map(b, alpha0, step=0.5, max_steps=MAX_STEPS)
    dev_a, dev_s = V.alpha_map(b, alpha0, step=0.5, max_steps=MAX_STEPS, device=True)
    assert np.array_equal(bits(host_a), bits(dev_a)) and np.array_equal(host_s, dev_s)
    arena = Arena(LibTransport(L), [slot("B", b, field=True), slot("alpha0", alpha0, field=True),
                                    slot("alpha", np.full(n, 7.0), output=True),
                                    slot("status", np.full(n, 77, dtype=np.int32), output=True)])
    _b, _a0, alpha, status = arena.run(
        lambda dB, da0, dal, dst: L.ndsm_hip_vecpot_alpha_map_device(V.h, dB, da0, 1, 0.5, MAX_STEPS, dal, dst))
    assert arena.rc == 0
    assert np.array_equal(bits(alpha), bits(host_a.reshape(-1))) and np.array_equal(status, host_s.reshape(-1))
    # without the status
    arena = Arena(LibTransport(L), [slot("B", b, field=True), slot("alpha0", alpha0, field=True),
                                    slot("alpha", np.full(n, 7.0), output=True)])
    _b, _a0, alpha = arena.run(
        lambda dB, da0, dal: L.ndsm_hip_vecpot_alpha_map_device(V.h, dB, da0, 1, 0.5, MAX_STEPS, dal, None))
    assert arena.rc == 0 and np.array_equal(bits(alpha), bits(host_a.reshape(-1)))
    B = np.ascontiguousarray(b).reshape(-1).copy()
    a0 = np.ascontiguousarray(alpha0).reshape(-1).copy()
    alpha = np.full(n, 7.0)
    rc = L.ndsm_hip_vecpot_alpha_map(V.h, B.ctypes.data, a0.ctypes.data, 1, 0.5, MAX_STEPS, alpha.ctypes.data, None)
    assert rc == 0 and np.array_equal(bits(alpha), bits(host_a.reshape(-1)))


def test_one_shot_form_and_repeat(hip):
    """map_alpha on a handle of its own gives VecPot.alpha_map's bits, and two calls give the same bits: a node
    depends on its own line only, not on the launch"""
    import ndsm_amd
    mesh, V = handle("aniso", (17, 12, 9))
    b = abc_hole(mesh)
    alpha0 = alpha0_of(mesh, 2134)
    a1, s1 = V.alpha_map(b, alpha0, polarity=-1, step=0.25, max_steps=MAX_STEPS)
    a2, s2 = V.alpha_map(b, alpha0, polarity=-1, step=0.25, max_steps=MAX_STEPS)
    a3, s3 = ndsm_amd.map_alpha(*mesh, b, alpha0, polarity=-1, step=0.25, max_steps=MAX_STEPS)
    for a, s in ((a2, s2), (a3, s3)):
        assert np.array_equal(bits(a1), bits(a)) and np.array_equal(s1, s)


@pytest.mark.parametrize("kind", sorted(MESHES))
def test_sub_box_of_a_linear_field(hip, kind):
    """A node takes nothing from its neighbours: the map of a sub-box shifted by whole cells - its own handle, its own
    launch, other lanes beside each node - equals the full map at the shared nodes.  The field is linear in x, y, z
    in physical coordinates (the trilinear interpolant reproduces it in either box), B_z = 0.9 > 0, and the sub-box
    shares the lower face, so a line that ends ZLO in the sub-box is the full box's line, step for step.  Compared
    where both end ZLO.  Not bit for bit: the seed lo' + i h of the sub-box and lo + (i + o) h of the full box differ by
    rounding, which the linear field (rates <= 0.4 over <= 1.3 box lengths: a factor e^0.5) carries to the foot and
    the bilinear rule multiplies by |grad alpha0| h <= 4 per cell: ~60 steps of a few eps of the coordinates each,
    times 4 / h = 64, stay below 1e-12; the bound is 1e-10 max |alpha0|, and a lane that read a neighbour's line
    would be off by O(|alpha0|)."""
    import ndsm_amd
    shape, off, sub = (17, 12, 9), (3, 2, 0), (9, 7, 9)
    mesh, V = handle(kind, shape)
    x0, y0, z0 = mesh[0][0], mesh[1][0], mesh[2][0]

    def field(m):
        X, Y, Z = grids(m)
        return np.stack([0.3 + 0.4 * (X - x0) + 0.2 * (Z - z0), -0.2 - 0.4 * (Y - y0) + 0.1 * (Z - z0),
                         np.full(X.shape, 0.9)])
    alpha0 = alpha0_of(mesh, 2135)
    full_a, full_s = V.alpha_map(field(mesh), alpha0, step=0.5, max_steps=MAX_STEPS)
    smesh = [q[o:o + m].copy() for q, o, m in zip(mesh, off, sub)]
    window = (slice(off[2], off[2] + sub[2]), slice(off[1], off[1] + sub[1]), slice(off[0], off[0] + sub[0]))
    W = ndsm_amd.VecPot(*smesh)
    try:
        sub_a, sub_s = W.alpha_map(field(smesh), np.ascontiguousarray(alpha0[window[1:]]), step=0.5,
                                   max_steps=MAX_STEPS)
    finally:
        W.close()
    both = (sub_s == ZLO) & (full_s[window] == ZLO)
    gap = np.abs(sub_a - full_a[window])[both].max()
    print(kind, "nodes compared:", int(both.sum()), "of", both.size, "max gap:", gap)
    assert both.sum() >= 50
    assert np.all(full_s[window][sub_s == ZLO] == ZLO)        # a line that stays in the sub-box stays in the box
    assert gap <= 1e-10 * np.abs(alpha0).max()


# ---------------------------------------------------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_scalars_and_null_arrays(hip):
    """a scalar out of range is 9004 and a NULL handle or required array 9002, from both entries; the host entry
    clears its outputs, nothing is launched"""
    mesh, V = handle("uniform", (5, 5, 4))
    L = V.L
    n = 5 * 5 * 4
    B = np.ascontiguousarray(sheared(mesh)).reshape(-1).copy()
    a0 = np.ascontiguousarray(alpha0_of(mesh)).reshape(-1).copy()

    def call(entry, h, pb, pa0, pol, step, ms, with_alpha=True):
        alpha, status = np.full(n, 7.0), np.full(n, 77, dtype=np.int32)
        rc = entry(h, pb, pa0, pol, step, ms, alpha.ctypes.data if with_alpha else None, status.ctypes.data)
        return rc, alpha, status

    pb, pa0 = B.ctypes.data, a0.ctypes.data
    for pol, step, ms in ((0, 0.5, 10), (2, 0.5, 10), (-3, 0.5, 10), (1, 0.0, 10), (1, -0.5, 10),
                          (1, float("nan"), 10), (1, float("inf"), 10), (1, 0.5, 0), (-1, 0.5, -4)):
        rc, alpha, status = call(L.ndsm_hip_vecpot_alpha_map, V.h, pb, pa0, pol, step, ms)
        assert rc == 9004, (pol, step, ms, rc)
        assert np.all(alpha == 0.0) and np.all(status == 0)
        # (the device entry is refused before any pointer is looked at: host addresses do no harm here)
        rc, alpha, status = call(L.ndsm_hip_vecpot_alpha_map_device, V.h, pb, pa0, pol, step, ms)
        assert rc == 9004, (pol, step, ms, rc)
        assert np.all(alpha == 7.0) and np.all(status == 77)
    for entry in (L.ndsm_hip_vecpot_alpha_map, L.ndsm_hip_vecpot_alpha_map_device):
        assert call(entry, None, pb, pa0, 1, 0.5, 10)[0] == 9002
        assert call(entry, V.h, None, pa0, 1, 0.5, 10)[0] == 9002
        assert call(entry, V.h, pb, None, 1, 0.5, 10)[0] == 9002
        assert call(entry, V.h, pb, pa0, 1, 0.5, 10, with_alpha=False)[0] == 9002
    rc, alpha, status = call(L.ndsm_hip_vecpot_alpha_map, V.h, None, pa0, 1, 0.5, 10)
    assert np.all(alpha == 0.0) and np.all(status == 0)
    # the Python layer raises with the code
    with pytest.raises(hip.NdsmHipError, match="9004"):
        V.alpha_map(sheared(mesh), alpha0_of(mesh), polarity=0)
