"""Every form of the inter-level transfers against the oracle port, bit for bit, at small shapes.

Which kernel restricts a residual or interpolates a correction is decided by the size of the fine level: the gather
kernel restrict_k or the LDS-streamed restrict_stream_k (three forms: 5 table walk, 8 scheduled, 10 DMA), the per-point
prolong_add_k or the LDS-tiled prolong_tile_k.  Left alone, the large-level forms run from 6 Mi and 2 Mi points on,
where the oracle is slow and where a shape hits the kernels' edges - a tile of 64 x 8 coarse columns, z chunks of at
most 64 coarse planes, odd nx - only by accident.  ndsm_hip_debug_transfer_cfg moves the sizes and picks form and chunk
length at run time, ndsm_hip_debug_transfer_form reports what the launchers will do from the very functions they ask,
and every test here first asserts from that report that the form it names is the one that runs.

The yardstick is port.restrict / port.interp (pinned to the reference by test_oracle.py); every comparison is
np.array_equal - there is no tolerance in this file.  Fields come from rand_field; each shape runs on uniform_mesh and
on aniso_mesh.  The fp32 instantiation of prolong_tile_k and the fp32 fine side of the streamed restriction stay with
the mixed-precision tests (test_gpu_mixed.py, test_gpu_bc_matrix.py::test_mixed_precision_cycle): their yardstick is
the fp32 model, not the port.

The tests that count forms (test_every_form_ran) look at what the parametrised cases before them recorded: run the
module as a whole.
"""
import collections
import itertools

import numpy as np
import pytest

from golden_inputs import aniso_mesh, rand_field, uniform_mesh

gpu = pytest.mark.gpu
MESHES = (uniform_mesh, aniso_mesh)
BCS = "NDDNDD"
NEVER = 1 << 40          # a level size no grid reaches: the large-level form is off

# ---------------------------------------------------------------------------------------------------------------------
# the cases (checked without a GPU below)
# ---------------------------------------------------------------------------------------------------------------------
# restriction: classes of the fine n per axis, by what the coarse n = n // 2 is to the streamed kernel's tile of 64 x 8
# coarse columns and to its chunks of at most 64 coarse planes
RESTRICT_X = (40, 128, 129, 130, 131)     # nc = 20 under a tile, 64 one tile, 64 odd nx, 65 a tile + 1, 65 odd nx
RESTRICT_Y = (8, 16, 17, 18, 34)          # nc = 4, 8, 8, 9, 17
RESTRICT_Z = (8, 16, 129, 130, 131)       # c_cnt = 4, 8, 64, 65, 65
# a three-factor, five-level orthogonal array (row (i, j) takes z class (i + j + 1) mod 5): every pair of classes once
RESTRICT_ROWS = (
    (40, 8, 16), (40, 16, 129), (40, 17, 130), (40, 18, 131), (40, 34, 8),
    (128, 8, 129), (128, 16, 130), (128, 17, 131), (128, 18, 8), (128, 34, 16),
    (129, 8, 130), (129, 16, 131), (129, 17, 8), (129, 18, 16), (129, 34, 129),
    (130, 8, 131), (130, 16, 8), (130, 17, 16), (130, 18, 129), (130, 34, 130),
    (131, 8, 8), (131, 16, 16), (131, 17, 129), (131, 18, 130), (131, 34, 131),
)
CHUNK_SHAPES = ((130, 18, 129), (130, 18, 130), (131, 17, 131))
CHUNKS = (-1, 1, 4, 64)
# pairs 9 -> 4 and 11 -> 5 on each axis in turn: the only ones with six taps, more than the streamed kernel holds
SIX_TAP_SHAPES = ((9, 16, 16), (11, 16, 16), (16, 9, 16), (16, 11, 16), (16, 16, 9), (16, 16, 11), (22, 18, 9))
FIVE_TAP_SHAPES = ((10, 16, 16), (16, 12, 16), (16, 16, 13))      # their neighbours: streamed

# prolongation: the tiled kernel's fine tile is 64 x 8 x 8 points; it needs nx >= 64 and 16 coarse points per axis
PROLONG_X = (64, 65, 127, 128, 129)       # one tile, a tile + 1, two tiles - 1, two tiles, two tiles + 1
PROLONG_Y = (32, 33, 39, 40)              # whole tiles (nc = 16, the least), + 1, - 1, whole
PROLONG_Z = (32, 33, 39, 41)
# row (i, j) takes z class (i + j) mod 4: every pair of classes at least once in 20 rows
PROLONG_ROWS = (
    (64, 32, 32), (64, 33, 33), (64, 39, 39), (64, 40, 41),
    (65, 32, 33), (65, 33, 39), (65, 39, 41), (65, 40, 32),
    (127, 32, 39), (127, 33, 41), (127, 39, 32), (127, 40, 33),
    (128, 32, 41), (128, 33, 32), (128, 39, 33), (128, 40, 39),
    (129, 32, 32), (129, 33, 33), (129, 39, 39), (129, 40, 41),
)
PROLONG_OUTSIDE = ((63, 32, 32), (64, 31, 32), (64, 32, 31))      # nx = 63, nc[1] = 15, nc[2] = 15: per point

# three slabs of 22 planes; ny = 18 has 9 coarse rows, under the tiled prolongation's 16: the second shape has 17
SLAB_SHAPES = ((130, 18, 66), (130, 34, 66))

# shapes per form that must have run when the module is through
EXPECTED = {"gather": 25, "rs5": 25, "rs8": 25, "rs10": 15, "rs10->8": 10, "tiled": 20, "per-point": 20}
RAN = collections.Counter()


def _tag(ns):
    return "x".join(str(n) for n in ns)


def _covers_every_pair(rows, axes):
    for i, j in itertools.combinations(range(len(axes)), 2):
        if {(r[i], r[j]) for r in rows} != set(itertools.product(axes[i], axes[j])):
            return False
    return all(r[d] in axes[d] for r in rows for d in range(len(axes)))


def test_restriction_rows_cover_every_pair_of_classes():
    axes = (RESTRICT_X, RESTRICT_Y, RESTRICT_Z)
    assert len(RESTRICT_ROWS) == 25 == len(set(RESTRICT_ROWS))
    assert _covers_every_pair(RESTRICT_ROWS, axes)
    for i, j in itertools.combinations(range(3), 2):          # an orthogonal array: every pair exactly once
        assert len({(r[i], r[j]) for r in RESTRICT_ROWS}) == 25
    # the classes are what the comments say they are to the kernel (coarse n = n // 2: floor(n / 2) points)
    assert [n // 2 for n in RESTRICT_X] == [20, 64, 64, 65, 65] and [n & 1 for n in RESTRICT_X] == [0, 0, 1, 0, 1]
    assert [n // 2 for n in RESTRICT_Y] == [4, 8, 8, 9, 17]
    assert [n // 2 for n in RESTRICT_Z] == [4, 8, 64, 65, 65]
    assert max(r[0] * r[1] * r[2] for r in RESTRICT_ROWS) == 131 * 34 * 131
    assert sum(1 for r in RESTRICT_ROWS if r[0] % 2 == 0) == EXPECTED["rs10"]
    assert sum(1 for r in RESTRICT_ROWS if r[0] % 2 == 1) == EXPECTED["rs10->8"]
    assert sorted(ns[2] // 2 for ns in CHUNK_SHAPES) == [64, 65, 65] and [ns[0] & 1 for ns in CHUNK_SHAPES] == [0, 0, 1]


def test_prolongation_rows_cover_every_pair_of_classes():
    assert len(PROLONG_ROWS) <= 20 and len(set(PROLONG_ROWS)) == len(PROLONG_ROWS)
    assert _covers_every_pair(PROLONG_ROWS, (PROLONG_X, PROLONG_Y, PROLONG_Z))
    assert all(r[0] >= 64 and min(n // 2 for n in r) >= 16 for r in PROLONG_ROWS)
    assert [(ns[0] >= 64, ns[1] // 2 >= 16, ns[2] // 2 >= 16) for ns in PROLONG_OUTSIDE] == [
        (False, True, True), (True, False, True), (True, True, False)]


# ---------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    yield _lib
    _lib.transfer_cfg()


def _shp(ns):
    return tuple(int(v) for v in ns[::-1])


def _pad_r(solver, arr):
    """place a level-l array at the start of the level-1 sized residual scratch"""
    full = np.zeros(solver._npshape(1))
    full.ravel()[:arr.size] = arr.ravel()
    return full


def _restricted(hip, S, f, lvl=1):
    """rhs(lvl + 1) = R f as the solver's restriction forms it, after asserting that it zeroes a non-zero u(lvl + 1)"""
    S.upload(1, hip.BUF_R, _pad_r(S, f))
    S.upload(lvl + 1, hip.BUF_U, np.full(S._npshape(lvl + 1), 3.25))
    S.upload(lvl + 1, hip.BUF_RHS, np.full(S._npshape(lvl + 1), -7.5))
    S.op(hip.OP_RESTRICT, lvl)
    assert not S.download(lvl + 1, hip.BUF_U).any(), "the restriction leaves the coarse u zero"
    return S.download(lvl + 1, hip.BUF_RHS)


def _chunks(c_cnt, chunk):
    kc = max(1, min(chunk, c_cnt, 64))
    return kc, -(-c_cnt // kc)


@gpu
def test_the_seam(hip):
    """the knobs' own contract: a bad form is refused and changes nothing, (-1, -1, -1, -1) restores the built-in
    choices, and with those a small level takes the gather and the per-point kernels"""
    ns = [40, 34, 16]
    try:
        hip.transfer_cfg(restrict_min_points=0, prolong_min_points=0, rs_variant=8, rs_chunk=2)
        with pytest.raises(hip.NdsmHipError):
            hip.transfer_cfg(rs_variant=7)
        S = hip.MGSolver(ns, uniform_mesh(ns), BCS)
        try:
            assert S.transfer_form(1) == (8, 2, 4, 0)            # nx = 40 < 64: no tiled prolongation at any size
            with pytest.raises(hip.NdsmHipError):
                S.transfer_form(0)
            with pytest.raises(hip.NdsmHipError):
                S.transfer_form(S.ngrids)
            hip.transfer_cfg()
            assert S.transfer_form(1)[0] == 10                   # marked when it was built; form and chunk are back
            assert S.transfer_form(1)[1] * S.transfer_form(1)[2] >= 8
        finally:
            S.close()
        S = hip.MGSolver(ns, uniform_mesh(ns), BCS)
        try:
            assert S.transfer_form(1) == (0, 0, 0, 0)
        finally:
            S.close()
    finally:
        hip.transfer_cfg()


@gpu
@pytest.mark.parametrize("ns", RESTRICT_ROWS, ids=_tag)
def test_restriction_axis_classes(hip, port, ns):
    """restrict_k and the three forms of restrict_stream_k, level 1 -> 2, at every pair of the axis classes: coarse
    columns under / at / over one tile in x and y, odd nx (register-staged, element loads), z windows under a chunk,
    one full chunk, one plane over"""
    ns = list(ns)
    odd = ns[0] & 1
    ran = collections.Counter()
    try:
        for meshf in MESHES:
            mesh = meshf(ns)
            f = rand_field(_shp(ns), 3001)
            want = port.restrict(f, ns, mesh, 1)
            assert want.shape == _shp([n // 2 for n in ns]) and want.any()
            hip.transfer_cfg()
            S = hip.MGSolver(ns, mesh, BCS)
            try:
                assert S.transfer_form(1)[:3] == (0, 0, 0)
                assert np.array_equal(_restricted(hip, S, f), want), ("gather", meshf.__name__)
                ran["gather"] += 1
            finally:
                S.close()
            hip.transfer_cfg(restrict_min_points=0)
            S = hip.MGSolver(ns, mesh, BCS)
            try:
                for form in (5, 8, 10):
                    hip.transfer_cfg(restrict_min_points=0, rs_variant=form)
                    got, kc, nkc, _ = S.transfer_form(1)
                    assert 1 <= kc <= 64 and nkc == -(-(ns[2] // 2) // kc)
                    if form == 10 and odd:
                        assert got == 8, "odd nx: the DMA form is demoted to the register-staged one"
                        ran["rs10->8"] += 1
                        continue
                    assert got == form
                    assert np.array_equal(_restricted(hip, S, f), want), (form, meshf.__name__)
                    ran["rs%d" % form] += 1
            finally:
                S.close()
    finally:
        hip.transfer_cfg()
    for k, v in ran.items():
        assert v == len(MESHES)
        RAN[k] += 1


@gpu
@pytest.mark.parametrize("ns", CHUNK_SHAPES, ids=_tag)
def test_restriction_chunks(hip, port, ns):
    """the z chunks of the streamed restriction, forced: one chunk of exactly 64 coarse planes, 64 + a last chunk of
    one plane, chunks of one plane, of four - and the launcher's own choice, which depends on the card"""
    ns = list(ns)
    c_cnt = ns[2] // 2
    seen = set()
    try:
        for meshf in MESHES:
            mesh = meshf(ns)
            f = rand_field(_shp(ns), 3002)
            want = port.restrict(f, ns, mesh, 1)
            hip.transfer_cfg(restrict_min_points=0)
            S = hip.MGSolver(ns, mesh, BCS)
            try:
                for form in ((5, 8) if ns[0] & 1 else (5, 8, 10)):
                    for chunk in CHUNKS:
                        hip.transfer_cfg(restrict_min_points=0, rs_variant=form, rs_chunk=chunk)
                        got, kc, nkc, _ = S.transfer_form(1)
                        assert got == form
                        if chunk < 0:
                            assert 1 <= kc <= 64 and nkc == -(-c_cnt // kc)
                        else:
                            assert (kc, nkc) == _chunks(c_cnt, chunk)
                            seen.add((chunk, kc, nkc))
                        assert np.array_equal(_restricted(hip, S, f), want), (form, chunk, meshf.__name__)
            finally:
                S.close()
    finally:
        hip.transfer_cfg()
    assert (1, 1, c_cnt) in seen and (4, 4, -(-c_cnt // 4)) in seen
    assert (64, 64, 1 if c_cnt == 64 else 2) in seen and c_cnt in (64, 65)


@gpu
@pytest.mark.parametrize("ns", SIX_TAP_SHAPES + FIVE_TAP_SHAPES, ids=_tag)
def test_restriction_six_taps(hip, port, ns):
    """a pair 9 -> 4 or 11 -> 5 on any axis has coarse points with six taps, one more than the streamed kernel holds
    per axis: such a pair takes restrict_k - its all-six-taps edge - whatever the size says; the neighbouring sizes
    are streamed.  Every level pair of the hierarchy, against the port."""
    ns = list(ns)
    try:
        for meshf in MESHES:
            mesh = meshf(ns)
            shapes, _ = port.hierarchy(ns, mesh)
            shapes = [tuple(int(v) for v in s) for s in shapes]
            hip.transfer_cfg(restrict_min_points=0)
            S = hip.MGSolver(ns, mesh, BCS)
            try:
                assert S.shapes == shapes and len(shapes) >= 2
                six = []
                for lvl in range(1, len(shapes)):
                    pairs = set(zip(shapes[lvl - 1], shapes[lvl]))
                    form = S.transfer_form(lvl)[0]
                    if pairs & {(9, 4), (11, 5)}:
                        assert form == 0, (lvl, shapes[lvl - 1])
                        six.append(lvl)
                    elif lvl == 1:
                        assert form == 10 - 2 * (ns[0] & 1), (lvl, shapes[lvl - 1])
                    f = rand_field(shapes[lvl - 1][::-1], 3100 + lvl)
                    assert np.array_equal(_restricted(hip, S, f, lvl), port.restrict(f, ns, mesh, lvl)), (lvl, form)
                assert (1 in six) == (tuple(ns) in SIX_TAP_SHAPES)
            finally:
                S.close()
    finally:
        hip.transfer_cfg()


def _prolonged(hip, S, c, base):
    S.upload(2, hip.BUF_U, c)
    S.upload(1, hip.BUF_U, base)
    S.op(hip.OP_PROLONG, 1)
    return S.download(1, hip.BUF_U)


@gpu
@pytest.mark.parametrize("ns", PROLONG_ROWS + PROLONG_OUTSIDE, ids=_tag)
def test_prolongation_axis_classes(hip, port, ns):
    """prolong_tile_k<double> and prolong_add_k<3>, level 2 -> 1, u = 0 and u non-zero, at every pair of the axis
    classes: fine tiles of 64 x 8 x 8 whole, one point over, one under.  Just outside the tiled kernel's own
    conditions (nx = 63, 15 coarse points in y or z) the per-point kernel runs whatever the size says."""
    ns = list(ns)
    inside = tuple(ns) in PROLONG_ROWS
    ran = collections.Counter()
    try:
        for meshf in MESHES:
            mesh = meshf(ns)
            f = rand_field(_shp(ns), 3003)
            c = rand_field(_shp([n // 2 for n in ns]), 4003)
            want = port.interp(c, ns, mesh, 1)
            assert want.shape == f.shape
            hip.transfer_cfg()
            S = hip.MGSolver(ns, mesh, BCS)
            try:
                for name, size in (("tiled", 0), ("per-point", NEVER)):
                    hip.transfer_cfg(prolong_min_points=size)
                    tiled = S.transfer_form(1)[3]
                    assert tiled == (1 if name == "tiled" and inside else 0), (name, ns)
                    assert np.array_equal(_prolonged(hip, S, c, np.zeros_like(f)), want), (name, meshf.__name__, "u = 0")
                    assert np.array_equal(_prolonged(hip, S, c, f), f + want), (name, meshf.__name__, "u += P c")
                    ran[name] += 1
            finally:
                S.close()
    finally:
        hip.transfer_cfg()
    if inside:
        for k, v in ran.items():
            assert v == len(MESHES)
            RAN[k] += 1


# (ms, letters) of the slab Worlds.  ms = 5: post-smoothing is 1 + 2 + 2 sweeps and the one-sweep pass interpolates the
# correction itself (the fused smoother's own business: not this file's); ms = 4: 2 + 2, and a two-sweep pass with a
# right-hand side cannot, so the stand-alone prolongation runs on every slab.  The second set is Neumann at the upper x
# face: the smoother then reads the right-hand side of the last coarse column, which under Dirichlet nothing reads.
SLAB_CYCLES = ((5, "DNDDND"), (4, "DDDNDD"))


@gpu
@pytest.mark.parametrize("ns", SLAB_SHAPES, ids=_tag)
def test_slab_windows(hip, port, ns):
    """two V-cycles of a three-slab loop-back World with both sizes forced to 0, against port.vcycle: the streamed
    restriction with a window of the fine planes and pieces of the coarse ones (f_k0, c_k0, c_beg non-zero) in its
    three forms, and, in the cycles with ms = 4, the stand-alone prolongation with f_k0, f_beg and c_k0 non-zero -
    tiled where the level has the 16 coarse rows it needs (130x34x66), per point where not (130x18x66).  A World has no
    handle transfer_form takes; the seam is read per level pair when a slab's hierarchy is built, exactly as for a
    single domain, so the form is asserted on an MGSolver of the same shape built under the same setting.  That these
    kernels run inside the World is shown by scratch builds with one of them broken."""
    ns = list(ns)
    u, rhs = rand_field(_shp(ns), 2112), rand_field(_shp(ns), 2113)
    try:
        for meshf, (ms, bcs) in itertools.product(MESHES, SLAB_CYCLES):
            mesh = meshf(ns)
            want = port.vcycle(port.vcycle(u, rhs, mesh, bcs, ms=ms), rhs, mesh, bcs, ms=ms)
            hip.transfer_cfg(restrict_min_points=0, prolong_min_points=0)
            plan = hip.slab_plan(ns, mesh, 3)
            assert len(plan) == 3 and all(s["z1"] - s["z0"] >= 8 for s in plan)
            S = hip.MGSolver(ns, mesh, bcs, ms=ms)
            W = hip.World(ns, mesh, bcs, 3, ms=ms)
            try:
                assert W.nlocal == 3 and W.slabs[0]["k0"] < 0 < W.slabs[1]["k0"] and W.slabs[1]["cb0"] > 0
                W.upload(hip.BUF_RHS, rhs)
                for form in (10, 8, 5):
                    hip.transfer_cfg(restrict_min_points=0, prolong_min_points=0, rs_variant=form)
                    assert S.transfer_form(1)[0] == form and S.transfer_form(1)[3] == int(ns[1] // 2 >= 16)
                    W.upload(hip.BUF_U, u)
                    W.vcycle(2)
                    assert np.array_equal(W.download(hip.BUF_U), want), (form, ms, bcs, meshf.__name__)
            finally:
                W.close()
                S.close()
    finally:
        hip.transfer_cfg()


@gpu
def test_built_in_thresholds(hip):
    """the seam at its defaults, solvers only: the streamed restriction from exactly 6 Mi fine points on, the tiled
    prolongation from 2 Mi on - if a threshold moves, or a refactor switches a form off, this says so"""
    hip.transfer_cfg()
    for ns, restrict_streamed, prolong_tiled in (([256, 192, 128], True, True), ([256, 192, 127], False, True),
                                                 ([128, 128, 128], False, True), ([128, 128, 127], False, False)):
        npts = ns[0] * ns[1] * ns[2]
        assert (npts >= 6 << 20) == restrict_streamed and (npts >= 1 << 21) == prolong_tiled
        S = hip.MGSolver(ns, uniform_mesh(ns), BCS)
        try:
            form, kc, nkc, tiled = S.transfer_form(1)
            assert (form in (5, 8, 10)) == restrict_streamed and form in (0, 5, 8, 10), (ns, form)
            assert (kc >= 1 and nkc == -(-(ns[2] // 2) // kc)) if restrict_streamed else (kc, nkc) == (0, 0)
            assert tiled == int(prolong_tiled), ns
            for lvl in range(2, S.ngrids):                       # every smaller pair: gather, per point
                assert S.transfer_form(lvl) == (0, 0, 0, 0), (ns, lvl)
        finally:
            S.close()


@gpu
def test_every_form_ran():
    """no form may have dropped out of the cases above without notice: shapes per form"""
    short = {k: (RAN[k], n) for k, n in EXPECTED.items() if RAN[k] != n}
    assert not short and set(RAN) == set(EXPECTED), (
        "shapes that passed per form (got, expected) - a case above failed, or only part of the module ran: %r" % short)
