"""nlfff_model.history_row_model against references that share none of its partition (no GPU).

The energy: both sides add the same float64 terms w |B|^2; the reference is math.fsum of them, the exact sum rounded
once.  A term of the model passes through at most L additions (nlfff_model.chain_length: the points of a thread, 8 tree
levels, the partials of a thread of the final fold, 8 tree levels), each within 2^-53 relative of a sum of positive
numbers: the model is within (L + 1) 2^-53 of the exact sum (the + 1: the reference's own rounding).

The current-weighted sine: the reference evaluates curl_h B, J x B and the norms in np.longdouble (64 bits of
mantissa here: asserted) and adds each of the two sums exactly (every longdouble term as a float64 head and tail
through fsum).  The model's terms are float64 restatements of curl_h and carry their own rounding, a difference of
products that may cancel, so its allowance is measured, not derived: SINE_TOL is four times the largest relative
deviation of the plain numpy restatement test_gpu_nlfff.history_row from the longdouble reference over the cases below
(the model and the kernel differ from that restatement by summation order alone).  The figures are in DESIGN.md
section 25, and the test prints them again."""
import math

import numpy as np
import pytest

import nlfff_model as M
from alpha_model import ZLO
from golden_inputs import aniso_mesh, uniform_mesh
from line_model import abc, sheared
from test_gpu_nlfff import history_row

# (mesh, shape): the smallest grid, the anisotropic suite shape, 2050 rows of 257 points (two rows for blocks 0 and 1,
# two points for thread 0), the suite's wide shape (2400 rows of 300 points)
CASES = (("uniform", (4, 4, 4)), ("aniso", (17, 12, 9)), ("uniform", (257, 41, 50)), ("aniso", (257, 41, 50)),
         ("uniform", (300, 40, 60)), ("aniso", (300, 40, 60)))
IDS = ["%s-%s" % (k, "x".join(map(str, s))) for k, s in CASES]
MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}

# largest relative deviation of history_row's sine from the longdouble reference over CASES: 8.07e-16 (257 x 41 x 50,
# equal spacings; 1.4e-16 at 4 x 4 x 4, 2.2e-16 on the two large anisotropic grids, 0 on the rest); four times that
SINE_MEASURED = 8.07e-16
SINE_TOL = 4.0 * SINE_MEASURED

_CACHE = {}


def case(kind, shape):
    """(mesh, b_new, b_old, status), cached: the sheared field plus a tenth of an ABC field (currents of both, no
    symmetry), three nodes set to zero (|B| = 0: skipped by the two current sums), the sheared field as B_old, a
    seeded status of codes 1 .. 9"""
    if (kind, shape) not in _CACHE:
        mesh = MESHES[kind](shape)
        b_old = sheared(mesh)
        b_new = b_old + 0.1 * abc(mesh, k=2.3, phase=0.4)
        nz, ny, nx = b_new.shape[1:]
        for (k, j, i) in ((0, 0, 0), (nz // 2, ny // 2, nx // 2), (nz - 1, 1, nx - 1)):
            b_new[:, k, j, i] = 0.0
        status = np.random.default_rng(11).integers(1, 10, size=b_new.shape[1:]).astype(np.int32)
        _CACHE[(kind, shape)] = (mesh, b_new, b_old, status)
    return _CACHE[(kind, shape)]


def exact_sum(terms):
    """the exact sum of longdouble terms, rounded once to float64: each term as head + tail"""
    head = terms.astype(np.float64)
    tail = (terms - head.astype(np.longdouble)).astype(np.float64)
    return math.fsum(head.ravel().tolist() + tail.ravel().tolist())


def ld_gradient(f, h, axis):
    """derivq's differences in longdouble: (f[i+1] - f[i-1]) / 2h inside, (-3 f0 + 4 f1 - f2) / 2h on the end planes"""
    f = np.moveaxis(f, axis, 0)
    d = np.empty_like(f)
    d[1:-1] = (f[2:] - f[:-2]) / (2 * h)
    d[0] = (-3 * f[0] + 4 * f[1] - f[2]) / (2 * h)
    d[-1] = (3 * f[-1] - 4 * f[-2] + f[-3]) / (2 * h)
    return np.moveaxis(d, 0, axis)


def sine_reference(mesh, b_new):
    """sum w |J x B| / |B| over sum w |J| (points with |B| = 0 skipped), every term in longdouble, both sums exact"""
    ld = np.longdouble
    b = b_new.astype(ld)
    h = [ld(q[1]) - ld(q[0]) for q in mesh]
    ws = []
    for q, hq in zip(mesh, h):
        w = np.full(len(q), hq, dtype=ld)
        w[0] = w[-1] = hq / 2
        ws.append(w)
    w = ws[2][:, None, None] * ws[1][None, :, None] * ws[0][None, None, :]

    def g(f, axis):
        return ld_gradient(f, h[axis], 2 - axis)
    j = np.stack([g(b[2], 1) - g(b[1], 2), g(b[0], 2) - g(b[2], 0), g(b[1], 0) - g(b[0], 1)])
    bm = np.sqrt((b * b).sum(axis=0))
    ok = bm > 0
    cross = np.stack([j[1] * b[2] - j[2] * b[1], j[2] * b[0] - j[0] * b[2], j[0] * b[1] - j[1] * b[0]])
    num = (w * np.sqrt((cross * cross).sum(axis=0)))[ok] / bm[ok]
    den = (w * np.sqrt((j * j).sum(axis=0)))[ok]
    return exact_sum(num) / exact_sum(den)


def test_longdouble_is_wider_than_double():
    """the sine's reference needs it: on a platform whose longdouble is float64 this fails and says so (the reference
    would then be fsum of float64 terms, which shares the model's per-term rounding and proves less)"""
    assert np.finfo(np.longdouble).eps < 2e-19, np.finfo(np.longdouble)


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_model_against_exact_sums(kind, shape):
    mesh, b_new, b_old, status = case(kind, shape)
    nx, ny, nz = shape
    row = M.history_row_model(mesh, b_new, b_old, status)
    terms = M.point_terms(mesh, b_new, b_old, status)
    # the maximum and the count have no rounding of their own
    assert row[0] == np.abs(b_new - b_old).max() > 0.0
    assert row[3] == (status == ZLO).sum() > 0
    # the energy
    L = M.chain_length(nx, ny * nz)
    energy = 0.5 * math.fsum(terms["energy"].ravel().tolist())
    rel = abs(row[1] - energy) / energy
    print(kind, shape, "L =", L, "energy: model", row[1], "fsum", energy, "relative %.3e, allowed %.3e"
          % (rel, (L + 1) * 2.0 ** -53))
    assert rel <= (L + 1) * 2.0 ** -53
    # the sine
    sine = sine_reference(mesh, b_new)
    plain = history_row(mesh, b_new, b_old)[2]
    print(kind, shape, "sine: model", row[2], "longdouble", sine, "relative %.3e; plain numpy %.3e; allowed %.3e"
          % (abs(row[2] - sine) / sine, abs(plain - sine) / sine, SINE_TOL))
    assert 0.0 < sine < 1.0
    assert abs(row[2] - sine) <= SINE_TOL * sine
    assert abs(plain - sine) <= SINE_TOL * sine          # (the measurement behind SINE_TOL, repeated)


@pytest.mark.parametrize("shape", ((4, 4, 4), (257, 41, 50), (300, 40, 60), (256, 8, 256), (513, 3, 700)),
                         ids=lambda s: "x".join(map(str, s)))
def test_partition_takes_every_point_once(shape):
    """integer terms add exactly in any order: the sum of 1 over the partition is the number of points, the sum of the
    point's own index the triangular number, and the maximum of the indices the last one.  (513 x 3 x 700: three points
    per thread, 2100 rows for 2048 blocks.)"""
    nx, ny, nz = shape
    n = nx * ny * nz
    ones = np.ones((ny * nz, nx))
    idx = np.arange(n, dtype=np.float64).reshape(ny * nz, nx)
    assert M.kernel_sum(ones) == n
    assert M.kernel_sum(idx) == n * (n - 1) // 2 < 2 ** 53
    assert M.kernel_max(idx) == n - 1
    mask = (idx % 3) == 0
    assert M.kernel_sum(ones, mask) == mask.sum()
    # points per thread + 8 + partials per thread of the final fold + 8
    want = {(4, 4, 4): 1 + 8 + 1 + 8, (257, 41, 50): 4 + 8 + 8 + 8, (300, 40, 60): 4 + 8 + 8 + 8,
            (256, 8, 256): 1 + 8 + 8 + 8, (513, 3, 700): 6 + 8 + 8 + 8}
    assert M.chain_length(nx, ny * nz) == want[shape]


def test_ddq_is_numpy_gradient_to_rounding():
    """the model's differences against np.gradient(edge_order=2), the suite's other statement of derivq"""
    mesh = aniso_mesh((9, 7, 6))
    f = abc(mesh)[0]
    for axis in range(3):
        h = mesh[axis][1] - mesh[axis][0]
        want = np.gradient(f, h, axis=2 - axis, edge_order=2)
        assert np.abs(M.ddq(f, axis, h) - want).max() <= 1e-14 * np.abs(f).max() / h
