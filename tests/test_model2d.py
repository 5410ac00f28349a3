"""tests/model2d.py against the oracle, on the cases of tests/test_gpu_2d.py - CPU only.

What ties the model to the reference: on every boundary set with a Dirichlet face its sweeps, coarsest-grid solve,
V-cycle and solve are the oracle's bit for bit; on the all-Neumann set, where only the order of one sum differs, it
stays within the rounding bound of that sum - and is NOT bit-equal to the oracle's order, so the bitwise assertions
of the GPU tests can tell the orders apart.
"""
import math

import numpy as np
import pytest

import model2d as m2
from golden_inputs import aniso_mesh, rand_field, uniform_mesh
from model2d import gamma, neumann_bound

NON_NEUMANN = tuple(b for b in m2.BCS_2D if b != "NNNN")


def _tag(ns):
    return "x".join(str(n) for n in ns)


def _cases(shapes=m2.SHAPES_2D):
    return ([pytest.param(ns, uniform_mesh, id=_tag(ns)) for ns in shapes] +
            [pytest.param(ns, aniso_mesh, id="aniso-" + _tag(ns)) for ns in shapes if ns in list(m2.ANISO_2D)])


def _fields(ns):
    shp = tuple(ns[::-1])
    return rand_field(shp, 2112), rand_field(shp, 2113)


# ---------------------------------------------------------------------------------------------------------------------
# the sums
# ---------------------------------------------------------------------------------------------------------------------
SUM_SIZES = (1, 63, 64, 65, 255, 256, 257, 1800, 2048, 4096, 4104, 19321, 19456, 19458, 78000, 524288 + 513)


@pytest.mark.parametrize("n", SUM_SIZES)
def test_sum_orders_against_fsum_and_on_integers(n):
    v = rand_field((n,), 7)
    exact = math.fsum(v)
    tol = gamma(n) * math.fsum(np.abs(v))
    ints = np.random.default_rng(8).integers(-1000, 1000, n).astype(np.float64)
    for order in (lambda a: m2.wg_sum(a, 1024), lambda a: m2.wg_sum(a, 256), m2.two_stage_sum, m2.serial_sum):
        assert abs(order(v) - exact) <= tol
        assert order(ints) == float(int(ints.sum()))        # every partial sum is an integer below 2^53: exact
        assert order(np.arange(n, dtype=np.float64)) == n * (n - 1) / 2.0


def test_sum_orders_follow_the_kernels_lane_for_lane():
    """a scalar restatement of the kernels' loops (threads, lanes, shfl_down with every lane reading before it writes)"""
    def tree(lanes):
        lanes = list(lanes)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + (lanes[l + o] if l + o < 64 else lanes[l]) for l in range(64)]
        return lanes[0]

    def workgroup(v, threads):
        acc = []
        for t in range(threads):
            s = 0.0
            for p in range(t, len(v), threads):
                s = s + v[p]
            acc.append(s)
        return [tree(acc[w * 64:(w + 1) * 64]) for w in range(threads // 64)]

    for n in (100, 1800, 5250):
        v = [float(x) for x in rand_field((n,), 9)]
        red = workgroup(v, 1024)
        tot = 0.0
        for q in range(16):
            tot = tot + red[q]
        assert m2.wg_sum(v, 1024) == tot
        sh = workgroup(v, 256)
        assert m2.wg_sum(v, 256) == ((sh[0] + sh[1]) + sh[2]) + sh[3]
        nb = min(-(-n // 256), 2048)
        part = []
        for b in range(nb):
            acc = []
            for t in range(256):
                s = 0.0
                for p in range(b * 256 + t, n, nb * 256):
                    s = s + v[p]
                acc.append(s)
            ssm = [tree(acc[w * 64:(w + 1) * 64]) for w in range(4)]
            s = ssm[0]
            for w in range(1, 4):
                s = s + ssm[w]
            part.append(s)
        ssm = workgroup(part, 256)
        s = ssm[0]
        for w in range(1, 4):
            s = s + ssm[w]
        assert m2.two_stage_sum(v) == s


# ---------------------------------------------------------------------------------------------------------------------
# sweeps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,meshf", _cases())
def test_sweeps_are_the_oracles_bit_for_bit(port, ns, meshf):
    mesh = meshf(ns)
    u, rhs = _fields(ns)
    for bcs in NON_NEUMANN:
        want = port.relax_nd(u, rhs, mesh, bcs)
        assert np.array_equal(m2.sweep2d(u, rhs, mesh, bcs), want), bcs
        for _ in range(2):
            want = port.relax_nd(want, rhs, mesh, bcs)
        for variant in (0, 1):
            assert np.array_equal(m2.relax2d(u, rhs, mesh, bcs, 3, variant), want), bcs
    assert np.array_equal(m2.sweep2d(u, None, mesh, "DNND"), port.relax_nd(u, np.zeros_like(u), mesh, "DNND"))
    # all-Neumann with the oracle's own order: the same bits, three sweeps deep
    rhs0 = rhs - rhs.mean()
    want = u
    for _ in range(3):
        want = port.relax_nd(want, rhs0, mesh, "NNNN")
    assert np.array_equal(m2.relax2d(u, rhs0, mesh, "NNNN", 3, order=m2.serial_sum), want)


@pytest.mark.parametrize("ns,meshf", _cases())
def test_neumann_sweep_within_the_summation_bound_and_orders_distinguishable(port, ns, meshf):
    mesh = meshf(ns)
    u, rhs = _fields(ns)
    rhs0 = rhs - rhs.mean()
    want = port.relax_nd(u, rhs0, mesh, "NNNN")
    n = u.size
    for variant in (0, 1):
        got = m2.relax2d(u, rhs0, mesh, "NNNN", 1, variant)
        assert np.abs(got - want).max() <= neumann_bound(want, n), variant


def test_every_size_class_tells_the_summation_orders_apart(port):
    """The orders move the mean by 1e-18 .. 7e-17 here, which changes the bits of some point on most shapes but not on
    all.  Every size class (and variant 1, the two-stage order, on each) must have a shape on which the device-order
    mean does NOT give the oracle's bits after one sweep: there a kernel that summed in the oracle's - or any other -
    order would not pass the bitwise assertions of test_gpu_2d.py."""
    classes = {"small": lambda n: n <= m2.SMALL_2D, "medium": lambda n: m2.SMALL_2D < n <= m2.MEDIUM_2D,
               "colour": lambda n: n > m2.MEDIUM_2D}
    told_apart = {(c, v): [] for c in classes for v in (0, 1)}
    met = []
    for ns in m2.SHAPES_2D:
        mesh = uniform_mesh(ns)
        u, rhs = _fields(ns)
        rhs0 = rhs - rhs.mean()
        want = port.relax_nd(u, rhs0, mesh, "NNNN")
        cls = next(c for c, inside in classes.items() if inside(u.size))
        got = [m2.relax2d(u, rhs0, mesh, "NNNN", 1, variant) for variant in (0, 1)]
        for variant in (0, 1):
            if not np.array_equal(got[variant], want):
                told_apart[(cls, variant)].append(_tag(ns))
        if cls != "colour" and not np.array_equal(got[0], got[1]):     # the single-workgroup and the two-stage order
            met.append(_tag(ns))
    assert all(told_apart.values()), told_apart
    assert met


# ---------------------------------------------------------------------------------------------------------------------
# the coarsest-grid solve
# ---------------------------------------------------------------------------------------------------------------------
def exact_case(port, root, ngrids, level, meshf):
    """(ns, mesh, u, rhs) of the solved level"""
    shapes, meshes = port.hierarchy(root, meshf(root), ngrids)
    ns = [int(v) for v in shapes[level - 1]]
    u, rhs = _fields(ns)
    return ns, meshes[level - 1], u, rhs


def _port_exact(port, u, rhs, mesh, bcs, ex_tol, use_max, nmax):
    """the oracle's solve_exact: one V-cycle of a one-level hierarchy (u, sweep count)"""
    _ierr, out, _du, _hist, _nc, sw = port.solve_bvp(u, rhs, mesh, bcs, ms=0, ex_tol=ex_tol, du_max=use_max,
                                                     nmax_exact=nmax, vc_tol=0.0, nmax=1, ngrids=1)
    return out, sw


@pytest.mark.parametrize("root,ngrids,level", m2.EXACT_ROOTS, ids=lambda v: _tag(v) if isinstance(v, list) else str(v))
@pytest.mark.parametrize("meshf", (uniform_mesh, aniso_mesh), ids=("uniform", "aniso"))
def test_exact_solve_against_the_oracle_and_clear_of_ex_tol(port, root, ngrids, level, meshf):
    ns, mesh, u, rhs = exact_case(port, root, ngrids, level, meshf)
    nd = len(ns)
    exact = m2.exact2d if nd == 2 else m2.exact3d
    if nd == 3:      # the model's 3-D sweep is the oracle's
        for bcs in ("NDDNDD", "DDNDDN", "DNDDND", "DDDDDD"):
            assert np.array_equal(m2.sweep3d(u, rhs, mesh, bcs), port.relax3d(u, rhs, mesh, bcs)), bcs
    for bcs in m2.EXACT_BCS[nd]:
        alln = m2.all_neumann(bcs)
        r = rhs - rhs.mean() if alln else rhs
        for ex_tol, use_max, nmax in m2.EXACT_OPTIONS:
            got, sweeps, conv, dus = exact(u, r, mesh, bcs, ex_tol, use_max, nmax)
            tag = (bcs, ex_tol, use_max, nmax)
            assert sweeps == len(dus) and conv == (nmax == 10000), tag
            assert (3 <= sweeps <= 32) if conv else sweeps == nmax, (tag, sweeps)     # several sweeps, far from the cap
            # input condition: no stop decision within rounding of the threshold
            if ex_tol > 0:
                assert min(abs(d - ex_tol) / ex_tol for d in dus) > 1e-6, (tag, dus)
            # the loop itself: with every sum in the oracle's order it IS the oracle's solve_exact, all-Neumann sets
            # and the mean metric included
            want, sw = _port_exact(port, u, r, mesh, bcs, ex_tol, use_max, nmax)
            ser, ssw, _c, _d = exact(u, r, mesh, bcs, ex_tol, use_max, nmax, order=m2.serial_sum)
            assert ssw == sw and np.array_equal(ser, want), tag
            # with the device's orders: the same stop decisions (the margin above), hence the same sweep count, and
            # the same bits wherever no sum enters u
            assert sweeps == sw, tag
            if not alln:
                assert np.array_equal(got, want), tag


# ---------------------------------------------------------------------------------------------------------------------
# V-cycle and solve
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,meshf", _cases(m2.VCYCLE_SHAPES))
def test_vcycle_and_solve_are_the_oracles_bit_for_bit(port, ns, meshf):
    mesh = meshf(ns)
    u, rhs = _fields(ns)
    for bcs, ms in zip(NON_NEUMANN, (5, 1, 5, 1)):
        kw = dict(ms=ms, **m2.VCYCLE_KW)
        levels, _sw, _un = m2.vcycle2d(port, u, rhs, mesh, bcs, **kw)
        assert np.array_equal(levels[0][0], port.vcycle(u, rhs, mesh, bcs, **kw)), bcs
        ierr, got, du, hist, nc, sweeps, _unc = m2.solve2d(port, u, rhs, mesh, bcs, vc_tol=1e-9, nmax=6, **kw)
        ierr2, want, du2, hist2, nc2, sw2 = port.solve_bvp(u, rhs, mesh, bcs, vc_tol=1e-9, nmax=6, hist_len=8, **kw)
        assert (ierr, nc, sweeps, du) == (ierr2, nc2, sw2, du2) and hist == list(hist2), bcs
        assert np.array_equal(got, want), bcs
    # with every sum in the oracle's order the model IS the oracle on the all-Neumann set and with the mean metric too:
    # what the device-order runs of test_gpu_2d.py differ in is the sums alone
    rhs0 = rhs - rhs.mean()
    for bcs, ms, du_max in (("NNNN", 5, True), ("NNNN", 1, False), ("DNND", 5, False)):
        kw = dict(ms=ms, du_max=du_max, **m2.VCYCLE_KW)
        r = rhs0 if bcs == "NNNN" else rhs
        levels, _sw, _un = m2.vcycle2d(port, u, r, mesh, bcs, order=m2.serial_sum, **kw)
        assert np.array_equal(levels[0][0], port.vcycle(u, r, mesh, bcs, **kw)), bcs
        ierr, got, du, hist, nc, sweeps, _unc = m2.solve2d(port, u, r, mesh, bcs, vc_tol=1e-9, nmax=6,
                                                           order=m2.serial_sum, **kw)
        ierr2, want, du2, hist2, nc2, sw2 = port.solve_bvp(u, r, mesh, bcs, vc_tol=1e-9, nmax=6, hist_len=8, **kw)
        assert (ierr, nc, sweeps, du) == (ierr2, nc2, sw2, du2) and hist == list(hist2), bcs
        assert np.array_equal(got, want), bcs
