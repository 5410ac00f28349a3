"""GPU tests of the solver options at their edge values, on every solve path (run with -m gpu on an MI355X).

The options - ms, ncycles_max, niterex_max, vc_tol, ex_tol, the max / mean metric - are the stop logic of every solve
the library offers.  Here they take the values the rest of the suite leaves out: no sweep at all (ms = 0), 12, 14 and
22 post-smoothing sweeps (ms = 6, 7, 11), no V-cycle (ncycles_max = 0), no or one coarsest-grid sweep, zero
tolerances, negative values - on the plain, tail-launch, tracked, mixed-precision, side-by-side (lane), replayed-graph
and z-slab paths and through the pipeline.

Expected values come from the oracle port (pinned to the reference on these very options by
test_oracle.py::test_pipeline_options_reference / test_scalar_options_reference) or from a plain statement; where two
library paths are compared with each other, one of them is compared with the port in this module as well.

Tolerances: bit for bit wherever the suite compares that operation bit for bit (3-D and 2-D solves with a Dirichlet
face: u, du history, cycle count, coarsest-grid sweep counter; any two library paths).  All-Neumann solves carry the
mean shift, whose summation order differs between device and port: the rule of
test_gpu_project.py::test_all_neumann_3d_solver_matches_oracle (|du| <= 1e-13 max|u|, equal ierr and cycle count).
The pipeline (its face solves are all-Neumann) against the port: the rule of
test_gpu_parity.py::test_pipeline_vs_oracle_options (|dA| <= 1e-11 max|A|, |dB| <= 1e-11 max|A| 4/h, equal ierr).

Pruning: the scalar, tracked, slab and flat-shape matrices are pairwise selections (every pair of values of two
options occurs, so every value of every option occurs on every shape); the 2.2 M point shape takes one case per ms
value.  The pipeline runs its whole 93-case matrix at 24x20x18 on every path and against the port; at 64x64x64 and on
the flat shape the whole / pairwise matrix on every path and a pairwise / ncycles_max <= 1 part against the port.
"""
import ctypes
import itertools
import os

import numpy as np
import pytest

from golden_inputs import (BCS3, HUGE, OPTION_PIPELINE_SHAPE, aniso_mesh, negative_option_cases, noisy_case,
                           pipeline_option_cases, rand_field, uniform_mesh, zero_field_cases)

pytestmark = pytest.mark.gpu

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def _tag(ns):
    return "x".join(str(n) for n in ns)


def pairwise(*axes):
    """a small subset of the product of `axes` in which every pair of values of two axes occurs (greedy, and
    deterministic: the candidate that covers most uncovered pairs, the first of equals)"""
    todo = {(i, a, j, b) for i, j in itertools.combinations(range(len(axes)), 2) for a in axes[i] for b in axes[j]}
    cands = list(itertools.product(*axes))
    out = []
    while todo:
        def gain(c):
            return sum((i, c[i], j, c[j]) in todo for i, j in itertools.combinations(range(len(axes)), 2))
        best = max(cands, key=gain)
        out.append(best)
        todo -= {(i, best[i], j, best[j]) for i, j in itertools.combinations(range(len(axes)), 2)}
    return out


def test_pairwise_selection_covers_every_pair():
    axes = ((0, 1, 2, 5, 6, 7, 11), (0, 1, 3), (0, 1, 3, 10000), (False, True))
    sel = pairwise(*axes)
    assert len(sel) < 40
    for i, j in itertools.combinations(range(4), 2):
        assert {(c[i], c[j]) for c in sel} == set(itertools.product(axes[i], axes[j]))


class _env:
    """environment switches of the library for the length of a with block"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.keep = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# =====================================================================================================================
# scalar solves: MGSolver.solve against port.solve_bvp
# =====================================================================================================================
SC_MS = (0, 1, 2, 5, 6, 7, 11)
SC_NMAX = (0, 1, 3)
SC_NEX = (0, 1, 3, 10000)


def _neumann(bcs):
    return set(bcs) == {"N"}


def _problem(ns, meshf, bcs, seed=2112):
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, seed), rand_field(shp, seed + 1)
    if _neumann(bcs):
        rhs = rhs - rhs.mean()
    return mesh, u, rhs


def _solve_dev(hip, ns, mesh, bcs, u, rhs, ms, nmax, nex, mean, vc_tol=1e-10, precision=None, want_mixed=None):
    S = hip.MGSolver(ns, mesh, bcs, ms=ms, du_max=not mean, nmax_exact=nex)
    try:
        if precision is not None:
            assert S.set_precision(precision) == want_mixed, (ns, bcs, ms)
        S.upload(1, hip.BUF_U, u)
        if rhs is None:
            S.zero_rhs()
        else:
            S.upload(1, hip.BUF_RHS, rhs)
        ie, du, nc, h = S.solve(vc_tol=vc_tol, nmax=nmax, hist_len=8)
        return ie, du, nc, list(h), S.info()[0], S.download(1, hip.BUF_U)
    finally:
        S.close()


def _solve_port(port, mesh, bcs, u, rhs, ms, nmax, nex, mean, vc_tol=1e-10):
    r = np.zeros_like(u) if rhs is None else rhs
    ie, us, du, h, nc, sw = port.solve_bvp(u, r, mesh, bcs, ms=ms, nmax_exact=nex, du_max=not mean, vc_tol=vc_tol,
                                           nmax=nmax, hist_len=8)
    return ie, du, nc, list(h), sw, us


def mean_sum_bound(npts):
    """Relative distance allowed between two mean-metric du values of the SAME N non-negative differences added in
    two orders: the summation bound for non-negative terms, (N-1)u / (1 - (N-1)u) with u = 2^-53 - a sum in any
    order is within that of the exact sum.  Derived, not measured (the blocked sums of the device and the port's
    loop stay far inside it: their last bits differ).  max|du| does not depend on the order: compared exactly."""
    u = 2.0 ** -53
    return (npts - 1) * u / (1.0 - (npts - 1) * u)


def _same_du(got, want, npts, mean, what):
    """(ierr, du_last, ncycles, du history) of two library paths: exact for max|du|; for the mean metric the two
    paths add the differences in different orders (inside the last sweep's launch or in a pass of its own; per
    slab or over the whole level), so du may differ by mean_sum_bound - ierr and the cycle count may not"""
    assert got[0] == want[0] and got[2] == want[2], (what, got[:4], want[:4])
    if mean and want[2] > 0:
        rel = mean_sum_bound(npts)
        assert abs(got[1] - want[1]) <= rel * want[1], (what, got[1], want[1])
        assert len(got[3]) == len(want[3]), what
        assert np.all(np.abs(np.array(got[3]) - np.array(want[3])) <= rel * np.array(want[3])), (what, got[3], want[3])
    else:
        assert got[1] == want[1] and got[3] == want[3], (what, got[:4], want[:4])


def _same_solve(got, want, what, neumann=False, mean_vs_port=False):
    """(ierr, du_last, ncycles, du history, coarsest-grid sweeps, u) of two runs of one solve.  mean_vs_port: `want`
    is the port's and the metric is the mean - the device adds the N differences in another order than the port's
    loop, so du may differ by mean_sum_bound(N) (relative); u, the counts and ierr are exact all the same."""
    print(what, "ierr %d/%d nc %d/%d du %.17g/%.17g sweeps %d/%d max|du| %.3e" % (
        got[0], want[0], got[2], want[2], got[1], want[1], got[4], want[4], np.abs(got[5] - want[5]).max()))
    assert got[0] == want[0] and got[2] == want[2], what
    if not neumann or want[2] == 0:
        if mean_vs_port and want[2] > 0:
            rel = mean_sum_bound(want[5].size)
            assert abs(got[1] - want[1]) <= rel * want[1], (what, got[1], want[1])
            assert np.all(np.abs(np.array(got[3]) - np.array(want[3])) <= rel * np.array(want[3])), (what, got[3], want[3])
        else:
            assert got[1] == want[1] and got[3] == want[3], (what, got[3], want[3])
        assert got[4] == want[4], (what, got[4], want[4])
        assert np.array_equal(got[5], want[5]), what
    else:
        # test_gpu_project.py::test_all_neumann_3d_solver_matches_oracle: 1e-13 max|u| (the mean is summed in another
        # order); du is a max / mean of differences of such u, so it moves by no more than twice that
        tol = 1e-13 * np.abs(want[5]).max()
        assert np.abs(got[5] - want[5]).max() <= tol, what
        dtol = 2 * tol + (mean_sum_bound(want[5].size) if mean_vs_port else 0.0) * np.array(want[3])
        assert np.all(np.abs(np.array(got[3]) - np.array(want[3])) <= dtol) and abs(got[1] - want[1]) <= dtol[-1], what
        if want[4] <= 3 * want[2]:           # coarsest-grid solves that ran out of their 0, 1 or 3 sweeps
            assert got[4] == want[4], (what, got[4], want[4])
    if want[2] == 0:
        assert got[:3] == (1, HUGE, 0) and got[3] == [] and got[4] == 0, what


# shape, mesh, letter sets, the development switch of the tail launch, pruning
SCALAR_SHAPES = [
    pytest.param([17, 23, 19], uniform_mesh, BCS3 + ("NNNNNN",), 1, "pairs", id="17x23x19-tail"),
    pytest.param([17, 23, 19], uniform_mesh, BCS3 + ("NNNNNN",), 0, "pairs", id="17x23x19-no-tail"),
    pytest.param([17, 23, 19], aniso_mesh, BCS3 + ("NNNNNN",), 1, "pairs", id="aniso-17x23x19-tail"),
    pytest.param([129, 64, 66], uniform_mesh, BCS3 + ("NNNNNN",), 1, "pairs", id="129x64x66-colour-passes"),
    pytest.param([161, 120, 115], uniform_mesh, BCS3, 1, "values", id="161x120x115-fused-odd-nx"),
    pytest.param([27, 36], uniform_mesh, ("NNNN", "DNND"), 1, "pairs", id="27x36"),
    pytest.param([27, 36], aniso_mesh, ("NNNN", "DNND"), 1, "pairs", id="aniso-27x36"),
    pytest.param([70, 9], uniform_mesh, ("NNNN", "DNND"), 1, "pairs", id="70x9"),
]


@pytest.mark.parametrize("ns,meshf,bcsets,tail,prune", SCALAR_SHAPES)
def test_scalar_solve_options_vs_port(hip, port, ns, meshf, bcsets, tail, prune):
    """one solve per selected (ms, nmax, nmax_exact, metric, letters): u, ierr, du_last, the cycle count, the du
    history and the coarsest-grid sweep counter against the port.  17x23x19: the whole hierarchy below level 1 in
    the tail launch, and the same kernel by kernel; 129x64x66: level 1 on the colour passes, odd nx; 161x120x115:
    the fused launches (1+2+2 split: 12, 14, 22 sweeps in one call), odd nx, tracked form; 2-D: the face solves'
    hierarchies.  Then the zero problem: du = 0 does not meet vc_tol = 0 (the test is strict), it meets 1e-10."""
    L = hip.load_library()
    if prune == "pairs":
        cases = pairwise(SC_MS, SC_NMAX, SC_NEX, (False, True), bcsets)
    else:            # one case per ms, the other options in turn: every value of every option still occurs
        cases = [(ms, SC_NMAX[i % 3], SC_NEX[i % 4], bool(i % 2), bcsets[i % len(bcsets)])
                 for i, ms in enumerate(SC_MS)] + [(5, 3, 3, True, bcsets[0])]
    for ax, vals in enumerate((SC_MS, SC_NMAX, SC_NEX, (False, True), bcsets)):
        assert {c[ax] for c in cases} == set(vals)
    try:
        L.ndsm_hip_debug_tail(tail)
        for ms, nmax, nex, mean, bcs in cases:
            mesh, u, rhs = _problem(ns, meshf, bcs)
            want = _solve_port(port, mesh, bcs, u, rhs, ms, nmax, nex, mean)
            got = _solve_dev(hip, ns, mesh, bcs, u, rhs, ms, nmax, nex, mean)
            _same_solve(got, want, (_tag(ns), bcs, ms, nmax, nex, mean), neumann=_neumann(bcs) and ms + nex > 0,
                        mean_vs_port=mean)
            if nmax == 0:
                assert np.array_equal(got[5], u)
        bcs = bcsets[0]
        mesh, u, rhs = _problem(ns, meshf, bcs)
        z0 = np.zeros_like(u)
        for vt, ie_want, nc_want in ((0.0, 1, 3), (1e-10, 0, 1)):
            want = _solve_port(port, mesh, bcs, z0, z0, 5, 3, 10000, False, vc_tol=vt)
            got = _solve_dev(hip, ns, mesh, bcs, z0, z0, 5, 3, 10000, False, vc_tol=vt)
            _same_solve(got, want, (_tag(ns), "zero problem", vt))
            assert got[:3] == (ie_want, 0.0, nc_want), (vt, got[:3])
    finally:
        L.ndsm_hip_debug_tail(1)


def test_additive_entries_refuse_negative_counts(hip, port):
    """include/ndsm_hip.h: the solver and world handles refuse a negative ms or nmax_exact with 9002; a negative
    nmax of their solve runs no cycle, like 0"""
    ns = [17, 23, 19]
    mesh, u, rhs = _problem(ns, uniform_mesh, "NDDNDD")
    for kw in (dict(ms=-1), dict(nmax_exact=-3)):
        with pytest.raises(hip.NdsmHipError, match="9002"):
            hip.MGSolver(ns, mesh, "NDDNDD", **kw)
        with pytest.raises(hip.NdsmHipError, match="9002"):
            hip.World([64, 64, 64], uniform_mesh([64, 64, 64]), "NDDNDD", 2, **kw)
    S = hip.MGSolver(ns, mesh, "NDDNDD")
    assert S.L.ndsm_hip_mg_set_ms(S.h, -1) == 9002 and S.L.ndsm_hip_mg_set_ms(S.h, 2) == 0
    S.close()
    want = _solve_port(port, mesh, "NDDNDD", u, rhs, 5, -2, 10000, False)
    got = _solve_dev(hip, ns, mesh, "NDDNDD", u, rhs, 5, -2, 10000, False)
    _same_solve(got, want, "nmax = -2")
    assert got[:3] == (1, HUGE, 0) and np.array_equal(got[5], u)


# =====================================================================================================================
# tracked form (metric inside the last fused sweep): against the separate metric pass and against the port
# =====================================================================================================================
@pytest.mark.parametrize("ns", ([128, 128, 128], [144, 128, 128]), ids=_tag)
def test_tracked_solve_options(hip, port, ns):
    """level 1 of exactly 2 Mi points (the threshold of mg_track_applies) and above it, even nx: the default run,
    NDSM_HIP_NO_TRACK and the port - u, du history, counts, bit for bit - for ms in {1, 6, 7} x nmax in {0, 1, 2} x
    both metrics (pairwise), Poisson and declared-zero right-hand side.  ms = 0 cannot run tracked (no sweep to
    carry the metric): it takes the plain form and still equals the port."""
    cases = pairwise((1, 6, 7), (0, 1, 2), (False, True))
    assert {c[0] for c in cases} == {1, 6, 7} and {c[1] for c in cases} == {0, 1, 2}
    cases.append((0, 2, False))
    for i, (ms, nmax, mean) in enumerate(cases):
        bcs = ("NDDNDD", "DDNDDN")[i % 2]
        mesh, u, rhs = _problem(ns, uniform_mesh, bcs, seed=11)
        if i % 3 == 0:
            rhs = None
        want = _solve_port(port, mesh, bcs, u, rhs, ms, nmax, 10000, mean)
        with _env(NDSM_HIP_NO_TRACK=None):
            got = _solve_dev(hip, ns, mesh, bcs, u, rhs, ms, nmax, 10000, mean)
        with _env(NDSM_HIP_NO_TRACK="1"):
            plain = _solve_dev(hip, ns, mesh, bcs, u, rhs, ms, nmax, 10000, mean)
        _same_solve(got, want, (_tag(ns), "tracked", bcs, ms, nmax, mean), mean_vs_port=mean)
        _same_solve(plain, want, (_tag(ns), "no-track", bcs, ms, nmax, mean), mean_vs_port=mean)
        # (the mean metric: identical was tried first - at 128^3, ms = 1 the tracked form gave
        # 0.47744785824357555, the separate pass 0.4774478582435755: the two reductions add in different orders)
        _same_du(got, plain, u.size, mean, (_tag(ns), "tracked against no-track", bcs, ms, nmax, mean))
        assert got[4] == plain[4] and np.array_equal(got[5], plain[5]), (ms, nmax, mean)


# =====================================================================================================================
# mixed precision
# =====================================================================================================================
def test_mixed_precision_options(hip, port):
    """set_precision(2) at 128x64x160: without a V-cycle u is untouched (ierr 1, 0 cycles, du_last = huge); ms = 0
    cannot run the fp32 correction cycle: set_precision says so and the solve is the fp64 one, bit for bit; ms = 6,
    7: the single-domain mixed solve against the loop-back world, bit for bit (as
    test_slab_world_mixed_precision_bitwise does for smaller ms), and the mode really is on"""
    ns = [128, 64, 160]
    bcs = "NDDNDD"
    mesh, u, rhs = _problem(ns, uniform_mesh, bcs)
    for mean in (False, True):
        got = _solve_dev(hip, ns, mesh, bcs, u, rhs, 5, 0, 10000, mean, precision=2, want_mixed=True)
        assert got[:4] == (1, HUGE, 0, []) and np.array_equal(got[5], u), got[:4]
    for nmax in (0, 2):
        a = _solve_dev(hip, ns, mesh, bcs, u, rhs, 0, nmax, 10000, False, precision=2, want_mixed=False)
        b = _solve_dev(hip, ns, mesh, bcs, u, rhs, 0, nmax, 10000, False)
        _same_solve(a, b, ("mixed asked, ms = 0", nmax))
    want = _solve_port(port, mesh, bcs, u, rhs, 0, 2, 10000, False)
    _same_solve(b, want, "fp64, ms = 0, against the port")
    for ms, lap in ((6, False), (7, True)):
        r = None if lap else rhs
        a = _solve_dev(hip, ns, mesh, bcs, u, r, ms, 3, 10000, False, precision=2, want_mixed=True)
        f = _solve_dev(hip, ns, mesh, bcs, u, r, ms, 3, 10000, False)
        b = _solve_world(hip, ns, mesh, bcs, u, r, ms, 3, False, 2, precision=2)
        assert b[:4] == a[:4] and np.array_equal(b[4], a[5]), (ms, b[:4], a[:4])
        assert not np.array_equal(a[5], f[5]) and np.abs(a[5] - f[5]).max() <= 1e-6 * np.abs(f[5]).max(), ms


# =====================================================================================================================
# z-slab worlds (loop-back) against the single-domain solver
# =====================================================================================================================
def _solve_world(hip, ns, mesh, bcs, u, rhs, ms, nmax, mean, nranks, precision=None, vc_tol=1e-10):
    W = hip.World(ns, mesh, bcs, nranks, ms=ms, du_max=not mean)
    try:
        if precision is not None:
            assert W.set_precision(precision)
        W.upload(hip.BUF_U, u)
        if rhs is None:
            W.zero_rhs()
        else:
            W.upload(hip.BUF_RHS, rhs)
        ie, du, nc, h = W.solve(vc_tol=vc_tol, nmax=nmax, hist_len=8)
        return ie, du, nc, list(h), W.download(hip.BUF_U), W.dist_levels
    finally:
        W.close()


@pytest.mark.parametrize("ns,nranks,levels", (([128, 64, 160], 2, 0), ([64, 64, 256], 4, 2)), ids=str)
def test_slab_world_options(hip, port, ns, nranks, levels):
    """loop-back worlds, level 1 only and two levels distributed: ms in {0, 1, 6, 7} x nmax in {0, 1, 3} x both
    metrics (pairwise) against the single-domain solver, bit for bit (the mean metric's du: added slab by slab,
    within mean_sum_bound) - ms = 0 has no out-of-place pass for the world's buffer rotation - and the
    single-domain solver against the port for the ms = 0 and ms = 7 cases"""
    cases = pairwise((0, 1, 6, 7), (0, 1, 3), (False, True))
    assert {c[0] for c in cases} == {0, 1, 6, 7} and {c[1] for c in cases} == {0, 1, 3}
    ported = set()
    with _env(NDSM_HIP_DIST_LEVELS=str(levels) if levels else None):
        for i, (ms, nmax, mean) in enumerate(cases):
            bcs = ("NDDNDD", "DDNDDN")[i % 2]
            mesh, u, rhs = _problem(ns, uniform_mesh, bcs)
            if i % 3 == 1:
                rhs = None
            s = _solve_dev(hip, ns, mesh, bcs, u, rhs, ms, nmax, 10000, mean)
            w = _solve_world(hip, ns, mesh, bcs, u, rhs, ms, nmax, mean, nranks)
            if levels:
                assert w[5] == levels
            print(_tag(ns), nranks, levels, bcs, ms, nmax, mean, s[:4], w[:4])
            _same_du(w, s, u.size, mean, (ms, nmax, mean))
            assert np.array_equal(w[4], s[5]), (ms, nmax, mean)
            if nmax == 0:
                assert w[:4] == (1, HUGE, 0, []) and np.array_equal(w[4], u)
            if ms in (0, 7) and nmax == 1 and ms not in ported:
                ported.add(ms)
                _same_solve(s, _solve_port(port, mesh, bcs, u, rhs, ms, nmax, 10000, mean), ("single domain", ms),
                            mean_vs_port=mean)
    assert ported == {0, 7}


# =====================================================================================================================
# the pipeline: ndsm_vector_solve and VecPot.solve
# =====================================================================================================================
PATHS = (("default", {}), ("no-face-lanes", {"NDSM_HIP_FACE_LANES": "0"}), ("no-side3d", {"NDSM_HIP_NO_SIDE3D": "1"}),
         ("no-graphs", {"NDSM_HIP_NO_GRAPHS": "1"}), ("host-faces", {"NDSM_HIP_HOST_FACES": "1"}))
_SWITCHES = ("NDSM_HIP_FACE_LANES", "NDSM_HIP_NO_SIDE3D", "NDSM_HIP_NO_GRAPHS", "NDSM_HIP_HOST_FACES")


def vector_solve(L, x, y, z, b, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False):
    """ndsm_vector_solve as the reference's ndsm.py calls it, but the option vectors come back too:
    ierr, A, B, ioptc, ropt"""
    nshape = np.array(b.shape[::-1], dtype=np.intc)
    ioptc = np.zeros(16, dtype=np.intc)
    ropt = np.zeros(16)
    ioptc[L.get_iopt_ms()] = ms
    ioptc[L.get_iopt_ncycles()] = ncycles_max
    ioptc[L.get_iopt_iopt_nmaxex()] = niterex_max
    ioptc[L.get_iopt_dumax()] = 0 if mean else 1
    ropt[L.get_ropt_vtol()] = vc_tol
    ropt[L.get_ropt_ctol()] = ex_tol
    A = np.zeros(b.size)
    bb = np.ascontiguousarray(b, dtype=np.float64).ravel().copy()
    xs, ys, zs = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, y, z))
    ierr = L.ndsm_vector_solve(ctypes.c_size_t(bb.size), nshape.ctypes.data_as(_ip), ioptc.ctypes.data_as(_ip),
                               ropt.ctypes.data_as(_dp), xs.ctypes.data_as(_dp), ys.ctypes.data_as(_dp),
                               zs.ctypes.data_as(_dp), A.ctypes.data_as(_dp), bb.ctypes.data_as(_dp))
    assert ierr < 9000, (ierr, dict(ms=ms, ncycles_max=ncycles_max, niterex_max=niterex_max))
    return ierr, A.reshape(b.shape), bb.reshape(b.shape), ioptc, ropt


def _fresh(L):
    """drop the cached context (NDSM_HIP_NO_SIDE3D is read when it is built) and every recorded graph with it"""
    L.ndsm_hip_shutdown()
    assert L.ndsm_hip_init(0) == 0


def _same_call(L, got, want, what):
    """two library runs of one pipeline call: ierr, A, B, the whole ioptc, ropt but the wall time - identical"""
    assert got[0] == want[0], what
    assert np.array_equal(got[3], want[3]), (what, got[3], want[3])
    t = L.get_ropt_tim()
    assert np.array_equal(np.delete(got[4], t), np.delete(want[4], t), equal_nan=True), (what, got[4], want[4])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what


def _no_cycle_outputs(L, run, kw):
    if kw.get("ncycles_max", 1024) <= 0:
        assert run[3][L.get_iopt_fail3d()] == 0b111, kw
        assert run[3][L.get_iopt_ncyc_out()] == 0 and run[4][L.get_ropt_dulast()] == HUGE, kw
        assert run[0] == 1 and run[3][3] == 1, kw


def _vs_port(got, want, x, kw):
    """test_gpu_parity.py::test_pipeline_vs_oracle_options' rule, plus the option vector the reference leaves"""
    assert got[0] == want[0], kw
    assert np.array_equal(got[3][:8], want[3][:8]), (kw, got[3], want[3])
    scale = np.abs(want[1]).max()
    ea, eb = np.abs(got[1] - want[1]).max(), np.abs(got[2] - want[2]).max()
    print(kw, "ierr %d dA %.3e dB %.3e scale %.3e" % (got[0], ea, eb, scale))
    assert ea <= 1e-11 * scale, kw
    assert eb <= 1e-11 * scale * 4 / (x[1] - x[0]), kw


def _pipeline_paths(hip, port, x, y, z, b, kws, port_kws):
    """every keyword set on every path; the default path against the port for port_kws"""
    L = hip.load_library()
    runs = {}
    try:
        with _env(**{k: None for k in _SWITCHES}):
            for name, env in PATHS:
                with _env(**env):
                    _fresh(L)
                    runs[name] = [vector_solve(L, x, y, z, b, **kw) for kw in kws]
        for i, kw in enumerate(kws):
            _no_cycle_outputs(L, runs["default"][i], kw)
            for name, _e in PATHS[1:]:
                _same_call(L, runs[name][i], runs["default"][i], (name, kw))
            if kw in port_kws:
                _vs_port(runs["default"][i], port.vector_potential(x, y, z, b, **kw), x, kw)
    finally:
        _fresh(L)
    return runs["default"]


def _kw_pairs(ncyc=(0, 1, 3)):
    return [dict(ms=ms, ncycles_max=nc, niterex_max=nex, mean=mean)
            for ms, nc, nex, mean in pairwise((0, 1, 6, 7, 11), ncyc, (0, 1, 10000), (False, True))]


def test_pipeline_options_every_path_small(hip, port):
    """24x20x18, all three components iterate: the 93 option sets of test_oracle's pipeline matrix, the negative
    ones (taken as 0, as the reference does) and the zero field (du = 0 < vc_tol is strict) under the default
    (lanes + replayed graphs), NDSM_HIP_FACE_LANES=0, NDSM_HIP_NO_SIDE3D=1, NDSM_HIP_NO_GRAPHS=1 and
    NDSM_HIP_HOST_FACES=1: identical ierr, A, B, ioptc and ropt on all of them, and the port's ierr, ioptc[:8], A
    and B on every set.  Without a V-cycle: fail3d 0b111, 0 cycles, du_last = huge.  Then VecPot.solve, host and
    device entry, returns ndsm_vector_solve's bits and option vectors."""
    L = hip.load_library()
    x, y, z, b = noisy_case(OPTION_PIPELINE_SHAPE)
    kws = pipeline_option_cases() + negative_option_cases()
    assert len(kws) == 100
    runs = _pipeline_paths(hip, port, x, y, z, b, kws, kws)
    b0 = np.zeros_like(b)
    zruns = _pipeline_paths(hip, port, x, y, z, b0, zero_field_cases(), zero_field_cases())
    assert [r[0] for r in zruns] == [1, 0]
    assert zruns[0][3][L.get_iopt_fail3d()] == 0b111 and zruns[0][3][L.get_iopt_ncyc_out()] == 3
    assert zruns[1][3][L.get_iopt_fail3d()] == 0 and zruns[1][3][L.get_iopt_ncyc_out()] == 1
    assert zruns[0][4][L.get_ropt_dulast()] == 0.0 and not zruns[0][1].any()
    V = hip.VecPot(x, y, z)
    try:
        for i, kw in enumerate(kws):
            if i % 7 and kw.get("ncycles_max", 1) > 0 and kw.get("ms", 1) > 0:
                continue
            for device in (False, True):
                ierr, A, B = V.solve(b, device=device, **kw)
                _same_call(L, (ierr, A, B, V.last_ioptc, V.last_ropt), runs[i], ("VecPot", device, kw))
    finally:
        V.close()


def test_pipeline_options_every_path_64(hip, port):
    """64x64x64 (level 1 on the colour passes, component solves side by side with replayed graphs): the whole
    matrix on every path, a pairwise part and the extra sets against the port"""
    x, y, z, b = noisy_case([64, 64, 64])
    kws = pipeline_option_cases()
    port_kws = _kw_pairs() + [kws[90], kws[92]] + [dict(ncycles_max=-2), dict(ms=-1, ncycles_max=1)]
    kws = kws + port_kws[-2:]
    assert all(kw in kws for kw in port_kws)
    _pipeline_paths(hip, port, x, y, z, b, kws, port_kws)


FLAT = [192, 176, 32]          # z faces of 33792 points: their solves are replayed as graphs (>= 32768)


def test_pipeline_options_every_path_replayed_face_graphs(hip, port):
    """a flat shape whose z faces reach the size at which the 2-D face solves are replayed as recorded graphs: the
    pairwise matrix on every path, identical; against the port for ncycles_max in {0, 1} (the port is slow here)"""
    x, y, z, b = noisy_case(FLAT)
    assert FLAT[0] * FLAT[1] >= 32768
    kws = _kw_pairs()
    port_kws = [kw for kw in kws if kw["ncycles_max"] == 0][:1] + \
               [kw for kw in kws if kw["ncycles_max"] == 1 and kw["niterex_max"] <= 1][:2]
    assert len(port_kws) == 3
    _pipeline_paths(hip, port, x, y, z, b, kws, port_kws)


@pytest.mark.parametrize("ns", (FLAT, [64, 64, 64]), ids=_tag)
def test_pipeline_option_sequence_on_one_context(hip, ns):
    """calls on ONE cached context whose options change from call to call - no cycle and no sweeps after calls
    that recorded graphs, ordinary calls after those: every call returns what a fresh context returns for its
    options (A, B, ierr, ioptc, ropt); nothing is left from the call before - no recorded graph of other sweeps,
    no cycle count, du or fail bits"""
    L = hip.load_library()
    x, y, z, b = noisy_case(ns)
    seq = [dict(ncycles_max=4), dict(ncycles_max=4), dict(ncycles_max=0), dict(ncycles_max=4),
           dict(ms=0, ncycles_max=3), dict(ncycles_max=4), dict(ms=7, ncycles_max=2, mean=True),
           dict(ms=0, ncycles_max=0), dict(ncycles_max=-1, niterex_max=0), dict(ms=6, ncycles_max=3, niterex_max=1),
           dict(ncycles_max=4)]
    try:
        with _env(**{k: None for k in _SWITCHES}):
            want = {}
            for kw in seq:
                key = tuple(sorted(kw.items()))
                if key not in want:
                    _fresh(L)
                    want[key] = vector_solve(L, x, y, z, b, **kw)
            _fresh(L)
            for i, kw in enumerate(seq):
                got = vector_solve(L, x, y, z, b, **kw)
                _same_call(L, got, want[tuple(sorted(kw.items()))], (i, kw))
                _no_cycle_outputs(L, got, kw)
    finally:
        _fresh(L)


# =====================================================================================================================
# the other entries of the handle
# =====================================================================================================================
def _field_with_currents(ns):
    """mesh (equal spacing) and a field with currents and divergence whose flux through each of the six faces is
    zero up to rounding (cos(pi q) sums to nothing over [0, 1]): the flux-balance fields the pipeline adds to A
    are then of rounding size too, so the solved components can be compared with the port's"""
    mesh = uniform_mesh(ns)
    Z, Y, X = np.meshgrid(mesh[2], mesh[1], mesh[0], indexing="ij")
    k = np.pi
    b = np.stack([np.cos(k * Y) * (1 + Z) + np.sin(2 * k * X) * np.cos(k * Y), np.cos(k * Z) * (1 + X),
                  np.cos(k * X) * (1 + Y)])
    return mesh, b


def _start(a_c, c):
    """the initial guess of component c's solve: zero but for the Dirichlet data on the four tangential faces,
    which the solve leaves as they are"""
    u0 = np.zeros_like(a_c)
    for d in range(3):
        if d != c:
            idx = [slice(None)] * 3
            for k in (0, -1):
                idx[2 - d] = k
                u0[tuple(idx)] = a_c[tuple(idx)]
    return u0


def _curl(v, mesh):
    def g(f, axis):
        return np.gradient(f, mesh[axis][1] - mesh[axis][0], axis=2 - axis, edge_order=2)
    return np.stack([g(v[2], 1) - g(v[1], 2), g(v[0], 2) - g(v[2], 0), g(v[1], 0) - g(v[0], 1)])


def _hel_key(h):
    return tuple(h[:10])


def test_handle_entries_options(hip, port):
    """solve_field, helicity, project and the devore chain on one handle (33^3, a field with currents).
    ncycles_max = 0: ierr 1, fail3d 0b111 (field solve) / 0b111111 (helicity), project runs 0 cycles and returns B
    as passed.  ms in {0, 6}, two cycles: component c of the field solve is port.solve_bvp's result for
    -(curl b)_c, the letters BCS3[c] and the call's own Dirichlet data (ms = 5 for A_z, as the pipeline has it);
    host and device entries give identical bits, lanes on and off; after each such call a default
    call on the same handle gives the bits of a fresh handle."""
    import ndsm_amd
    L = hip.load_library()
    ns = [33, 33, 33]
    mesh, b = _field_with_currents(ns)
    J = _curl(b, mesh)
    opt = dict(vc_tol=1e-9)
    edge = (("none", dict(ncycles_max=0)), ("ms0", dict(ms=0, ncycles_max=2)), ("ms6", dict(ms=6, ncycles_max=2)))

    def entries(V, device, **kw):
        f = V.solve_field(b, device=device, **kw)
        fi, fr = V.last_ioptc.copy(), V.last_ropt.copy()
        h = V.helicity(b, device=device, return_fields=True, **kw)
        hi = V.last_ioptc.copy()
        p = V.project(b, device=device, return_phi=True, **kw)
        d = V.helicity(b, gauge="devore", return_fields=True, **kw)
        return f, fi, fr, h, hi, p, d

    def same(a, c, what):
        assert a[0][0] == c[0][0] and np.array_equal(a[0][1], c[0][1]) and np.array_equal(a[0][2], c[0][2]), what
        assert np.array_equal(a[1], c[1]) and a[2][L.get_ropt_dulast()] == c[2][L.get_ropt_dulast()], what
        assert _hel_key(a[3]) == _hel_key(c[3]) and np.array_equal(a[4], c[4]), what
        for k in (10, 11, 12):
            assert np.array_equal(a[3][k], c[3][k]) and np.array_equal(a[6][k], c[6][k]), (what, k)
        assert a[5][0] == c[5][0] and a[5][3:] == c[5][3:], what
        assert np.array_equal(a[5].B, c[5].B) and np.array_equal(a[5].phi, c[5].phi), what
        assert _hel_key(a[6]) == _hel_key(c[6]), what

    F = ndsm_amd.VecPot(*mesh)
    fresh = entries(F, False, **opt)
    F.close()
    assert fresh[0][0] == 0 and fresh[3].ierr == 0 and fresh[5].ierr == 0
    with _env(NDSM_HIP_NO_SIDE3D="1"):           # (read when a handle's 3-D hierarchies are built)
        N = ndsm_amd.VecPot(*mesh)
        per_kw_nolanes = {}
        for name, kw in edge:
            per_kw_nolanes[name] = entries(N, False, **kw)
        N.close()
    V = ndsm_amd.VecPot(*mesh)
    try:
        for name, kw in edge:
            host = entries(V, False, **kw)
            dev = entries(V, True, **kw)
            same(dev, host, (name, "device entry"))
            same(per_kw_nolanes[name], host, (name, "one after the other"))
            f, fi, fr, h, hi, p, d = host
            if name == "none":
                assert f[0] == 1 and fi[L.get_iopt_fail3d()] == 0b111 and fi[L.get_iopt_ncyc_out()] == 0
                assert fr[L.get_ropt_dulast()] == HUGE
                assert h.ierr == 1 and hi[L.get_iopt_fail3d()] == 0b111111
                assert p.ierr == 1 and p.ncycles == 0 and p.du_last == HUGE and np.array_equal(p.B, b)
                assert not p.phi.any() and p.E_removed == 0.0
                assert d.ierr == 1
            else:
                assert fi[L.get_iopt_ncyc_out()] == 2 and p.ncycles == 2
                for c in range(3):
                    msc = 5 if c == 2 else kw["ms"]
                    ie, uc, du, _h, nc, _sw = port.solve_bvp(_start(f[1][c], c), -J[c], mesh, BCS3[c], ms=msc, nmax=2,
                                                             vc_tol=1e-9)
                    # (the right-hand side is formed on the device and a flux-balance field of rounding size is
                    # added to the solved component: the rule of test_pipeline_vs_oracle_options, 1e-11 of the scale)
                    err = np.abs(f[1][c] - uc).max()
                    print(name, "component", c, "max|A - port| %.3e of %.3e" % (err, np.abs(uc).max()))
                    assert err <= 1e-11 * np.abs(uc).max(), (name, c, err)
            same(entries(V, False, **opt), fresh, (name, "default call afterwards"))
    finally:
        V.close()
