"""The block-resident smoother (csrc/smooth_block.hip): the launch `relax` takes on whole 3-D levels of more than
4096 points that the z-streaming fused kernel declines (run with -m gpu on an MI355X).

Everything is compared BIT FOR BIT: OP_RELAX (the new path: two sweeps per launch, a last single one for odd counts,
out of place) against OP_RELAX_COLOR (one colour per launch, in place) on the same solver, and against the oracle
port's relax3d.  The one exception is the all-Neumann letter set against the ORACLE: there relax falls back to the
colour passes + mean shift (so OP_RELAX == OP_RELAX_COLOR exactly), and the device adds the mean as a tree where
the port adds it in a loop.  Bound used for that comparison only, derived and not measured: two sums of the same N
numbers of magnitude <= V differ by at most 2 g V in their mean, g = mean_sum_bound(N); the shift u - m carries
that over to every point (plus two roundings), and a later sweep - a convex combination of neighbours, then
another shift by a mean - at most doubles a difference.  With V_s <= max|u_(s-1)| + max|rhs| (the smoother's
weights are non-negative and add up to one, w1 < 1 on these meshes): tol_s = 2 tol_(s-1) + 8 (g + 2^-53) V_s.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_inputs import aniso_mesh, digest, noisy_case, rand_field, uniform_mesh

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def mean_sum_bound(npts):
    """a sum of N numbers in any order is within (N-1)u / (1 - (N-1)u) of the exact sum, relative to the sum of
    their magnitudes (u = 2^-53)"""
    u = 2.0 ** -53
    return (npts - 1) * u / (1.0 - (npts - 1) * u)

# Fortran order [nx, ny, nz]: the smallest level above the single-workgroup limit (odd nx); 18x17x17; one axis
# shorter than block + ring, so that both faces lie in one halo (y, then x); a thin z; partial blocks on every
# axis; 64^3 (a level of the benchmarked hierarchy)
SHAPES = ([17, 16, 16], [18, 17, 17], [40, 6, 20], [6, 40, 24], [34, 33, 9], [33, 20, 41], [64, 64, 64])
BCS = ("NDDNDD", "DDDDDD", "DDDNNN", "NNNNNN")      # lower faces then upper faces; the last falls back
COUNTS = (1, 2, 3, 5, 10)


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


def _cases(shapes):
    return ([pytest.param(ns, uniform_mesh, id=_tag(ns)) for ns in shapes] +
            [pytest.param(ns, aniso_mesh, id="aniso-" + _tag(ns)) for ns in shapes])


def _solver(hip, ns, mesh, bcs, rhs, **kw):
    S = hip.MGSolver(ns, mesh, bcs, **kw)
    if rhs is None:
        S.zero_rhs()
    else:
        S.upload(1, hip.BUF_RHS, rhs)
    return S


@pytest.mark.parametrize("ns,meshf", _cases(SHAPES))
def test_relax_ops_bitwise(hip, port, ns, meshf):
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    assert shp[0] * shp[1] * shp[2] > 4096
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    zero = np.zeros(shp)
    for bcs in BCS:
        for lap in (False, True):
            what = (bcs, "zero rhs" if lap else "rhs")
            r = zero if lap else rhs
            want, tol = {0: u}, {0: 0.0}                      # the oracle's sweeps, computed once per input
            for s in range(1, max(COUNTS) + 1):
                want[s] = port.relax3d(want[s - 1], r, mesh, bcs)
                v = np.abs(want[s - 1]).max() + np.abs(r).max()
                tol[s] = 2.0 * tol[s - 1] + 8.0 * (mean_sum_bound(u.size) + 2.0 ** -53) * v
            S = _solver(hip, ns, mesh, bcs, None if lap else rhs)

            def check(got, s, tag):
                if bcs == "NNNNNN":
                    assert np.abs(got - want[s]).max() <= tol[s], (what, tag, s)
                else:
                    assert np.array_equal(got, want[s]), (what, tag, s)

            for n in COUNTS:
                S.upload(1, hip.BUF_U, u)
                S.op(hip.OP_RELAX_COLOR, 1, n)
                colour = S.download(1, hip.BUF_U)
                S.upload(1, hip.BUF_U, u)
                S.op(hip.OP_RELAX, 1, n)
                got = S.download(1, hip.BUF_U)               # wherever the result landed, download finds it
                assert np.array_equal(got, colour), (what, n)
                check(got, n, "relax")
            # calls in a row, no upload in between: an odd and an even number of out-of-place launches, then the
            # in-place colour passes on whichever array holds the level now
            S.upload(1, hip.BUF_U, u)
            S.op(hip.OP_RELAX, 1, 1)
            check(S.download(1, hip.BUF_U), 1, "chain")
            S.op(hip.OP_RELAX, 1, 2)
            check(S.download(1, hip.BUF_U), 3, "chain")
            S.op(hip.OP_RELAX_COLOR, 1, 2)
            check(S.download(1, hip.BUF_U), 5, "chain")
            S.op(hip.OP_RELAX, 1, 5)
            check(S.download(1, hip.BUF_U), 10, "chain")
            S.close()


@pytest.mark.parametrize("ns,meshf", _cases(([18, 17, 17], [33, 20, 41], [64, 64, 64])))
def test_relax_plus_residual_bitwise(hip, ns, meshf):
    """OP_RELAX_RES: u and r of the new path against the colour passes + residual3"""
    mesh = meshf(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    for bcs in BCS[:3]:
        for lap in (False, True):
            S = _solver(hip, ns, mesh, bcs, None if lap else rhs)
            for n in (1, 5):
                S.upload(1, hip.BUF_U, u)
                S.op(hip.OP_RELAX_COLOR, 1, n)
                S.op(hip.OP_RESIDUAL, 1)
                a, ra = S.download(1, hip.BUF_U), S.download(1, hip.BUF_R)
                S.upload(1, hip.BUF_U, u)
                S.upload(1, hip.BUF_R, np.full(shp, np.nan))
                S.op(hip.OP_RELAX_RES, 1, n)
                assert np.array_equal(a, S.download(1, hip.BUF_U)), (bcs, lap, n)
                assert np.array_equal(ra, S.download(1, hip.BUF_R)), (bcs, lap, n)
            S.close()


@pytest.mark.parametrize("ns", ([40, 36, 33], [64, 64, 64]), ids=_tag)
def test_cycles_vs_oracle(hip, port, ns):
    """level 1 and the coarse levels above 4096 points take the new path: two V-cycles, then a solve to
    vc_tol = 1e-10 - u, the du history and the cycle count against the oracle port"""
    mesh = uniform_mesh(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 31), rand_field(shp, 32) * 10.0
    bcs = "NDDNDD"
    S = _solver(hip, ns, mesh, bcs, rhs)
    S.upload(1, hip.BUF_U, u)
    S.vcycle(2)
    want = port.vcycle(port.vcycle(u, rhs, mesh, bcs), rhs, mesh, bcs)
    assert np.array_equal(S.download(1, hip.BUF_U), want)
    ie2, u2, du2, h2, nc2, _sw = port.solve_bvp(u.copy(), rhs, mesh, bcs, vc_tol=1e-10, nmax=64, hist_len=64)
    S.upload(1, hip.BUF_U, u)
    ie, du, nc, h = S.solve(vc_tol=1e-10, nmax=64, hist_len=64)
    got = S.download(1, hip.BUF_U)
    S.close()
    assert ie == ie2 == 0 and nc == nc2 and du == du2 and list(h) == list(h2[:nc]), (list(h), list(h2[:nc2]))
    assert np.array_equal(got, u2)


def _vecpot_digests(n):
    import ndsm_amd
    x, y, z, b = noisy_case(n)
    ierr, A, B = ndsm_amd.vector_potential(x, y, z, b)
    return "%d %s %s" % (ierr, digest(A), digest(B))


def test_vector_potential_recorded_cycles_bitwise(hip):
    """40^3: the three component solves side by side, their cycles recorded and replayed (the block launch sets no
    function attribute and asks no occupancy, so it may be recorded), against one after the other in a fresh process"""
    got = _vecpot_digests(40)
    env = dict(os.environ, NDSM_HIP_NO_SIDE3D="1")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_block_smoother as t; "
            "print('digests', t._vecpot_digests(40))" % (os.path.dirname(HERE), HERE))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert got.split()[0] == "0" and "digests " + got in out.stdout, (got, out.stdout[-500:])
