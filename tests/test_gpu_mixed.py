"""The mixed-precision solve (fp64 residual, fp32 correction V-cycle on level 1; csrc/mixed.hip, mg_solve_mixed)
against a CPU model of the same cycle, at the shapes where its kernels change path (run with -m gpu on an MI355X).

Every other mixed-precision test compares converged answers or two device paths with each other; iterative refinement
with a correct fp64 residual converges to the right answer even when the fp32 cycle is subtly wrong.  Here every CYCLE
is compared: u after 1, 2 and 3 cycles (vc_tol = 0, nmax = 1, 2, 3 from the same start) against

  ref64   the oracle's fp64 V-cycle (port.vcycle), and
  model   tests/mixed_model.py in float32: the same refinement with level 1 in numpy float32, operand for operand as
          the T = float kernels have it, levels >= 2 from the oracle (tied to the oracle by test_mixed_model.py).

The model turned out BIT-IDENTICAL to the device at every case (first run on an MI355X: u_1, u_2, u_3 of all 35
cases), so A below asserts equality - no margin.  dev_model = max|u_k(model) - ref64_k|, what a correct fp32
evaluation of the cycle costs against fp64 (3e-7 .. 1e-6 of max|u_1 - u_0|), is still printed with the device's figure
next to it: it is the scale a bound would have to be built from (4 dev_model was the plan) if a change to the kernels'
operation order ever ends the bit-identity on purpose.  A wrong stencil weight, mirror or transfer tap is an
O(max|e|) error at some point, five to six orders of magnitude above dev_model.

Shapes (mixed_model.MIXED_SHAPES): update_residual_k tiles x in 128 interior columns and y in 13 rows and cuts z into
chunks of >= 16 planes - a second x tile of one or two column pairs, a y tile of one row, a z chunk of one plane, the
smallest level the gate admits, odd ny / nz, an odd-nx level 2.  Cases (mixed_model.mixed_cases): five per shape.
"""
import math
import time

import numpy as np
import pytest

import mixed_model as mm
from golden_inputs import rand_field, uniform_mesh
from test_gpu_options import mean_sum_bound

pytestmark = pytest.mark.gpu

NCYC = 3


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def _fields(ns):
    shp = tuple(ns[::-1])
    return rand_field(shp, 2112), rand_field(shp, 2113) * 10.0


class _Solver:
    """one MGSolver for several solves from the same start; rhs None: the declared-zero right-hand side"""

    def __init__(self, hip, ns, mesh, bcs, ms, mean, u0, rhs, precision=2, want=True):
        self.hip, self.u0 = hip, u0
        self.S = hip.MGSolver(ns, mesh, bcs, ms=ms, du_max=not mean)
        if precision is not None:
            got = self.S.set_precision(precision)
            if got is not want:
                self.S.close()
                raise AssertionError("set_precision(%d) says %s at %s %s ms = %d" % (precision, got, ns, bcs, ms))
        if rhs is None:
            self.S.zero_rhs()
        else:
            self.S.upload(1, hip.BUF_RHS, rhs)

    def solve(self, nmax, vc_tol=0.0):
        self.S.upload(1, self.hip.BUF_U, self.u0)
        ie, du, nc, h = self.S.solve(vc_tol=vc_tol, nmax=nmax, hist_len=8)
        return ie, du, nc, list(h), self.S.download(1, self.hip.BUF_U)

    def close(self):
        self.S.close()


@pytest.mark.parametrize("case", mm.mixed_cases(), ids=mm.case_id)
def test_mixed_cycles_against_model(hip, port, case):
    ns, meshf, bcs, ms, mean, has_rhs = case
    mesh = meshf(ns)
    u0, rhs = _fields(ns)
    rhs = rhs if has_rhs else None
    npts = u0.size
    what = mm.case_id(case)

    # ---- the reference side: fp64 V-cycles and the float32 model ----
    t0 = time.time()
    zero = np.zeros_like(u0)
    ref = [u0]
    for _ in range(NCYC):
        ref.append(port.vcycle(ref[-1], zero if rhs is None else rhs, mesh, bcs, ms=ms, du_max=not mean))
    um, dum = mm.mixed_cycles(port, u0, rhs, mesh, bcs, ms, NCYC, mean, np.float32)
    t_model = time.time() - t0

    # ---- the device: nmax = 1, 2, 3 from the same start, the last one twice ----
    t0 = time.time()
    D = _Solver(hip, ns, mesh, bcs, ms, mean, u0, rhs)
    try:
        runs = [D.solve(k) for k in (1, 2, 3)]
        again = D.solve(3)
        vc_tol = math.sqrt(dum[1] * dum[2])
        stop = D.solve(8, vc_tol=vc_tol)
    finally:
        D.close()
    uploaded = None
    if rhs is None:
        Z = _Solver(hip, ns, mesh, bcs, ms, mean, u0, zero)
        try:
            uploaded = Z.solve(3)
        finally:
            Z.close()
    t_dev = time.time() - t0
    ud = [r[4] for r in runs]
    hist = runs[2][3]

    # A. the cycle itself: the device's iterates are the float32 model's, bit for bit (module docstring)
    for k in (1, 3):
        dev_model = np.abs(um[k - 1] - ref[k]).max()
        dev_device = np.abs(ud[k - 1] - ref[k]).max()
        print("RATIO %s k=%d dev_model %.3e dev_device %.3e (ratio %.3f) device-model %.3e" % (
            what, k, dev_model, dev_device, dev_device / dev_model, np.abs(ud[k - 1] - um[k - 1]).max()))
        assert dev_model > 0.0, (what, k)
    print("TIME %s model+ref %.2f s device %.2f s" % (what, t_model, t_dev))
    for k in range(NCYC):
        assert np.array_equal(ud[k], um[k]), (what, "u_%d" % (k + 1), np.abs(ud[k] - um[k]).max(),
                                              np.abs(um[k] - ref[k + 1]).max())

    # B. Dirichlet faces keep u0's bits (all of them on the uniform meshes; mixed_model.leak_free_faces)
    faces = mm.leak_free_faces(port, ns, mesh, bcs)
    assert faces or "D" not in bcs
    for k in range(NCYC):
        assert mm.faces_kept(ud[k], u0, faces), (what, k, faces)

    # C. the metric: hist[k] is max|e| (sum|e| / N) of the cycle; u_{k+1} - u_k gives e back up to one rounding in
    # u + e and one in the subtraction
    prev = u0
    for k in range(NCYC):
        d = np.abs(ud[k] - prev)
        tol = 2.0 ** -52 * max(np.abs(prev).max(), np.abs(ud[k]).max())
        if mean:
            val = math.fsum(d.ravel()) / npts               # (the exact sum, rounded once)
            tol += mean_sum_bound(npts) * val
        else:
            val = float(d.max())
        print("METRIC %s k=%d hist %.17g from u %.17g diff %.3e tol %.3e" % (what, k, hist[k], val, abs(hist[k] - val), tol))
        assert abs(hist[k] - val) <= tol, (what, k, hist[k], val, tol)
        prev = ud[k]
    # ... and, the iterates being the model's, the model's own e gives the metric directly: max|e| is exact, the sum
    # of |e| is the exact one (fsum) up to the order the device adds in
    for k in range(NCYC):
        assert abs(hist[k] - dum[k]) <= (mean_sum_bound(npts) * dum[k] if mean else 0.0), (what, k, hist[k], dum[k])

    # D. prefix and determinism
    for k in (1, 2, 3):
        ie, du, nc, h, _u = runs[k - 1]
        assert (ie, nc, len(h)) == (1, k, k) and h == hist[:k] and du == hist[k - 1], (what, k, ie, nc, h, hist)
    assert again[3] == hist and np.array_equal(again[4], ud[2]), (what, "repeat")

    # E. the declared-zero right-hand side is an uploaded zero one, bit for bit
    if uploaded is not None:
        assert uploaded[:4] == runs[2][:4] and np.array_equal(uploaded[4], ud[2]), (what, uploaded[:4], runs[2][:4])

    # F. the stopping rule: du_1, du_2 >= vc_tol > du_3 (strict) - the model's values say where to put vc_tol
    assert dum[2] < vc_tol < dum[1] <= dum[0], (what, dum)
    assert (stop[0], stop[2]) == (0, 3) and stop[3] == hist and stop[1] == hist[2], (what, stop[:4], vc_tol)
    assert np.array_equal(stop[4], ud[2]), what


GATE_CASES = [([64, 32, 31], "NDDNDD"), ([64, 31, 32], "NDDNDD"), ([62, 32, 32], "NDDNDD"), ([65, 32, 32], "NDDNDD"),
              ([66, 35, 17], "NDDNDD"), ([64, 32, 32], "NNNNNN")]


@pytest.mark.parametrize("ns,bcs", GATE_CASES, ids=["x".join(map(str, ns)) + "-" + b for ns, b in GATE_CASES])
def test_gate_refuses_and_runs_fp64(hip, ns, bcs):
    """where mg_mixed_applies refuses - a level-2 axis below 16, nx below 64 or odd, all-Neumann - set_precision(2)
    says so and the solve is the fp64 one, bit for bit"""
    mesh = uniform_mesh(ns)
    u0, rhs = _fields(ns)
    if set(bcs) == {"N"}:
        rhs = rhs - rhs.mean()
    out = []
    for precision, want in ((None, None), (2, False)):
        D = _Solver(hip, ns, mesh, bcs, 5, False, u0, rhs, precision, want)
        try:
            out.append(D.solve(2))
        finally:
            D.close()
    assert out[0][:4] == out[1][:4] and out[0][2] == 2, (out[0][:4], out[1][:4])
    assert np.array_equal(out[0][4], out[1][4])


def test_mode1_threshold(hip):
    """mode 1 takes the mixed path from 6 * 2^20 points on: 256 x 192 x 128 is exactly that many (and then runs what
    mode 2 runs, bit for bit), 256 x 192 x 126 is below"""
    ns = [256, 192, 128]
    assert ns[0] * ns[1] * ns[2] == 6 * 2 ** 20
    mesh = uniform_mesh(ns)
    u0, rhs = _fields(ns)
    out = []
    for precision in (1, 2):
        D = _Solver(hip, ns, mesh, "NDDNDD", 5, False, u0, rhs, precision, True)
        try:
            out.append(D.solve(1))
        finally:
            D.close()
    assert out[0][:4] == out[1][:4] and out[0][2] == 1, (out[0][:4], out[1][:4])
    assert np.array_equal(out[0][4], out[1][4])
    ns = [256, 192, 126]
    S = hip.MGSolver(ns, uniform_mesh(ns), "NDDNDD")
    try:
        assert S.set_precision(1) is False
        assert S.set_precision(2) is True        # (it is the size that mode 1 refuses, not the shape)
    finally:
        S.close()
