"""GPU tests of the two Grad-Rubin entries at their edges (run with -m gpu on an MI355X): VecPot.solve_current and
VecPot.force_free where test_gpu_nlfff.py does not reach.

  A. the history row bit for bit against nlfff_model.history_row_model at shapes where both stride loops of
     nlfff_part_k run (more than 256 points per row, more than 2048 rows) and where they just do not
  B. the smallest shapes the handle takes: the driver against the hand-built chain for 1, 2 and 3 passes, every row
     of the history against the model
  D. the options ms, ncycles_max, niterex_max, mean, flxcrl and mixed_precision on both entries (a pairwise selection)
  E. identities that include/ndsm_hip.h states: the potential start, polarity -1, status = NULL, "only its faces are
     read"
  F. one handle shared with the helicity, projection, trace and DeVore entries, in two orders

(C, the device entries on offset caller arrays, is section e of test_gpu_caller_arrays.py.)  Everything is compared bit
for bit: the driver is documented to run the kernels of the chain alpha_map -> solve_current in the same order, the
reductions are deterministic, and nothing in the library branches on where an array lies."""
import ctypes

import numpy as np
import pytest

from alpha_model import ZLO
from golden_inputs import aniso_mesh, uniform_mesh
from line_model import abc, sheared
from nlfff_model import history_row_model
from test_gpu_nlfff import VC_TOL, curl
from test_gpu_options import pairwise

pytestmark = pytest.mark.gpu

MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
IDS = lambda s: "x".join(map(str, s))   # noqa: E731
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(got, want, what):
    """two results of one call - tuples of arrays, numbers and None, named tuples included - bit for bit"""
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        if g is None or w is None:
            assert g is None and w is None, (what, k)
        elif isinstance(g, np.ndarray):
            assert bits_equal(g, w), (what, k, float(np.nanmax(np.abs(g.astype(float) - w.astype(float)))))
        else:
            assert np.array([g]).tobytes() == np.array([w]).tobytes(), (what, k, g, w)


def case(kind, shape):
    """mesh, the sheared field (B_z = 1 everywhere, a current of its own) and boundary_alpha's alpha0 of it"""
    import ndsm_amd
    mesh = MESHES[kind](shape)
    b = sheared(mesh)
    alpha0 = ndsm_amd.boundary_alpha(mesh[0], mesh[1], b, 1e-3)
    assert np.abs(alpha0).max() > 0.1
    return mesh, b, alpha0


def chain_steps(V, b, alpha0, passes, b0=None, a0=None, polarity=1, step=0.5, **opts):
    """test_gpu_nlfff.chain with everything kept: alpha_map -> numpy j = alpha * B^k -> solve_current(b's B.n, j, A^k),
    `passes` times from (b0 - None: b -, a0).  Returns the fields B^0 .. B^passes, the last A, the alpha and status of
    every pass, the ierr of every solve and the option vectors the last solve left."""
    fields, ak, alphas, stats, ierrs, iopts = [b if b0 is None else b0], a0, [], [], [], []
    for _ in range(passes):
        alpha, status = V.alpha_map(fields[-1], alpha0, polarity=polarity, step=step)
        ierr, ak, bk = V.solve_current(b, alpha * fields[-1], a_init=ak, **opts)
        fields.append(bk)
        alphas.append(alpha)
        stats.append(status)
        ierrs.append(ierr)
        iopts.append((V.last_ioptc.copy(), V.last_ropt.copy()))
    return fields, ak, alphas, stats, ierrs, iopts


def assert_rows(mesh, hist, fields, stats, what, exact_sine=True):
    """every row of the history is the model's row of (B^{k+1}, B^k, the status of pass k), bit for bit"""
    assert len(hist) == len(fields) - 1 == len(stats), what
    for k in range(len(hist)):
        row = history_row_model(mesh, fields[k + 1], fields[k], stats[k])
        print(what, "pass", k, "hist", hist[k].tolist(), "model", row.tolist())
        for q in (0, 1, 3) + ((2,) if exact_sine else ()):
            assert hist[k, q].tobytes() == row[q].tobytes(), (what, k, q, hist[k, q], row[q])
        assert hist[k, 3] == (stats[k] == ZLO).sum()


# ---------------------------------------------------------------------------------------------------------------------
# A. the history row where the stride loops of nlfff_part_k run
# ---------------------------------------------------------------------------------------------------------------------
# 257 x 41 x 50: 2050 rows, blocks 0 and 1 own two; 257 points, thread 0 owns two per row.  300 x 40 x 60: the suite's
# wide shape (2400 rows of 300).  256 x 8 x 256: exactly one point per thread and exactly 2048 rows.
METRIC_SHAPES = ((257, 41, 50), (300, 40, 60), (256, 8, 256))


@pytest.mark.parametrize("shape", METRIC_SHAPES, ids=IDS)
@pytest.mark.parametrize("kind", list(MESHES))
def test_history_row_is_the_model_bit_for_bit(hip, kind, shape):
    """force_free(start="given", niter_max=1) returns B^1 and the status of its one pass, B^0 is the caller's: the row
    of the history against the model on them, all four entries bit for bit, host and device entry.  (Three V-cycles per
    solve: the row is that of whatever field came out, and the test is about the reduction.)"""
    import ndsm_amd
    mesh, b, alpha0 = case(kind, shape)
    V = ndsm_amd.VecPot(*mesh)
    try:
        runs = [V.force_free(b, alpha0, start="given", niter_max=1, step=0.5, ncycles_max=3, device=device)
                for device in (False, True)]
    finally:
        V.close()
    for device, (ierr, _A, B1, _alpha, status, hist) in zip((False, True), runs):
        assert ierr in (0, 1) and hist.shape == (1, 4) and np.isfinite(B1).all()
        assert_rows(mesh, hist, [b, B1], [status], "%s %s device %s" % (kind, shape, device))
        assert 0.0 < hist[0, 2] < 1.0 and 0 < hist[0, 3] <= status.size
    assert_same(runs[1][1:], runs[0][1:], "device entry against host entry")


# ---------------------------------------------------------------------------------------------------------------------
# B. the smallest shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((4, 4, 4), (4, 4, 5), (5, 7, 4)), ids=IDS)
@pytest.mark.parametrize("kind", list(MESHES))
def test_driver_is_the_chain_at_the_smallest_shapes(hip, kind, shape):
    """four points per axis is the handle's minimum: one-sided differences meet in the middle of an axis, a block of the
    reduction has four live threads.  Driver = chain bit for bit in A, B and alpha for 1, 2 and 3 passes, host and
    device entry; every row of the history is the model's."""
    import ndsm_amd
    mesh, b, alpha0 = case(kind, shape)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for passes in (1, 2, 3):
            fields, ak, alphas, stats, ierrs, _io = chain_steps(V, b, alpha0, passes, vc_tol=VC_TOL)
            for device in (False, True):
                what = "%s %s %d passes device %s" % (kind, shape, passes, device)
                ierr, A, B, alpha, status, hist = V.force_free(b, alpha0, start="given", niter_max=passes, step=0.5,
                                                               vc_tol=VC_TOL, device=device)
                assert ierr == max(ierrs) and hist.shape == (passes, 4), what
                assert_same((A, B, alpha, status), (ak, fields[-1], alphas[-1], stats[-1]), what)
                assert_rows(mesh, hist, fields, stats, what)
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------------
# D. the options on both entries
# ---------------------------------------------------------------------------------------------------------------------
OPTION_SETS = [dict(ms=ms, ncycles_max=nc, niterex_max=nex, mean=mean, flxcrl=fl, mixed_precision=mp)
               for ms, nc, nex, mean, fl, mp in pairwise((0, 1, 6), (0, 1, 3), (0, 1, 10000), (False, True),
                                                         (False, True), (False, True))]


@pytest.mark.parametrize("kind,shape", (("aniso", (17, 12, 9)), ("uniform", (24, 20, 18))), ids=lambda v: v if isinstance(v, str) else IDS(v))
def test_options_on_both_entries(hip, kind, shape):
    """Every option set of a pairwise selection, two passes from the given start:
      - the driver is the chain alpha_map + solve_current with the same options bit for bit (A, B, alpha, status, the
        history against the model on the chain's fields), the host entry is the device entry;
      - the option vectors: every slot of ioptc and ropt but the wall time is that of the chain's LAST solve_current,
        except ioptc[IOPT_IERR] and ioptc[fail3d], which the header defines over every pass: the largest ierr and the
        union of the fail bits of the chain's solves.  Found: that is what the driver leaves;
      - mixed_precision = True gives the bits of False (at these sizes mode 1 declines every level);
      - ncycles_max = 0: ierr 1, all three fail bits, a finite B and both rows of the history; one pass leaves in A what
        the potential entry leaves without a cycle from the same guess - the guess with the face data imposed, and the
        flux-balance fields added - because no solve has looked at the current;
      - after each set a default call on the same handle gives the bits of a fresh handle."""
    import ndsm_amd
    mesh, b, alpha0 = case(kind, shape)
    L = hip.load_library()
    guess = 0.01 * np.cos(abc(mesh))
    keep = np.arange(16) != L.get_ropt_tim()
    F = ndsm_amd.VecPot(*mesh)
    try:
        fresh = F.force_free(b, alpha0, start="given", niter_max=2)
    finally:
        F.close()
    assert fresh[0] == 0
    assert len(OPTION_SETS) < 20
    V = ndsm_amd.VecPot(*mesh)
    try:
        for kw in OPTION_SETS:
            what = "%s %s %s" % (kind, shape, kw)
            fields, ak, alphas, stats, ierrs, iopts = chain_steps(V, b, alpha0, 2, a0=guess, **kw)
            host = V.force_free(b, alpha0, start="given", a_init=guess, niter_max=2, **kw)
            io, ro = V.last_ioptc.copy(), V.last_ropt.copy()
            dev = V.force_free(b, alpha0, start="given", a_init=guess, niter_max=2, device=True, **kw)
            io_d, ro_d = V.last_ioptc.copy(), V.last_ropt.copy()
            assert_same(dev, host, what + ": device entry")
            assert np.array_equal(io, io_d) and ro[keep].tobytes() == ro_d[keep].tobytes(), (what, io, io_d, ro, ro_d)
            ierr, A, B, alpha, status, hist = host
            assert ierr == max(ierrs) and hist.shape == (2, 4), what
            assert_same((A, B, alpha, status), (ak, fields[-1], alphas[-1], stats[-1]), what + ": chain")
            assert_rows(mesh, hist, fields, stats, what)
            want_io, want_ro = iopts[-1][0].copy(), iopts[-1][1]
            want_io[3] = max(ierrs)
            want_io[L.get_iopt_fail3d()] = iopts[0][0][L.get_iopt_fail3d()] | iopts[1][0][L.get_iopt_fail3d()]
            assert np.array_equal(io, want_io), (what, io, want_io)
            assert ro[keep].tobytes() == want_ro[keep].tobytes(), (what, ro, want_ro)
            flipped = V.force_free(b, alpha0, start="given", a_init=guess, niter_max=2,
                                   **dict(kw, mixed_precision=not kw["mixed_precision"]))
            assert_same(flipped, host, what + ": mixed_precision flipped")
            if kw["ncycles_max"] == 0:
                assert ierr == 1 and io[3] == 1 and io[L.get_iopt_fail3d()] == 0b111, what
                assert np.isfinite(B).all() and np.isfinite(hist).all() and np.isfinite(A).all(), what
                one = V.force_free(b, alpha0, start="given", a_init=guess, niter_max=1, **kw)
                pot = V.solve(b, a_init=guess, **kw)
                assert one[0] == 1 and bits_equal(one[1], pot[1]), what
            after = V.force_free(b, alpha0, start="given", niter_max=2)
            assert_same(after, fresh, what + ": the default call afterwards")
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------------
# E. identities of the header
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", (("aniso", (17, 12, 9)), ("uniform", (17, 17, 17))), ids=lambda v: v if isinstance(v, str) else IDS(v))
def test_potential_start_is_the_potential_solve(hip, kind, shape):
    """start = 0: B^0 and A^0 are the bits of the potential solve from a zero guess, and the face phase is that of the
    input.  So the call equals the chain that starts from V.solve(b)'s (B_p, A_p) and keeps the B.n of b: A, B, alpha,
    status bit for bit, and every row of the history is the model's on the chain's fields (row 0 compares B^1 with
    B_p).  That is the whole of the identity: force_free(start="given") on (B_p, a_init=A_p) is a different problem,
    because it takes its B.n from the faces of B_p = curl_h A_p + balance, which meet b's only to the discretisation
    error of curl_h on the faces (the face phase runs from the input, never from an iterate).  Measured on an MI355X,
    max |B_given - B| / max |B| after three passes: 0.29 at 17 x 12 x 9 (aniso), 0.032 at 17^3; the figure is printed,
    and asserted only to be a difference (were it 0 the face phase would have run from an iterate)."""
    import ndsm_amd
    mesh, b, alpha0 = case(kind, shape)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for device in (False, True):
            ierr_p, Ap, Bp = V.solve(b, vc_tol=VC_TOL, device=device)
            got = V.force_free(b, alpha0, start="potential", niter_max=3, step=0.5, vc_tol=VC_TOL, device=device)
            fields, ak, alphas, stats, ierrs, _io = chain_steps(V, b, alpha0, 3, b0=Bp, a0=Ap, vc_tol=VC_TOL)
            what = "%s %s device %s" % (kind, shape, device)
            assert ierr_p == 0 and got[0] == 0 and max(ierrs) == 0, what
            assert_same(got[1:5], (ak, fields[-1], alphas[-1], stats[-1]), what)
            assert_rows(mesh, got[5], fields, stats, what)
            given = V.force_free(Bp, alpha0, start="given", a_init=Ap, niter_max=3, step=0.5, vc_tol=VC_TOL,
                                 device=device)
            scale = np.abs(got[2]).max()
            print(what, "given start on (B_p, A_p): max |dB| / max |B| =", np.abs(given[2] - got[2]).max() / scale,
                  "max |dA| =", np.abs(given[1] - got[1]).max(), "hist", given[5].tolist(), got[5].tolist())
            assert 0.0 < np.abs(given[2] - got[2]).max() < scale, what
    finally:
        V.close()


@pytest.mark.parametrize("kind,shape", (("aniso", (17, 12, 9)), ("uniform", (17, 17, 17))), ids=lambda v: v if isinstance(v, str) else IDS(v))
def test_negative_polarity_through_the_driver(hip, kind, shape):
    """polarity = -1 on the reversed field: alpha0 is taken where B_z < 0 takes the current in, the lines are followed
    along B.  The driver equals the chain with alpha_map(polarity=-1) bit for bit, and lines reach the lower face in
    every pass.  (boundary_alpha of -b has the values of b's, both signs cancel exactly, with -0.0 where b's has +0.0.)"""
    import ndsm_amd
    mesh, b, alpha0p = case(kind, shape)
    alpha0 = ndsm_amd.boundary_alpha(mesh[0], mesh[1], -b, 1e-3)
    assert np.array_equal(alpha0, alpha0p)
    V = ndsm_amd.VecPot(*mesh)
    try:
        fields, ak, alphas, stats, ierrs, _io = chain_steps(V, -b, alpha0, 3, polarity=-1, vc_tol=VC_TOL)
        for device in (False, True):
            what = "%s %s device %s" % (kind, shape, device)
            got = V.force_free(-b, alpha0, polarity=-1, start="given", niter_max=3, step=0.5, vc_tol=VC_TOL,
                               device=device)
            assert got[0] == max(ierrs) == 0, what
            assert_same(got[1:5], (ak, fields[-1], alphas[-1], stats[-1]), what)
            assert_rows(mesh, got[5], fields, stats, what)
            assert np.all(got[5][:, 3] > 0), what
        # with the wrong polarity the lines are followed upwards: fewer of them end on the lower face
        wrong = V.force_free(-b, alpha0, polarity=1, start="given", niter_max=1, step=0.5, vc_tol=VC_TOL)
        assert wrong[5][0, 3] < got[5][0, 3]
    finally:
        V.close()


def test_status_null_and_status_given(hip):
    """status = NULL: the line count of the history comes from a scratch array; A, B, alpha, hist and niter_out are
    those of the call with a status array, host entry, both starts"""
    import ndsm_amd
    mesh, b, alpha0 = case("aniso", (17, 12, 9))
    V = ndsm_amd.VecPot(*mesh)
    L = V.L
    try:
        for start in (0, 1):
            res = {}
            for with_status in (True, False):
                io, ro = V._options(10000, 1024, 1e-13, VC_TOL, 5, False, False, False)
                B, a0 = b.reshape(-1).copy(), alpha0.reshape(-1).copy()
                A, alpha = np.zeros(B.size), np.full(B.size // 3, 7.0)
                status = np.full(B.size // 3, 7, dtype=np.int32)
                hist, niter = np.full((3, 4), np.nan), ctypes.c_int(7)
                rc = L.ndsm_hip_vecpot_nlfff(V.h, io.ctypes.data_as(_ip), ro.ctypes.data_as(_dp), B.ctypes.data,
                                             a0.ctypes.data, 1, start, 3, 0.0, 0.5, V.default_max_steps(0.5),
                                             A.ctypes.data, alpha.ctypes.data,
                                             status.ctypes.data if with_status else None, hist.ctypes.data_as(_dp),
                                             ctypes.byref(niter))
                assert rc == 0 and niter.value == 3
                res[with_status] = (A, B, alpha, hist, io)
                if with_status:
                    assert hist[-1, 3] == (status == ZLO).sum() > 0
            assert_same(res[False], res[True], "start %d" % start)
    finally:
        V.close()


@pytest.mark.parametrize("kind,shape", (("aniso", (17, 12, 9)), ("uniform", (9, 8, 7))), ids=lambda v: v if isinstance(v, str) else IDS(v))
def test_only_the_faces_of_b_are_read(hip, kind, shape):
    """"only its faces are read": with every interior node of b set to NaN (the six faces kept) solve_current and
    force_free(start="potential") give the bits of the clean b, host and device entry"""
    import ndsm_amd
    mesh, b, alpha0 = case(kind, shape)
    J = curl(b, mesh)
    hollow = b.copy()
    hollow[:, 1:-1, 1:-1, 1:-1] = np.nan
    assert np.isnan(hollow).sum() == 3 * (shape[0] - 2) * (shape[1] - 2) * (shape[2] - 2)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for device in (False, True):
            what = "%s %s device %s" % (kind, shape, device)
            clean = V.solve_current(b, J, vc_tol=VC_TOL, device=device)
            got = V.solve_current(hollow, J, vc_tol=VC_TOL, device=device)
            assert clean[0] == 0 and np.isfinite(got[1]).all() and np.isfinite(got[2]).all(), what
            assert_same(got, clean, what + ": solve_current")
            clean = V.force_free(b, alpha0, start="potential", niter_max=2, vc_tol=VC_TOL, device=device)
            got = V.force_free(hollow, alpha0, start="potential", niter_max=2, vc_tol=VC_TOL, device=device)
            assert clean[0] == 0 and np.isfinite(got[2]).all(), what
            assert_same(got, clean, what + ": force_free")
    finally:
        V.close()


# ---------------------------------------------------------------------------------------------------------------------
# F. one handle, many entries
# ---------------------------------------------------------------------------------------------------------------------
def test_entries_share_one_handle(hip):
    """The handle's second field is the other Grad-Rubin iterate and the helicity's B_rec, its first staging array
    holds J, the iteration's B and every line entry's B.  Eight calls on one handle, in the order given and in the
    reverse order: each returns the bits of the same call on a handle of its own."""
    import ndsm_amd
    mesh, b, alpha0 = case("aniso", (17, 12, 9))
    J = curl(b, mesh)
    seeds = np.stack([np.full(5, mesh[0][3]) + 0.01 * np.arange(5), np.full(5, mesh[1][4]), np.full(5, mesh[2][2])],
                     axis=1)

    def flat(r):
        out = []
        for v in r:
            out.extend(flat(v) if isinstance(v, tuple) else [v])
        return out

    calls = [
        ("force_free", lambda V: V.force_free(b, alpha0, niter_max=2, vc_tol=VC_TOL)),
        ("helicity", lambda V: V.helicity(b, vc_tol=VC_TOL, return_fields=True)),
        ("force_free given", lambda V: V.force_free(b, alpha0, start="given", niter_max=3, vc_tol=VC_TOL)),
        ("project", lambda V: V.project(b + 0.05 * abc(mesh, k=1.7), vc_tol=VC_TOL, return_phi=True)),
        ("trace", lambda V: V.trace(b, seeds, g=0.3 * abc(mesh))),
        ("solve_current", lambda V: V.solve_current(b, J, vc_tol=VC_TOL)),
        ("helicity devore", lambda V: V.helicity(b, gauge="devore", vc_tol=VC_TOL, return_fields=True)),
        ("force_free device", lambda V: V.force_free(b, alpha0, niter_max=2, vc_tol=VC_TOL, device=True)),
    ]
    want = {}
    for name, run in calls:
        V = ndsm_amd.VecPot(*mesh)
        try:
            want[name] = flat(run(V))
        finally:
            V.close()
    for order in (calls, calls[::-1]):
        V = ndsm_amd.VecPot(*mesh)
        try:
            for name, run in order:
                assert_same(flat(run(V)), want[name], "%s after %s" % (name, [n for n, _ in order]))
        finally:
            V.close()
