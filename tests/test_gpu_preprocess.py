"""GPU tests of the magnetogram preprocessing (csrc/preprocess.hip, vecpot_preprocess) against its numpy model
(tests/preprocess_model.py), bit for bit: the field as uint64, every history row, info.  The model restates the
kernels' expressions and the reduction's partition; nothing here is taken from the device code's results."""
import ctypes

import numpy as np
import pytest

import preprocess_model as M
from device_arena import Arena, LibTransport, slot
from golden_inputs import aniso_mesh, uniform_mesh

pytestmark = pytest.mark.gpu

IDS = lambda s: "x".join(map(str, s))   # noqa: E731
FILL = 7
NZ = 4      # the handle's third axis: the call never looks at it

# nx x ny.  A handle takes no axis under four points, so the planes of 3 x 3, 3 x 4, 4 x 3 and 257 x 3 nodes exist for
# the model alone (tests/test_preprocess_model.py); here 4x4: 2 x 2 interior nodes, every Lambda neighbour of theirs an
# edge node or one another; 4x5, 5x4, 5x7: one axis longer; 33x22: the suite's anisotropic plane; 257x4 and 513x4: a
# thread walks 2 and 3 points of a row; 65x9: one more than the update block on x and y; 4x2049: a block walks two rows
# and the final fold takes more than 256 partials
SHAPES = ([4, 4], [4, 5], [5, 4], [5, 7], [33, 22], [257, 4], [513, 4], [65, 9], [4, 2049])
CASES = [("uniform", s) for s in SHAPES] + [("aniso", [33, 22]), ("aniso", [5, 7])]
MESHES = {"uniform": uniform_mesh, "aniso": aniso_mesh}
MUS = {"default": M.MU, "mu2 alone": (0.0, 1.0, 0.0, 0.0, 0.0), "mu4 = 0": (1.0, 1.0, 1e-3, 1e-2, 0.0)}


@pytest.fixture(scope="module")
def hip():
    import ndsm_amd
    from ndsm_amd import _lib
    L = ndsm_amd.load_library()
    rc = L.ndsm_hip_init(-1)
    assert rc == 0, _lib.last_error(L)
    return _lib


def mesh_of(mname, ns):
    return MESHES[mname](list(ns) + [NZ])


def same(got, want, what):
    """(B, hist, info) of the device against the model's, bit for bit"""
    gB, gh, gi = got
    wB, wh, wi = want
    assert gi == wi, (what, gi, wi, gh, wh)
    assert gh.shape == wh.shape and gh.tobytes() == wh.tobytes(), (what, gh, wh)
    assert gB.shape == wB.shape, what
    bad = gB.view(np.uint64) != wB.view(np.uint64)
    assert not bad.any(), (what, int(bad.sum()), float(np.abs(gB - wB).max()))


@pytest.mark.parametrize("mname,ns", CASES, ids=[m + "-" + IDS(s) for m, s in CASES])
def test_driver_equals_the_model(hip, mname, ns):
    """after 1, 2 and 7 tries, with the default mu, with the torque term alone and without the smoothing term: the
    field, the history and info of the host entry are the model's; 1 and 2 accepted tries leave the current field in
    either buffer.  Two calls give the same bits, and so does another check interval"""
    import ndsm_amd
    mesh = mesh_of(mname, ns)
    b = M.test_magnetogram(mesh)
    V = ndsm_amd.VecPot(*mesh)
    try:
        parities = set()
        # (the model's sums over 2049 rows take a while: that plane runs with the default mu alone)
        for kind, mu in list(MUS.items())[:1 if ns[1] > 2048 else None]:
            for n in (1, 2, 7):
                what = "%s %s %s, %d tries" % (mname, ns, kind, n)
                wB, wh, wi, _ = M.run(mesh, b, mu=mu, niter_max=n, check=1, tol=0.0)
                ierr, B, hist, info = V.preprocess(b, mu=mu, niter_max=n, check=1, tol=0.0)
                assert ierr == 0, what
                same((B, hist, info), (wB, wh, wi), what)
                assert info == (n + 1, n, 0) and np.isfinite(hist).all() and hist[-1, 1] < hist[0, 1], (what, hist)
                parities.add(int(hist[-1, 8]) % 2)
                if n == 7:
                    again = V.preprocess(b, mu=mu, niter_max=n, check=1, tol=0.0)
                    same(again[1:], (B, hist, info), what + ", second call")
                    _, B3, hist3, info3 = V.preprocess(b, mu=mu, niter_max=n, check=3, tol=0.0)
                    w3 = M.run(mesh, b, mu=mu, niter_max=n, check=3, tol=0.0)
                    same((B3, hist3, info3), w3[:3], what + ", check 3")
                    assert info3 == (4, 7, 0) and np.array_equal(B3.view(np.uint64), B.view(np.uint64)), what
                    assert hist3[-1].tobytes() == hist[-1].tobytes()
        assert parities == {0, 1}
    finally:
        V.close()


@pytest.mark.parametrize("mname,ns", [("uniform", [5, 7]), ("aniso", [33, 22]), ("uniform", [513, 4])],
                         ids=["uniform-5x7", "aniso-33x22", "uniform-513x4"])
def test_rejections_stop_rules_observation_and_continuation(hip, mname, ns):
    """a first step 64 times too large: the first tries are rejected and write the same trial buffer again, later ones
    are accepted and flip the index; an overflowing step; the three stop rules and a history that runs out of rows; an
    observation of its own; a continued call"""
    import ndsm_amd
    mesh = mesh_of(mname, ns)
    b = M.test_magnetogram(mesh)
    V = ndsm_amd.VecPot(*mesh)
    try:
        for kw in (dict(niter_max=12, check=12, tol=0.0, dt0=0.64),                     # rejected, then accepted
                   dict(niter_max=11, check=4, tol=0.0, dt0=0.03, hist_rows=3),         # rows run out; a short tail
                   dict(niter_max=50, check=5, tol=0.999),                              # tol at the first check
                   dict(niter_max=50, check=5, dt0=100.0, dt_min=60.0),                 # dt_min after one rejection
                   dict(niter_max=50, check=5, dt0=1.0, dt_min=2.0),                    # dt_min before any try
                   dict(niter_max=40, check=40, tol=0.0, dt0=1e300),                    # overflow: inf and NaN in L_T
                   dict(niter_max=1, check=1, tol=0.0, mu=(0, 0, 0, 0, 0))):            # L = 0: a rejection
            what = "%s %s %s" % (mname, ns, kw)
            want = M.run(mesh, b, **kw)
            ierr, B, hist, info = V.preprocess(b, **kw)
            assert ierr == 0
            same((B, hist, info), want[:3], what)
        _, B, hist, info = V.preprocess(b, niter_max=12, check=12, tol=0.0, dt0=0.64)
        assert info == (2, 12, 0) and 0 < hist[1, 8] < 12, hist                     # both rejections and acceptances
        _, B, hist, info = V.preprocess(b, niter_max=50, check=5, dt0=100.0, dt_min=60.0)
        assert info == (2, 1, 2) and np.array_equal(B.view(np.uint64), b.view(np.uint64))
        _, B, hist, info = V.preprocess(b, niter_max=50, check=5, tol=0.999)
        assert info == (2, 5, 1)
        _, B, hist, info = V.preprocess(b, niter_max=40, check=40, tol=0.0, dt0=1e300)      # dt_min in mid-interval
        assert info == (2, 20, 2) and hist[-1, 8] == 0.0 and np.array_equal(B.view(np.uint64), b.view(np.uint64))
        _, B, hist, info = V.preprocess(b, niter_max=1, check=1, tol=0.0, mu=(0, 0, 0, 0, 0))
        assert hist[0, 1] == 0.0 and list(hist[1, [0, 1, 8]]) == [1.0, 0.0, 0.0]
        # obs given = obs None on the same data; an observation that differs from the start
        full = V.preprocess(b, niter_max=7, check=7, tol=0.0)
        same(V.preprocess(b, obs=b.copy(), niter_max=7, check=7, tol=0.0)[1:], full[1:], "obs = b")
        other = b + 0.01 * np.cos(np.arange(b.size, dtype=np.float64)).reshape(b.shape)
        for device in (False, True):
            got = V.preprocess(other, obs=b, niter_max=3, check=2, tol=0.0, device=device)
            same(got[1:], M.run(mesh, other, obs=b, niter_max=3, check=2, tol=0.0)[:3], "obs differs, device %s" % device)
            assert got[2][0, 4] > 0.0 and got[2][0, 5] > 0.0
        # continuation: 3 tries, then 4 more against the original from the first call's last dt = one call of 7
        _, B3, hist3, _ = V.preprocess(b, niter_max=3, check=3, tol=0.0)
        _, B4, hist4, _ = V.preprocess(B3, obs=b, niter_max=4, check=4, tol=0.0, dt0=hist3[-1, 7])
        assert np.array_equal(B4.view(np.uint64), full[1].view(np.uint64))
        assert hist4[-1, 1:8].tobytes() == full[2][-1, 1:8].tobytes()
    finally:
        V.close()


@pytest.mark.parametrize("mname,ns", [("uniform", [4, 4]), ("aniso", [5, 7]), ("aniso", [33, 22])],
                         ids=["uniform-4x4", "aniso-5x7", "aniso-33x22"])
def test_host_entry_device_entry_and_offset_arrays(hip, mname, ns):
    """ndsm_hip_vecpot_preprocess = ndsm_hip_vecpot_preprocess_device on arrays of their own = the same on views into
    one larger allocation (8 mod 16, NaN bands beside B and obs): B comes out, obs is read only, nothing else changes;
    2 and 3 tries, so that the result is copied into the caller's array once and lies there once"""
    import ndsm_amd
    mesh = mesh_of(mname, ns)
    b = M.test_magnetogram(mesh)
    start = b + 0.01 * np.sin(np.arange(b.size, dtype=np.float64)).reshape(b.shape)
    V = ndsm_amd.VecPot(*mesh)
    L = V.L
    mu = np.array(M.MU, dtype=np.float64)
    try:
        for obs in (None, b):
            for n in (2, 3):
                args = (n, 2, 0.0, 0.02, 1e-9)
                want = M.run(mesh, start, obs=obs, niter_max=n, check=2, tol=0.0, dt0=0.02, dt_min=1e-9, hist_rows=4)
                B = start.reshape(-1).copy()
                O = None if obs is None else obs.reshape(-1).copy()
                hist, info = np.full((4, 17), np.nan), np.full(3, FILL, dtype=np.intc)
                rc = L.ndsm_hip_vecpot_preprocess(V.h, B.ctypes.data, None if O is None else O.ctypes.data,
                                                  mu.ctypes.data, *args, hist.ctypes.data, 4, info.ctypes.data)
                assert rc == 0, hip.last_error(L)
                assert O is None or np.array_equal(O, obs.reshape(-1))
                rows = int(info[0])
                assert rows == want[2][0] < 4 and np.isnan(hist[rows:]).all()      # rows past the ones written are left alone
                same((B.reshape(b.shape), hist[:rows], tuple(int(v) for v in info)), want[:3], "host entry")
                for plain in (False, True):
                    slots = [slot("B", start.reshape(-1), output=True, field=True)]
                    if obs is not None:
                        slots.append(slot("obs", obs.reshape(-1), field=True))
                    hist_d, info_d = np.full((4, 17), np.nan), np.full(3, FILL, dtype=np.intc)
                    R = Arena(LibTransport(L), slots, plain=plain)
                    got = R.run(lambda dB, dO=None: L.ndsm_hip_vecpot_preprocess_device(
                        V.h, dB, dO, mu.ctypes.data, *args, hist_d.ctypes.data, 4, info_d.ctypes.data))
                    what = "%s %s obs %s %d tries plain %s" % (mname, ns, obs is not None, n, plain)
                    assert R.rc == 0, (what, hip.last_error(L))
                    assert np.array_equal(got[0].view(np.uint64), B.view(np.uint64)), what
                    assert hist_d.tobytes() == hist.tobytes() and info_d.tobytes() == info.tobytes(), what
    finally:
        V.close()


def test_argument_errors_of_the_c_entries(hip):
    import ndsm_amd
    mesh = mesh_of("uniform", [5, 7])
    b = M.test_magnetogram(mesh)
    V = ndsm_amd.VecPot(*mesh)
    L = V.L
    nan, inf = float("nan"), float("inf")
    good = np.array(M.MU, dtype=np.float64)
    try:
        dB = ctypes.c_void_p()
        assert L.ndsm_hip_device_alloc(b.nbytes, ctypes.byref(dB)) == 0
        try:
            for name, host in (("ndsm_hip_vecpot_preprocess", True), ("ndsm_hip_vecpot_preprocess_device", False)):
                fn = getattr(L, name)

                def call(h=V.h, field=b, B=True, mu=good, args=(3, 1, 0.0, 1e-2, 0.0), rows=4, hist=True, info=True):
                    """(rc, hist, info, B after the call)"""
                    src = np.ascontiguousarray(field).copy()
                    assert L.ndsm_hip_memcpy_h2d(dB, src.ctypes.data, src.nbytes) == 0
                    hh, ii = np.full((4, 17), nan), np.full(3, FILL, dtype=np.intc)
                    pB = None if not B else (ctypes.c_void_p(src.ctypes.data) if host else dB)
                    rc = fn(h, pB, None, None if mu is None else mu.ctypes.data, *args,
                            hh.ctypes.data if hist else None, rows, ii.ctypes.data if info else None)
                    if not host:
                        assert L.ndsm_hip_memcpy_d2h(src.ctypes.data, dB, src.nbytes) == 0
                    return rc, hh, ii, src
                rc, hh, ii, out = call()
                assert rc == 0 and tuple(ii) == (4, 3, 0) and np.isfinite(hh).all() and not np.array_equal(out, b)
                for args in ((0, 1, 0.0, 1e-2, 0.0), (3, 0, 0.0, 1e-2, 0.0), (3, 1, -1e-9, 1e-2, 0.0),
                             (3, 1, nan, 1e-2, 0.0), (3, 1, inf, 1e-2, 0.0), (3, 1, 0.0, 0.0, 0.0),
                             (3, 1, 0.0, -1.0, 0.0), (3, 1, 0.0, inf, 0.0), (3, 1, 0.0, nan, 0.0),
                             (3, 1, 0.0, 1e-2, -1.0), (3, 1, 0.0, 1e-2, nan), (3, 1, 0.0, 1e-2, inf)):
                    rc, hh, ii, out = call(args=args)
                    assert rc == 9004 and not ii.any() and not hh.any() and np.array_equal(out, b), (name, args, rc)
                for k in range(5):
                    for v in (-1e-300, nan, inf, -inf):
                        bad = good.copy()
                        bad[k] = v
                        rc, hh, ii, out = call(mu=bad)
                        assert rc == 9004 and not ii.any() and not hh.any() and np.array_equal(out, b), (name, k, v)
                rc, hh, ii, out = call(rows=1)
                assert rc == 9004 and not ii.any() and not hh[0].any() and np.isnan(hh[1:]).all()
                # a zero observation: E = M = 0
                rc, hh, ii, out = call(field=np.zeros_like(b))
                assert rc == 9004 and not ii.any() and not hh.any() and not out.any(), (name, rc)
                assert call(h=None)[0] == 9002 and call(B=False)[0] == 9002 and call(mu=None)[0] == 9002
                assert call(hist=False)[0] == 9002 and call(info=False)[0] == 9002
        finally:
            L.ndsm_hip_device_free(dB)
    finally:
        V.close()


def test_other_entries_of_the_handle_are_untouched(hip):
    """solve(), optimize() and helicity() give the same bits before and after a preprocess() on one handle"""
    import ndsm_amd
    import optimize_model as OM
    mesh = uniform_mesh([12, 10, 9])
    b = OM.perturbed_abc(mesh)[1]
    bm = M.test_magnetogram(mesh)
    V = ndsm_amd.VecPot(*mesh)

    def others():
        s = V.solve(b)
        o = V.optimize(b, start="given", niter_max=3, check=2)
        h = V.helicity(b)
        return ([np.asarray(v) for v in s] + [np.asarray(v) for v in o[:3]] +
                [np.asarray(v, dtype=np.float64) for v in h[:10]])
    try:
        before = others()
        for device in (False, True):
            V.preprocess(bm, niter_max=3, check=2, device=device)
            after = others()
            assert len(before) == len(after)
            for x, y in zip(before, after):
                assert x.shape == y.shape and x.tobytes() == y.tobytes()
    finally:
        V.close()


# The end-to-end property on 17 x 17 x 9, measured with the CPU models alone (preprocess_model, then optimize_model from
# the CPU oracle's potential field with the face put over it; 400 tries at most, tol = 0, dt_min = 0): the raw test
# magnetogram ends at L_f = 0.1192 after 400 tries, the preprocessed one (2000 tries, the defaults: L 2.90e-2 ->
# 8.8e-4) stalls at L_f = 0.0719 after 232 tries - every later try is rejected, and the check at 300 stops the loop.
# A factor of 1.66; the face is all the two runs differ in
E2E_FACTOR = 1.66


def test_preprocessed_face_relaxes_further(hip):
    """L_f at the end of optimize(start="potential", niter_max=400) is lower with the preprocessed magnetogram on the
    lower face than with the raw one, by at least a quarter of the factor the CPU models give"""
    import ndsm_amd
    mesh = uniform_mesh([17, 17, 9])
    bm = M.test_magnetogram(mesh)
    V = ndsm_amd.VecPot(*mesh)
    try:
        ierr, pm, hist, info = V.preprocess(bm, niter_max=2000, check=50, tol=0.0)
        assert ierr == 0 and info == (41, 2000, 0)
        final = []
        for face in (bm, pm):
            b = np.zeros((3,) + tuple(len(q) for q in mesh[::-1]))
            b[:, 0] = face
            _, B, oh, oi = V.optimize(b, start="potential", niter_max=400, check=50, tol=0.0, dt_min=0.0)
            assert np.array_equal(B[:, 0], face)
            final.append(float(oh[-1, 2]))
        print("L_f raw", final[0], "preprocessed", final[1], "factor", final[0] / final[1])
        assert final[1] < final[0]
        assert final[0] / final[1] >= E2E_FACTOR / 4.0
    finally:
        V.close()
