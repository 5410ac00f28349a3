"""The planner's answer for a relax call whose source is a zero first guess that was never written
(csrc/relax_plan.hpp, Request::src_zero), read through ndsm_hip_debug_relax_plan(what = 2) on a machine without a GPU:
the launches are those of the same request on an array of zeros; the FIRST pass is marked `src_zero` where it is an
out-of-place fused pass of a whole fp64 level in mode plain or + residual, otherwise the plan says the zeros have to
be written first (`materialise`).  The schedules are literals ("Which launch a relax call makes")."""
import ctypes

import numpy as np

import plan_tools as pt
from ndsm_amd import _lib

_ip = ctypes.POINTER(ctypes.c_int)
_i64 = ctypes.POINTER(ctypes.c_int64)

F2, F2L1, F2S = "F2 136x30/1024", "F2 136x30/1024 L1", "F2 72x28/512"
F1, F1B, F1R = "F1 132x23/768", "F1 132x31/1024", "F1R 136x22/768"


def zplan(n, nsweeps, src_zero=True, all_neumann=False, zown=None, k0=0, nzg=None, variant=0, window=False, fp32=False,
          rhs=True, want_res=False, want_met=False, corr=False, nbufs=2, keep=-1, no_block=False):
    """(materialise, schedule, head) of the request: schedule = one string per pass, the instantiation / launch as
    test_relax_plan.py writes it, ' odd' for the odd-nx instantiation and ' Z' where the pass takes a zero source"""
    L = _lib.load_library()
    n = list(n) + [1] * (3 - len(n))
    ndim = 3 if n[2] > 1 else 2
    zown = zown if zown is not None else (0, n[2])
    grid = np.array([ndim] + n + [0, 0, 0] + [m - 1 for m in n] +
                    [int(all_neumann), k0, n[2] if nzg is None else nzg, zown[0], zown[1]], dtype=np.intc)
    req = np.array([nsweeps, variant, window, fp32, rhs, want_res, want_met, corr, 0, nbufs >= 2, nbufs >= 3, keep,
                    src_zero], dtype=np.int64)
    knobs = np.array([0, 0, 0, 0, -1, 0, 0, int(no_block)], dtype=np.int64)
    cap = 7 + 10 * max(nsweeps, 1)
    out = np.zeros(cap, dtype=np.intc)
    rc = L.ndsm_hip_debug_relax_plan(2, grid.ctypes.data_as(_ip), req.ctypes.data_as(_i64), knobs.ctypes.data_as(_i64),
                                     cap, out.ctypes.data_as(_ip))
    _lib._check(rc, "debug_relax_plan", L)
    rows = out[7:7 + 10 * out[1]].reshape(-1, 10)
    got = []
    for r in rows:
        kind = pt.PLAN_KINDS[r[0]]
        t = {"fused": pt.PLAN_INSTS[r[3] & 15], "block": "B%d/%d" % (r[1], r[4])}.get(kind, kind)
        got.append(t + (" odd" if r[3] & 16 else "") + (" Z" if r[9] else ""))
    return bool(out[6]), got, [int(v) for v in out[:6]]


def test_fused_levels_take_the_zero_source():
    # level 2 of the 512^3 hierarchy: five sweeps + residual on a level with a right-hand side
    assert zplan((256, 256, 256), 5, want_res=True) == (False, [F2 + " Z", F2, F1R], [0, 3, 1, 1, 0, 0])
    # level 3: exactly 2 Mi points, the 72 x 28 tile
    assert zplan((128, 128, 128), 5, want_res=True) == (False, [F2S + " Z", F2S, F1R], [0, 3, 1, 1, 0, 0])
    # odd nx (every other level of a floor-halving hierarchy)
    assert zplan((257, 256, 256), 5)[:2] == (False, [F2 + " odd Z", F2 + " odd", F1 + " odd"])
    assert zplan((129, 130, 130), 5, want_res=True)[:2] == (False, [F2 + " odd Z", F2 + " odd", F1R + " odd"])
    # one-sweep first passes: plain, and the sweep + residual launch
    assert zplan((256, 256, 256), 1)[:2] == (False, [F1 + " Z"])
    assert zplan((256, 256, 256), 1, want_res=True)[:2] == (False, [F1R + " Z"])
    assert zplan((512, 512, 512), 5, rhs=False)[:2] == (False, [F2L1 + " Z", F2L1, F1B])
    # the forced fused pass of the tests, at the smallest shapes it accepts
    assert zplan((16, 16, 8), 2, variant=2)[:2] == (False, [F2S + " Z"])
    assert zplan((17, 16, 9), 1, variant=2, want_res=True)[:2] == (False, [F1R + " odd Z"])
    # the tracked form's three buffers: the first pass still reads buffer 0 only
    assert zplan((512, 512, 512), 5, want_res=True, nbufs=3, keep=1)[:2] == (False, [F2L1 + " Z", F2L1, F1R])


def test_everything_else_materialises():
    assert zplan((64, 64, 64), 5) == (True, ["B2/8", "B2/8", "B1/8"], [0, 3, 1, 0, 0, 0])        # block-resident
    assert zplan((96, 96, 96), 5) == (True, ["color3d"] * 5, [0, 5, 0, 0, 0, 0])                  # colour passes
    assert zplan((16, 16, 16), 5)[:2] == (True, ["small3d"])
    assert zplan((128, 128), 5)[:2] == (True, ["medium2d"])
    assert zplan((256, 256, 256), 2, all_neumann=True)[:2] == (True, [F1, F1])                    # mean shift in between
    assert zplan((256, 256, 256), 5, variant=1)[:2] == (True, ["color3d"] * 5)
    assert zplan((256, 256, 256), 5, nbufs=1)[:2] == (True, ["color3d"] * 5)
    assert zplan((512, 512, 512), 5, want_res=True, fp32=True)[:2] == (True, [F2L1, F2L1, F1R])   # fp32: out of scope
    assert zplan((64, 64, 40), 2, zown=(4, 36), nzg=128, k0=10, window=True)[:2] == (True, [F2])  # windows / slabs
    assert zplan((64, 64, 40), 5, zown=(4, 36), nzg=128, k0=10)[1][0] == F2                        # a slab, no window
    assert zplan((64, 64, 40), 5, zown=(4, 36), nzg=128, k0=10)[0]
    assert zplan((512, 512, 512), 5, rhs=False, corr=True, nbufs=3, keep=1)[0]                    # correction pending
    assert zplan((256, 256, 256), 0) == (True, [], [0, 0, 0, 0, 0, 0])                            # no pass at all
    assert zplan((256, 256, 256), 1, want_met=True, nbufs=3, keep=1)[:2] == (True, ["F1M 132x23/768"])
    assert zplan((64, 64, 64), 5, no_block=True)[:2] == (True, ["color3d"] * 5)


def test_without_the_flag_nothing_changes():
    """the same requests without the flag: today's literals, no mark, nothing to materialise - and the what = 0
    layout still answers as it did"""
    assert zplan((256, 256, 256), 5, src_zero=False, want_res=True) == (False, [F2, F2, F1R], [0, 3, 1, 1, 0, 0])
    assert zplan((128, 128, 128), 5, src_zero=False, want_res=True) == (False, [F2S, F2S, F1R], [0, 3, 1, 1, 0, 0])
    assert zplan((257, 256, 256), 5, src_zero=False)[:2] == (False, [F2 + " odd", F2 + " odd", F1 + " odd"])
    assert zplan((64, 64, 64), 5, src_zero=False) == (False, ["B2/8", "B2/8", "B1/8"], [0, 3, 1, 0, 0, 0])
    assert zplan((96, 96, 96), 5, src_zero=False) == (False, ["color3d"] * 5, [0, 5, 0, 0, 0, 0])
    assert zplan((256, 256, 256), 2, src_zero=False, all_neumann=True)[:2] == (False, [F1, F1])
    for kw in (dict(n=(256, 256, 256), nsweeps=5, want_res=True), dict(n=(257, 256, 256), nsweeps=5),
               dict(n=(64, 64, 64), nsweeps=5), dict(n=(96, 96, 96), nsweeps=5), dict(n=(16, 16, 8), nsweeps=2, variant=2),
               dict(n=(256, 256, 256), nsweeps=2, all_neumann=True, want_res=True)):
        old = pt.relax_plan(**kw)
        for z in (False, True):       # the flag changes no launch
            mat, got, head = zplan(src_zero=z, **kw)
            assert head == [old["err"], len(old["passes"]), old["result"], old["res_done"], old["met_done"],
                            old["prolong_only"]], kw
            want = [{"fused": q["inst"], "block": "B%d/%d" % (q["sweeps"], q["bz"])}.get(q["kind"], q["kind"]) +
                    (" odd" if q["odd_nx"] else "") for q in old["passes"]]
            assert [t.replace(" Z", "") for t in got] == want, kw
            assert z or (not mat and not any(t.endswith(" Z") for t in got)), kw
