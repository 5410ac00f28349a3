"""Which launches a relax call makes (csrc/relax_plan.hpp), read through ndsm_hip_debug_relax_plan on a machine
without a GPU.  The schedules below are literals taken from DESIGN.md, "Which launch a relax call makes" - a change
that sends a level to another launch gives the same bits and passes every parity test, but not these."""
import random

import pytest

import plan_tools as _lib


def sched(**kw):
    """the plan as a list of short strings: 'F2 136x30/1024 L1', 'B2/8', 'color3d', 'small3d x5', with ' odd',
    'prol+' (stand-alone interpolation first) and '+shift' (mean shift after) where they apply"""
    p = _lib.relax_plan(**kw)
    out = []
    for q in p["passes"]:
        t = {"fused": q["inst"], "block": "B%d/%d" % (q["sweeps"], q["bz"])}.get(q["kind"], q["kind"])
        if q["kind"] in ("small3d", "small2d", "medium2d"):
            t += " x%d" % q["sweeps"]
        t = ("prol+" if q["prolong_first"] else "") + t + (" odd" if q["odd_nx"] else "") + ("+shift" if q["mean_shift"] else "")
        out.append(t)
    return p, out


F2, F2L1, F2S, F2N = "F2 136x30/1024", "F2 136x30/1024 L1", "F2 72x28/512", "F2 136x22/768"
F1, F1B, F1R = "F1 132x23/768", "F1 132x31/1024", "F1R 136x22/768"


@pytest.mark.parametrize("n,want", [
    ((512, 512, 512), [F2L1, F2L1, F1B]),
    ((256, 256, 256), [F2, F2, F1]),
    ((128, 128, 128), [F2S, F2S, F1]),            # exactly 2 Mi points: fused; below 6 M: the small tile
    ((257, 256, 256), [F2 + " odd", F2 + " odd", F1 + " odd"]),
    ((96, 96, 96), ["color3d"] * 5),              # above the block window, below the fused threshold
    ((64, 64, 64), ["B2/8", "B2/8", "B1/8"]),
    ((32, 32, 32), ["B2/4", "B2/4", "B1/4"]),     # 32 < 64 workgroups of full height
    ((17, 16, 16), ["B2/4", "B2/4", "B1/4"]),     # smallest level above 4096 points
    ((16, 16, 16), ["small3d x5"]),
])
def test_whole_levels_five_sweeps(n, want):
    p, got = sched(n=n, nsweeps=5)
    assert p["err"] == 0 and got == want
    assert not p["res_done"] and not p["met_done"]
    # out-of-place passes ping-pong between the two buffers; in-place ones stay in buffer 0
    assert p["result"] == (len(want) % 2 if want[0][0] in "FB" else 0)


def test_variations():
    assert sched(n=(16, 16, 16), nsweeps=5, all_neumann=True)[1] == ["color3d+shift"] * 5
    assert sched(n=(64, 64), nsweeps=5)[1] == ["small2d x5"]
    assert sched(n=(64, 64), nsweeps=5, all_neumann=True)[1] == ["small2d x5"]      # the kernel shifts the mean itself
    assert sched(n=(128, 128), nsweeps=5)[1] == ["medium2d x5"]
    assert sched(n=(140, 140), nsweeps=5)[1] == ["color2d"] * 5                     # above kMed2D = 19456 points
    p, got = sched(n=(256, 256, 256), nsweeps=2, all_neumann=True, want_res=True)
    assert got == [F1 + "+shift"] * 2 and not p["res_done"] and p["result"] == 0
    assert sched(n=(256, 256, 256), nsweeps=5, variant=1)[1] == ["color3d"] * 5
    assert sched(n=(256, 256, 256), nsweeps=5, nbufs=1)[1] == ["color3d"] * 5
    assert sched(n=(16, 16, 8), nsweeps=2, variant=2)[1] == [F2S]
    assert sched(n=(15, 16, 8), nsweeps=2, variant=2)[0]["err"] == 9002
    assert sched(n=(64, 64, 64), nsweeps=5, no_block=True)[1] == ["color3d"] * 5
    p, got = sched(n=(16, 16, 16), nsweeps=0, corr=True)
    assert got == [] and p["prolong_only"]


def test_level1_tracked_form():
    """three buffers, buffer 1 is `keep`: the out-of-place passes alternate between buffers 0 and 2"""
    t = dict(n=(512, 512, 512), nbufs=3, keep=1)
    p, got = sched(nsweeps=5, want_res=True, **t)
    assert got == [F2L1, F2L1, F1R] and p["res_done"] and p["result"] == 2
    p, got = sched(nsweeps=4, want_res=True, **t)
    assert got == [F2L1, F1B, F1R] and p["res_done"]
    p, got = sched(nsweeps=5, rhs=False, corr=True, want_met=True, **t)
    assert got == ["F1P 132x31/1024", F2L1, "F2M 136x30/1024"] and p["met_done"]
    p, got = sched(nsweeps=4, rhs=False, corr=True, want_met=True, **t)
    assert got == ["F2P 136x30/1024", "F2M 136x30/1024"] and p["met_done"] and p["result"] == 0
    p, got = sched(nsweeps=4, rhs=True, corr=True, **t)
    assert got == ["prol+" + F2L1, F2L1]
    # two sweeps: the correction launch takes both, so no launch is left to carry the metric
    p, got = sched(nsweeps=2, rhs=False, corr=True, want_met=True, **t)
    assert got == ["F2P 136x30/1024"] and not p["met_done"]
    p, got = sched(nsweeps=1, want_met=True, **t)
    assert got == ["F1M 132x31/1024"] and p["met_done"]
    p, got = sched(nsweeps=1, want_met=True, n=(256, 256, 256), nbufs=3, keep=1)       # below 64 M points
    assert got == ["F1M 132x23/768"] and p["met_done"]
    p, got = sched(nsweeps=1, want_met=True, want_res=True, **t)
    assert got == [F1R] and p["res_done"] and not p["met_done"]
    # a coarse plane of 2 GiB or a transfer that does not describe the level: stand-alone interpolation
    assert sched(nsweeps=5, rhs=False, corr=True, coarse_plane=1 << 28, **t)[1] == ["prol+" + F2L1, F2L1, F1B]
    assert sched(nsweeps=5, rhs=False, corr=True, coarse_plane=-1, **t)[1] == ["prol+" + F2L1, F2L1, F1B]
    # an in-place pass on `keep` is an error
    assert sched(n=(96, 96, 96), nsweeps=1, nbufs=3, keep=0)[0]["err"] == 9002
    assert sched(n=(16, 16, 16), nsweeps=1, nbufs=3, keep=0)[0]["err"] == 9002
    assert sched(n=(96, 96, 96), nsweeps=1, nbufs=3, keep=1)[0]["err"] == 0


def window(ghosts, **kw):
    return sched(n=(64, 64, 32 + 2 * ghosts), zown=(ghosts, ghosts + 32), nzg=128, k0=10, window=True, **kw)


def test_slab_windows():
    assert window(4, nsweeps=2)[1] == [F2]
    assert window(6, nsweeps=2)[1] == [F2]
    assert window(3, nsweeps=2)[0]["err"] == 9002                 # two sweeps consume 4 ghost planes
    p, got = window(3, nsweeps=1, want_res=True)
    assert got == [F1R] and p["res_done"]
    assert window(2, nsweeps=1, want_res=True)[0]["err"] == 9002    # the residual stage a third one
    for rhs in (True, False):
        for gh in (2, 3, 4):
            assert window(gh, nsweeps=1, corr=True, rhs=rhs)[1] == ["F1P 132x31/1024"]
    assert window(4, nsweeps=2, corr=True, rhs=False)[1] == ["F2P 136x30/1024"]
    assert window(4, nsweeps=2, corr=True, rhs=True)[0]["err"] == 9002           # prolong_ok: false
    assert window(4, nsweeps=1, want_met=True)[1] == ["F1M 132x23/768"]
    assert window(4, nsweeps=2, want_met=True)[1] == ["F2M 136x30/1024"]
    assert window(4, nsweeps=1, want_met=True, all_neumann=True)[0]["err"] == 9002   # metric_ok: false
    assert window(4, nsweeps=1, corr=True, all_neumann=True)[0]["err"] == 9002       # prolong_ok: false
    assert window(4, nsweeps=2, all_neumann=True)[1] == [F2]                         # the driver shifts the mean


def test_fp32():
    p, got = sched(n=(512, 512, 512), nsweeps=5, want_res=True, fp32=True)
    assert got == [F2L1, F2L1, F1R] and p["res_done"] and p["result"] == 1
    for kw in (dict(want_met=True), dict(corr=True, rhs=False)):
        for ns in (1, 2, 5):
            p = _lib.relax_plan(n=(512, 512, 512), nsweeps=ns, fp32=True, **kw)
            assert [q["mode"] for q in p["passes"]] == [""] * len(p["passes"]) and not p["met_done"]
    assert sched(n=(96, 96, 96), nsweeps=1, fp32=True)[0]["err"] == 9002         # fused or nothing
    assert sched(n=(257, 256, 256), nsweeps=1, fp32=True)[0]["err"] == 9002      # no odd-nx instantiation in fp32


def test_knobs():
    # big = 1: the large-level one-sweep tile; the two-sweep pass of a level below 6 M points keeps the small tile
    assert sched(n=(64, 64, 64), nsweeps=5, variant=2, fused_cfg=(0, 0, 0, 0, 1))[1] == [F2S, F2S, F1B]
    assert sched(n=(64, 64, 64), nsweeps=5, variant=2)[1] == [F2S, F2S, F1]
    assert sched(n=(256, 256, 256), nsweeps=5, fused_cfg=(0, 0, 0, 0, 1))[1] == [F2L1, F2L1, F1B]
    assert sched(n=(512, 512, 512), nsweeps=5, fused_cfg=(0, 0, 0, 0, 0))[1] == [F2, F2, F1]
    assert sched(n=(256, 256, 256), nsweeps=4, fused_cfg=(5, 0, 0, 0, -1))[1] == [F2S, F2S]
    assert sched(n=(256, 256, 256), nsweeps=4, fused_cfg=(3, 0, 0, 0, -1))[1] == [F2N, F2N]
    assert sched(n=(256, 256, 256), nsweeps=4, fused_cfg=(9, 0, 0, 0, -1))[1] == [F1] * 4
    assert sched(n=(256, 256, 256), nsweeps=1, fused_cfg=(0, 7, 0, 0, -1))[1] == [F1B]
    p, got = sched(n=(256, 256, 256), nsweeps=1, want_res=True, fused_cfg=(0, 0, 9, 0, -1))
    assert got == [F1] and not p["res_done"]
    # block first below 3 M points: taken without asking fused, a pending correction is interpolated stand-alone
    assert sched(n=(128, 128, 128), nsweeps=5, corr=True, rhs=False, block_cfg=(0, 3000000))[1] == \
        ["prol+B2/8", "B2/8", "B1/8"]
    assert sched(n=(64, 64, 64), nsweeps=2, block_cfg=(4, 0))[1] == ["B2/4"]
    assert sched(n=(32, 32, 32), nsweeps=2, block_cfg=(8, 0))[1] == ["B2/8"]


def test_z_chunks():
    assert _lib.fused_z_chunks(512, 96, 256, 4) == (8, 64)          # 3 rounds x (64 + 8 + 3) planes = 225
    assert _lib.fused_z_chunks(512, 96, 256, 4, work_items=96) == (1, 512)
    assert _lib.fused_z_chunks(512, 96, 256, 4, work_items=96 * 400) == (128, 4)     # clamped to the pipeline depth
    assert _lib.fused_z_chunks(3, 96, 256, 4, work_items=96 * 400) == (1, 3)


def test_structure_of_random_plans():
    rnd = random.Random(7)
    shapes = [(16, 16, 16), (17, 16, 16), (33, 20, 18), (64, 64, 64), (96, 96, 96), (130, 128, 128), (257, 256, 256),
              (512, 512, 512), (64, 64), (128, 128), (200, 200)]
    for _ in range(600):
        n = rnd.choice(shapes)
        nbufs = rnd.choice((1, 2, 3))
        kw = dict(n=n, nsweeps=rnd.randint(1, 7), variant=rnd.choice((0, 0, 0, 1)), rhs=rnd.random() < 0.5,
                  want_res=rnd.random() < 0.4, want_met=rnd.random() < 0.4, corr=rnd.random() < 0.4,
                  all_neumann=rnd.random() < 0.25, nbufs=nbufs, keep=rnd.choice((-1, -1, 1, 2)) if nbufs == 3 else -1,
                  fused_cfg=(rnd.choice((0, 0, 3, 5, 9)), rnd.choice((0, 7, 8)), rnd.choice((0, 9)), 0,
                             rnd.choice((-1, 0, 1))),
                  block_cfg=(rnd.choice((0, 4, 8)), rnd.choice((0, 3000000))), no_block=rnd.random() < 0.2)
        p = _lib.relax_plan(**kw)
        assert p["err"] == 0, kw
        ps = p["passes"]
        assert sum(q["sweeps"] for q in ps) == kw["nsweeps"], kw
        cur = 0
        for i, q in enumerate(ps):
            assert q["src"] == cur, kw
            assert (q["src"] != q["dst"]) == (q["kind"] in ("fused", "block")), kw
            assert q["dst"] != kw["keep"] and q["dst"] < nbufs, kw
            assert not q["prolong_first"] or (i == 0 and kw["corr"] and q["src"] != kw["keep"]), kw
            assert q["mean_shift"] == (kw["all_neumann"] and q["kind"] not in ("small2d", "medium2d")), kw
            cur = q["dst"]
        assert p["result"] == cur, kw
        if kw["corr"]:    # interpolated exactly once: stand-alone, or by the first launch
            assert ps[0]["prolong_first"] != (ps[0]["mode"] == "P"), kw
        assert p["res_done"] == (ps[-1]["mode"] == "R") and p["met_done"] == (ps[-1]["mode"] == "M"), kw
        assert all(q["mode"] in ("", "P") for q in ps[:-1]), kw
