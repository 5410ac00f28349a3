// Which launches a relax call makes: ONE pure function of the grid descriptor, the request and the development
// knobs ("Which launch a relax call makes").  Host-only C++17: no HIP, no globals, no environment -
// smooth.hip, smooth_fused.hip, smooth_block.hip and mixed.hip execute what it returns, and
// ndsmk_debug_relax_plan shows it to tests on machines without a GPU.
#pragma once

#include <cstdint>
#include <vector>

#include "ndsm_kernels.h"

namespace ndsm {
namespace plan {

enum Kind { SMALL3D = 1, SMALL2D, MEDIUM2D, FUSED, BLOCK, COLOR3D, COLOR2D };
enum Mode { PLAIN = 0, RES = 1, MET = 2, CORR = 3 };   // rbgs3_fused_k's MODE: + residual / + metric / + correction

// the instantiations of rbgs3_fused_k: sweeps (+ mode), TXH x TYH tile, threads, level-1 symbol; kOddNx added:
// the odd-nx instantiation (the tuning alternates and the level-1 symbol exist for even nx only)
enum FusedInst {
  NO_INST = 0,
  F2_136x30_1024 = 1,
  F2_136x30_1024_L1,
  F2_136x22_768,
  F2_72x28_512,
  F1_132x23_768,
  F1_132x31_1024,
  F1R_136x22_768,
  F2M_136x30_1024,
  F1M_132x31_1024,
  F1M_132x23_768,
  F1P_132x31_1024,
  F2P_136x30_1024,
  kOddNx = 16
};

constexpr int kMed2D = 19456;                      // points of the largest 2-D level one workgroup holds in LDS
constexpr int64_t kPlaneBytes = 0x80000000ll;      // a plane is addressed with 32-bit byte offsets below 2 GiB

struct Knobs {
  int fused[5] = {0, 0, 0, 0, -1};   // NDSM_FUSED_CFG: two-sweep cfg, one-sweep cfg, sweep+residual cfg, work items, big
  int64_t block[2] = {0, 0};         // NDSM_BLOCK_CFG: block height, "block first below this many points"
  bool block_on = true;              // NDSM_HIP_NO_BLOCK unset
};

struct Request {
  int nsweeps = 0;
  int variant = 0;            // 0 best launch per level, 1 colour passes only, 2 fused or an error ("force")
  bool window = false;        // ONE forced fused pass of exactly nsweeps sweeps over g's owned planes, or an error
  bool fp32 = false;          // the fp32 smoother of the mixed-precision mode: fused passes only
  bool rhs = true;            // false: the right-hand side is identically zero
  bool want_res = false, want_met = false;
  bool corr = false;          // u += P uc is pending
  int64_t coarse_plane = 0;   // points of a plane of uc; < 0: the transfer's windows do not fit g (stand-alone only)
  bool have[3] = {true, false, false};   // buffers that exist; buffer 0 holds u
  int keep = -1;              // index of the buffer that must survive, or -1
  bool src_zero = false;      // buffer 0 is zero but was never written: the first guess of a coarse level
};

struct Pass {
  int kind = 0, sweeps = 1;
  int mode = PLAIN, inst = NO_INST;   // fused passes
  int bz = 0;                         // block passes: block height (S = sweeps)
  int src = 0, dst = 0;               // in-place passes: src == dst
  bool prolong_first = false;         // the stand-alone interpolation runs on src in front of this pass
  bool mean_shift = false;            // the mean of dst is subtracted after it
  bool src_zero = false;              // fused passes: src is not read, every plane of it comes from a descriptor of
                                      // zero records (a zero source that was never written)
};

struct Plan {
  int err = 0;                  // NDSMK_EARG and its text, or 0
  const char *what = "";
  std::vector<Pass> pass;
  bool prolong_only = false;    // no pass at all, but the stand-alone interpolation runs on buffer 0
  int result = 0;               // the buffer that ends up holding the swept field
  bool res_done = false, met_done = false;   // a pass covered them; else the stand-alone kernels follow
  bool materialise = false;     // the request's zero source has to be written to buffer 0 before anything runs
};

struct FusedPass {
  int inst = NO_INST, sweeps = 0, mode = PLAIN;
};

// The fused launch that performs the next of `left` sweeps over g's owned planes, or none.
// want_res / want_met: the launch that performs the LAST sweep carries them.  corr: only a launch that interpolates
// while it loads will do.
inline FusedPass fused_pass(const ndsmk_grid &g, const Knobs &kn, const Request &rq, int left, bool have_dst,
                            bool want_res, bool want_met, bool corr) {
  const FusedPass none;
  const bool force = rq.window || rq.variant == 2;
  const int odd = (g.n[0] & 1) ? kOddNx : 0;
  const int nzo = g.zown1 - g.zown0;   // owned planes
  if (!have_dst || g.ndim != 3 || (odd && rq.fp32) || g.n[0] < 16 || g.n[1] < 16 || nzo < (force ? 1 : 8)) return none;
  if ((int64_t)g.n[0] * g.n[1] * (rq.fp32 ? 4 : 8) >= kPlaneBytes) return none;
  // a z-streaming workgroup walks >= 16 planes serially: with fewer than ~one
  // workgroup per CU the sweep is latency bound and the two colour passes win
  const int64_t npts = (int64_t)g.n[0] * g.n[1] * nzo;
  const bool slab = nzo != g.n[2];
  if (npts < (int64_t)2 * 1024 * 1024 && !slab && !force) return none;
  // Tile choices measured on MI355X (scripts/tune_smoother.py); z_chunks picks the z chunking.
  const int *cfg = kn.fused;
  const bool big = cfg[4] < 0 ? npts >= (int64_t)64 * 1024 * 1024 : cfg[4] != 0;
  // A z-slab carries zown0 ghost planes below and n[2] - zown1 above its owned range; the caller
  // (ndsmh_world) has exchanged as many as the pass it asks for consumes: 2 per sweep, +1 for
  // the residual stage.
  const int ghosts = slab ? (g.zown0 < g.n[2] - g.zown1 ? g.zown0 : g.n[2] - g.zown1) : 1 << 20;
  const bool res = want_res && ghosts >= 3 && cfg[2] != 9;
  // two sweeps per pass - not for the last two sweeps when the residual is wanted (it rides
  // on a one-sweep pass)
  const bool two = left >= 2 && ghosts >= 4 && cfg[0] != 9 && !(res && left == 2);
  // the convergence metric against the iterate the V-cycle started from: fp64 only
  const bool met = !rq.fp32 && want_met;
  // corr: u + P u_c is formed while the planes are loaded (MODE 3): a one-sweep pass (any right-hand side) or a
  // two-sweep pass (rhs == 0 only); else the caller interpolates with the stand-alone kernel first.
  // The TWO-sweep correction launch exists for the declared-zero right-hand side only: with a right-hand-side
  // window on top of the interpolation state it does not fit 128 registers (round 3, weights already in LDS: 124
  // bytes of scratch per lane).  The ONE-sweep one carries a right-hand side too (52 bytes of scratch per lane,
  // outside the plane loop's steady state; 512^3 Poisson cycle 6.83 -> 6.41 ms against the stand-alone
  // interpolation in front of the sweeps).
  // The interpolation costs ~100 instructions per plane-step and wave.  On top of a TWO-sweep pass - which is bound
  // by instruction issue with it - that is +240 us at 512^3 (720 against 480); a ONE-sweep pass has the issue
  // slots to spare (it is bound by memory: 430 us).  So an odd number of sweeps (NDSM's ms = 5) is taken as
  // 1 + 2 + 2 with the correction on the one-sweep pass - the sweeps that remain are two-sweep passes, the last
  // of which carries the convergence metric - instead of 2 + 2 + 1.
  if (corr) {
    if (rq.fp32 || rq.coarse_plane < 0 || rq.coarse_plane * 8 >= kPlaneBytes) return none;
    if (cfg[0] == 0 && (left & 1) && (left >= 3 || slab))   // (a slab window asks for exactly its pass)
      return {F1P_132x31_1024 + odd, 1, CORR};
    if (!rq.rhs && two && cfg[0] == 0) return {F2P_136x30_1024 + odd, 2, CORR};
    return none;
  }
  // the metric rides on the last launch, and the residual takes precedence
  if (met && two && left == 2) return {F2M_136x30_1024 + odd, 2, MET};
  if (met && !two && left == 1 && !res) return {(big ? F1M_132x31_1024 : F1M_132x23_768) + odd, 1, MET};
  // THREE sweeps per pass were tried and are not built: six LDS planes force a narrower tile (72 x 46 or
  // 88 x 38 owned 60 x 34 / 76 x 26: 1.6-1.7x redundant stage work instead of 1.45x) and the pass turns
  // LDS / issue bound - measured at 512^3 (Laplace): 1075-1120 us per three-sweep pass against 553 us per
  // two-sweep pass, i.e. 358 against 282 us per sweep; same bits (scripts/time_s3.py, round 2).
  if (two) {
    if (odd) return {F2_136x30_1024 + odd, 2, PLAIN};
    // levels of a few million points (the 128^3 level of a 512^3 hierarchy) do not fill the chip with
    // 136 x 30 tiles: the 72 x 28 tile (512 threads) gives four times the workgroups - measured 77 against
    // 98 us per five sweeps at 128^3, 293 against 280 us at 256^3 (scripts/time_tail.py)
    const int two_cfg = cfg[0] ? cfg[0] : (npts < (int64_t)6 * 1024 * 1024 && !slab ? 5 : 0);
    // (fp32: four LDS planes are 65 KB, so two workgroups would fit a CU at <= 64 VGPRs - tried:
    // __launch_bounds__(1024, 8) gives 64 VGPRs + 44 B of scratch and the mixed-precision cycle at 512^3
    // goes from 6.5 to 7.9 ms; not built)
    return {two_cfg == 3 ? F2_136x22_768 : two_cfg == 5 ? F2_72x28_512 : big ? F2_136x30_1024_L1 : F2_136x30_1024, 2,
            PLAIN};
  }
  if (res && left == 1) return {F1R_136x22_768 + odd, 1, RES};
  return {((cfg[1] ? cfg[1] : (big ? 7 : 8)) == 8 ? F1_132x23_768 : F1_132x31_1024) + odd, 1, PLAIN};
}

// g is a whole 3-D level (no z-slab window)
inline bool whole_level(const ndsmk_grid &g) { return g.k0 == 0 && g.zown0 == 0 && g.zown1 == g.n[2]; }

// The block-resident launch (two sweeps, or a last single one) takes the whole, not all-Neumann levels above the
// single-workgroup limit that the fused launcher declines - up to 512 K points: measured per five sweeps at
// 32^3 / 64^3 / 96^3 / 128^3, block 19 / 28 / 65 / 123 us, colour passes 28 / 38 / 56 / 107 us, fused
// 62 / 65 / 67 / 73 us (scripts/time_small_levels.py, profiles/block_levels.txt; the lines cross near 600 K).
// Returns the block height (4 or 8), or 0: not a block level.  *first: the knob sends it there before fused is asked.
inline int block_height(const ndsmk_grid &g, const Knobs &kn, const Request &rq, bool have_dst, bool *first) {
  const int64_t npts = (int64_t)g.n[0] * g.n[1] * g.n[2];
  *first = false;
  if (rq.variant != 0 || rq.fp32 || rq.window || !have_dst || g.ndim != 3 || g.all_neumann || npts <= 4096 ||
      !whole_level(g) || !(npts < (int64_t)512 * 1024 || npts < kn.block[1]))
    return 0;
  *first = npts < kn.block[1];
  if (!kn.block_on || g.nzg != g.n[2]) return 0;
  const int64_t gx = (g.n[0] + 15) / 16, gy = (g.n[1] + 7) / 8, gz8 = (g.n[2] + 7) / 8, gz4 = (g.n[2] + 3) / 4;
  if (gy > 65535 || gz4 > 65535) return 0;   // grid-dimension caps
  // 16 x 8 x 8 blocks; where they give fewer than 64 workgroups (32^3: 32) half-height blocks spread the
  // level over twice as many CUs
  return kn.block[0] == 4 || (kn.block[0] != 8 && gx * gy * gz8 < 64) ? 4 : 8;
}

inline Plan fail(const char *what) {
  Plan p;
  p.err = NDSMK_EARG;
  p.what = what;
  return p;
}

inline Plan relax_plan_as_stored(const ndsmk_grid &g, const Request &rq, const Knobs &kn);

// A zero source that was never written (Request::src_zero) changes no launch: the plan is the one of the same
// request on an array of zeros, and its FIRST pass takes the zeros from a descriptor of zero records where it is
// an out-of-place fused pass of a whole fp64 level in mode plain or + residual - one or two sweeps, even or odd
// nx.  Everything else reads its source from memory - in-place passes, the block-resident and single-workgroup
// launches, the stand-alone interpolation, no pass at all - or is out of scope (windows and z-slabs, fp32,
// all-Neumann levels, whose mean shift follows every sweep): the zeros are written first (Plan::materialise).
inline Plan relax_plan(const ndsmk_grid &g, const Request &rq, const Knobs &kn) {
  Plan pl = relax_plan_as_stored(g, rq, kn);
  if (!rq.src_zero || pl.err) return pl;
  const bool direct = !pl.pass.empty() && pl.pass[0].kind == FUSED && pl.pass[0].src == 0 && pl.pass[0].dst != 0 &&
                      (pl.pass[0].mode == PLAIN || pl.pass[0].mode == RES) && !pl.pass[0].prolong_first &&
                      !rq.window && !rq.fp32 && !rq.corr && !g.all_neumann && whole_level(g);
  if (direct)
    pl.pass[0].src_zero = true;
  else
    pl.materialise = true;
  return pl;
}

inline Plan relax_plan_as_stored(const ndsmk_grid &g, const Request &rq, const Knobs &kn) {
  if (!(g.ndim == 2 || g.ndim == 3) || !(g.n[0] >= 2 && g.n[1] >= 2 && (g.ndim == 2 ? g.n[2] == 1 : g.n[2] >= 2)))
    return fail("relax: 2 or 3 dimensions of >= 2 points each");
  for (int d = 0; d < g.ndim; ++d)
    if (g.lb[d] < 0 || g.ub[d] > g.n[d] - 1) return fail("relax: update bounds outside the level");
  if (rq.variant < 0 || rq.variant > 2) return fail("relax: variant 0, 1 or 2");
  if (g.ndim == 3 && !(g.zown0 >= 0 && g.zown1 <= g.n[2] && g.zown0 < g.zown1)) return fail("relax: empty owned planes");
  Plan pl;
  // ---- a window: the one fused pass the caller asked for.  No correction or metric on all-Neumann levels ----
  if (rq.window) {
    const FusedPass f = g.all_neumann && (rq.corr || rq.want_met)
                            ? FusedPass()
                            : fused_pass(g, kn, rq, rq.nsweeps, rq.have[1], rq.want_res, rq.want_met, rq.corr);
    if (f.sweeps != rq.nsweeps || (rq.want_res && f.mode != RES) || (rq.want_met && f.mode != MET))
      return fail(rq.want_res ? "fused sweep + residual: this window is not covered"
                              : "fused smoother: this window / sweep count is not covered");
    Pass p;
    p.kind = FUSED, p.sweeps = f.sweeps, p.mode = f.mode, p.inst = f.inst, p.dst = 1;
    pl.pass.push_back(p);
    pl.result = 1, pl.res_done = f.mode == RES, pl.met_done = f.mode == MET;
    return pl;
  }
  const int64_t npts = (int64_t)g.n[0] * g.n[1] * g.n[2];
  const bool empty = g.ub[0] < g.lb[0] || g.ub[1] < g.lb[1] || (g.ndim == 3 && g.ub[2] < g.lb[2]);
  if ((empty && !rq.fp32) || rq.nsweeps <= 0) {   // nothing to update
    pl.prolong_only = rq.corr;
    return pl;
  }
  const bool fused_only = rq.variant == 2 || rq.fp32;
  const char *const in_place = "relax: an in-place pass would overwrite the buffer to keep";
  // ---- every sweep in ONE single-workgroup launch: <= 4096 points (u and rhs in LDS; 3-D: not all-Neumann, the
  // 2-D kernels shift the mean themselves), 2-D up to kMed2D points (u in LDS only) ----
  int one_wg = 0;
  if (rq.variant == 0 && !rq.fp32) {
    if (g.ndim == 3)
      one_wg = !g.all_neumann && npts <= 4096 && whole_level(g) ? SMALL3D : 0;
    else
      one_wg = npts <= 4096 ? SMALL2D : npts <= kMed2D ? MEDIUM2D : 0;
  }
  if (one_wg) {
    if (rq.keep == 0) return fail(in_place);
    Pass p;
    p.kind = one_wg, p.sweeps = rq.nsweeps, p.prolong_first = rq.corr;
    pl.pass.push_back(p);
    return pl;
  }
  int cur = 0;
  bool corr = rq.corr;
  for (int sw = 0; sw < rq.nsweeps;) {
    Pass p;
    p.src = p.dst = cur;
    if (g.ndim == 3 && rq.variant != 1) {
      // destination of an out-of-place pass: not the current buffer, not the kept one
      int dst = -1;
      for (int c = 2; c >= 0; --c)
        if (c != cur && rq.have[c] && c != rq.keep) dst = c;
      // all-Neumann levels shift the mean after EVERY sweep: one sweep per pass there, and neither the residual nor
      // the metric rides along (the mean shift comes in between)
      const int left = g.all_neumann ? 1 : rq.nsweeps - sw;
      bool blk_first;
      const int bz = block_height(g, kn, rq, dst >= 0, &blk_first);
      FusedPass f;
      if (corr && !blk_first) f = fused_pass(g, kn, rq, left, dst >= 0, false, false, true);
      if (corr && !f.inst) p.prolong_first = true;   // not that launch: interpolate in place, then sweep as usual
      if (!f.inst && !blk_first)
        f = fused_pass(g, kn, rq, left, dst >= 0, rq.want_res && !g.all_neumann, rq.want_met && !g.all_neumann, false);
      if (f.inst) {
        p.kind = FUSED, p.sweeps = f.sweeps, p.mode = f.mode, p.inst = f.inst, p.dst = dst;
        pl.res_done = f.mode == RES, pl.met_done = f.mode == MET;
      } else if (bz) {
        p.kind = BLOCK, p.sweeps = left >= 2 ? 2 : 1, p.bz = bz, p.dst = dst;
      } else if (fused_only) {
        return fail(rq.fp32 ? "fp32 smoother: the fused kernel does not cover this level"
                            : "fused smoother does not support this level shape");
      }
    }
    if (!p.kind) {   // the two colour passes, in place
      if (g.ndim == 3 && !(g.zown0 == 0 && g.zown1 == g.n[2]))
        return fail("z-slab levels need the fused smoother (>= 16 x 16 points per plane, >= 8 owned planes)");
      p.kind = g.ndim == 3 ? COLOR3D : COLOR2D;
      p.prolong_first = corr;
    }
    corr = false;
    if ((p.prolong_first || p.src == p.dst) && p.src == rq.keep) return fail(in_place);
    p.mean_shift = g.all_neumann != 0;
    pl.pass.push_back(p);
    cur = p.dst;
    sw += p.sweeps;
  }
  pl.result = cur;
  return pl;
}

// z chunks of a fused launch.  A workgroup walks its chunk plus nst warm-up planes on either side, and
// the chip runs `slots` (= CUs x occupancy) workgroups at a time: pick the chunk count that
// minimises (rounds of workgroups) x (planes walked per workgroup).  nzo: owned planes; nst: pipeline depth;
// res: the residual pipeline; target_wgs > 0: that many work items instead.
struct Chunks {
  int nzc, zc;   // chunks, planes per chunk
};
inline Chunks z_chunks(int nzo, int tiles, int64_t slots, int nst, bool res, int target_wgs) {
  int nzc;
  if (target_wgs > 0) {
    nzc = (target_wgs + tiles - 1) / tiles;
    if (nzc < 1) nzc = 1;
    int zc = (nzo + nzc - 1) / nzc;
    if (zc < nst) zc = nst < nzo ? nst : nzo;   // (down to the pipeline depth: what the chunk-count timings force)
    nzc = (nzo + zc - 1) / zc;
  } else {
    int64_t best = -1;
    nzc = 1;
    for (int c = 1; c <= (nzo + 7) / 8; ++c) {
      const int zc = (nzo + c - 1) / c;
      const int cc = (nzo + zc - 1) / zc;
      const int64_t rounds = ((int64_t)tiles * cc + slots - 1) / slots;
      const int64_t cost = rounds * (zc + 2 * nst + (res ? 0 : nst - 1));
      if (best < 0 || cost < best) {
        best = cost;
        nzc = cc;
      }
    }
  }
  const int zc = (nzo + nzc - 1) / nzc;
  return {(nzo + zc - 1) / zc, zc};
}

}  // namespace plan
}  // namespace ndsm
