// The walk of a traced field line, stated once for the kernels that follow a line with trace_step.hpp's stage and
// step (trace.hip, paths.hip, alphamap.hip, separators.hip; skeleton.hip's skel_line_k keeps a text of its own, its
// header says why), and what stands round it in the count-and-fill entries: the slots of a lane, the store of a
// point, the point count, the body of a null-line kernel.  What a
// kernel does with the walk goes in as a visitor, a struct passed by reference whose members are inlined: no function
// pointer, no virtual call, no vector indexed with a run-time axis; the state stays in registers.  Every kernel walks
// with these very expressions in this very order, so a path's points, a skeleton line and an alpha map's end carry
// the bits of the trace entry's states.
//
//   per step `it` from r   stage 1 at r (kKeep: B and G at r into bv, gv); the full step of length ds; the first face
//                          the chord meets; on a face the step is redone from r with s = t ds (stage 1 kept).  A null
//                          in any of the three ends the walk with r, bv, gv and the visitor as the step before left
//                          them.
//   v.step(it, r, bv, gv, s, dI)   the state BEFORE step `it`, now known to move the line by s (ds on a full step)
//   on a face              the end is snapped onto it: the walk ends with the face's code
//   else                   r = r'; v.arrived(r) ends the walk with V::kArrived (never tested after the exit step)
//   kRedo false            the walk ends at the first face with r the state before that step: nothing is redone,
//                          snapped or told to the visitor (the closest approach of separators.hip needs no exit point)
#pragma once

#include "trace_step.hpp"

namespace ndsm {

// returns NDSMK_TRACE_NULL, the code of the exit face, V::kArrived, or NDSMK_TRACE_UNFINISHED after max_steps
template <bool kHasG, bool kKeep, bool kRedo = true, class V>
__device__ __forceinline__ int line_walk(const double *__restrict__ B, const double *__restrict__ G, const TrArgs &p,
                                         size_t N, size_t sy, size_t sz, double sgn, double r[3], double *bv,
                                         double *gv, V &v) {
  int st = NDSMK_TRACE_UNFINISHED;
  for (int it = 0; it < p.max_steps; ++it) {
    double k1[3], q1, rn[3], dI;
    if (!tr_stage<kHasG, kKeep>(B, G, p, N, sy, sz, sgn, r[0], r[1], r[2], k1, q1, bv, gv) ||
        !tr_rk4<kHasG>(B, G, p, N, sy, sz, sgn, r, k1, q1, p.ds, rn, dI)) {
      st = NDSMK_TRACE_NULL;
      break;
    }
    double t;
    const int face = line_first_face(p, r, rn, t);
    double s = p.ds;
    if (face != 0) {
      if (!kRedo) {
        st = face;
        break;
      }
      // the step is redone with the length that reaches the face; stage 1 is the same
      s = t * p.ds;
      if (!tr_rk4<kHasG>(B, G, p, N, sy, sz, sgn, r, k1, q1, s, rn, dI)) {
        st = NDSMK_TRACE_NULL;
        break;
      }
    }
    v.step(it, r, bv, gv, s, dI);
    if (face != 0) {
      line_snap(p, face, rn, r);
      st = face;
      break;
    }
    r[0] = rn[0], r[1] = rn[1], r[2] = rn[2];
    if (v.arrived(r)) {
      st = V::kArrived;
      break;
    }
  }
  return st;
}

__device__ __forceinline__ bool line_inside(const LineArgs &p, const double r[3]) {
  bool inside = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) inside = inside && (r[d] >= p.lo[d]) && (r[d] <= p.hi[d]);
  return inside;
}

// the points of a line of ns steps sampled every `every` steps: the states before step 0, every, 2 every, ... and the
// final one
__host__ __device__ __forceinline__ i64 line_npts(int ns, int every) {
  return ns <= 0 ? 1 : (i64)((ns - 1) / every) + 2;
}

struct LinePts {
  double *points, *bpt, *gpt, *ipt;   // bpt, gpt, ipt may be nullptr: skipped (gpt, ipt are not looked at without G)
};

// slot k of the concatenation (the caller has bounded k)
template <bool kHasG>
__device__ __forceinline__ void line_put(const LinePts &o, i64 k, const double r[3], const double bv[3],
                                         const double gv[3], double I) {
  o.points[3 * k] = r[0];
  o.points[3 * k + 1] = r[1];
  o.points[3 * k + 2] = r[2];
  if (o.bpt) {
    o.bpt[3 * k] = bv[0];
    o.bpt[3 * k + 1] = bv[1];
    o.bpt[3 * k + 2] = bv[2];
  }
  if (kHasG) {
    if (o.gpt) {
      o.gpt[3 * k] = gv[0];
      o.gpt[3 * k + 1] = gv[1];
      o.gpt[3 * k + 2] = gv[2];
    }
    if (o.ipt) o.ipt[k] = I;
  }
}

// The slots of a lane in a filling half and how far it has filled them.  Lane l owns [offsets[l], min(offsets[l + 1],
// max_points)) and nothing else: its own count from the counting half and the capacity bound every store, whatever the
// filling half computes.  room == 0: the lane has nothing to write and traces nothing.
struct LineSlots {
  LinePts o;
  i64 base, room, every;
  i64 j, due;   // points stored so far; the next step count whose state is stored

  __device__ __forceinline__ LineSlots(const LinePts &out, const i64 *__restrict__ offsets, size_t l, i64 every_,
                                       i64 max_points)
      : o(out), every(every_), j(0), due(0) {
    base = offsets[l];
    const i64 next_base = offsets[l + 1];
    const i64 stop = next_base < max_points ? next_base : max_points;
    room = (base >= 0 && stop > base) ? stop - base : 0;
  }

  // step `it` moves the line: the state before it is a point when `it` is a multiple of every
  template <bool kHasG>
  __device__ __forceinline__ void sample(int it, const double r[3], const double bv[3], const double gv[3], double I) {
    if ((i64)it == due) {
      if (j < room) line_put<kHasG>(o, base + j, r, bv, gv, I);
      j = j + 1;
      due = due + every;
    }
  }

  // the final state.  ran: a line was walked, so B and G are interpolated at it once more (after the snap, whatever
  // |B| is there); else the seed's bits as given with the zero bv, gv it started with.
  template <bool kHasG>
  __device__ __forceinline__ void last(const double *__restrict__ B, const double *__restrict__ G, const TrArgs &p,
                                       size_t N, size_t sy, size_t sz, double sgn, bool ran, const double r[3],
                                       double *bv, double *gv, double I) {
    if (j < room) {
      if (ran) {
        double k1[3], q1;
        (void)tr_stage<kHasG, true>(B, G, p, N, sy, sz, sgn, r[0], r[1], r[2], k1, q1, bv, gv);
      }
      line_put<kHasG>(o, base + j, r, bv, gv, I);
    }
  }
};

// ---- the lines of the nulls (separators.hip's sep_line_k; the statement of skel_line_k's body with its capture test
// as the policy Cap): a seed and a direction per lane from a LineScratch, no G, ended by a capture test after every accepted full step.  kFill false: the line's outputs and its point count;
// true: its points into the lane's slots.

struct NullLineOut {
  double *ends, *length;            // the counting pass
  int32_t *status, *nsteps, *hit;   // (hit: only for a capture that names the null, Cap::kHit)
  i64 *npts;                        // offsets before the scan
  LinePts pts;                      // the filling pass: points, bpt (may be nullptr)
};

template <bool kFill, class Cap>
struct NullLineVisitor {
  Cap &cap;
  LineSlots *w;   // (kFill)
  double len = 0.0;
  int ns = 0;
  __device__ __forceinline__ void step(int it, const double r[3], const double bv[3], const double *, double s,
                                       double) {
    if (kFill) w->template sample<false>(it, r, bv, nullptr, 0.0);
    len = len + s;
    ns = it + 1;
  }
  static constexpr int kArrived = NDSMK_SKEL_CAPTURED;
  __device__ __forceinline__ bool arrived(const double r[3]) { return cap.test(r); }
};

// lane l: the line from seeds[l] in the direction sgns[l]; 0: no line (NDSMK_SKEL_NONE, one point), then a seed
// outside the box: NDSMK_TRACE_OUTSIDE.  cap.test(r): r lies within the capture radius (cap.hit: of which null).
template <bool kFill, class Cap>
__device__ __forceinline__ void null_line(const double *__restrict__ B, const double *__restrict__ seeds,
                                          const double *__restrict__ sgns, size_t l, Cap &cap,
                                          const i64 *__restrict__ offsets, i64 every, i64 max_points,
                                          const NullLineOut &o, const TrArgs &p) {
  const double sgn = sgns[l];
  const size_t sy = (size_t)p.n[0], sz = (size_t)p.n[0] * (size_t)p.n[1];
  const size_t N = sz * (size_t)p.n[2];
  double r[3] = {seeds[3 * l], seeds[3 * l + 1], seeds[3 * l + 2]};
  double bv[3] = {0.0, 0.0, 0.0};
  NullLineVisitor<kFill, Cap> v = {cap, nullptr};
  int st = sgn == 0.0 ? NDSMK_SKEL_NONE : (line_inside(p, r) ? 0 : NDSMK_TRACE_OUTSIDE);
  const bool run = st == 0;
  if (kFill) {
    LineSlots w(o.pts, offsets, l, every, max_points);
    if (w.room == 0) return;
    v.w = &w;
    if (run) (void)line_walk<false, true>(B, nullptr, p, N, sy, sz, sgn, r, bv, nullptr, v);
    w.last<false>(B, nullptr, p, N, sy, sz, sgn, run, r, bv, nullptr, 0.0);
  } else {
    if (run) st = line_walk<false, true>(B, nullptr, p, N, sy, sz, sgn, r, bv, nullptr, v);
    o.ends[3 * l] = r[0];
    o.ends[3 * l + 1] = r[1];
    o.ends[3 * l + 2] = r[2];
    o.length[l] = v.len;
    o.status[l] = st;
    o.nsteps[l] = v.ns;
    if constexpr (Cap::kHit) o.hit[l] = cap.hit;
    o.npts[l] = line_npts(v.ns, (int)every);
  }
}

// rho = radius min(h) and cap2 = (capture min(h))^2 of the null-line entries
inline void null_line_radii(const double *h_dq3, double radius, double capture, double &rho, double &cap2) {
  const double hmin = fmin(fmin(h_dq3[0], h_dq3[1]), h_dq3[2]);
  rho = radius * hmin;
  const double cr = capture * hmin;
  cap2 = cr * cr;
}

}  // namespace ndsm
