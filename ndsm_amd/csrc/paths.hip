// Field-line paths on the device (DESIGN.md "Field-line paths"): the points of the lines that trace.hip only
// summarises, with B, G and the running integral at each.  The semantics are written out in include/ndsm_hip.h
// (ndsm_hip_vecpot_paths) and restated in numpy by tests/path_model.py bit for bit.  Variable-length results the way
// nulls.hip writes them - count, scan, then a second pass that repeats the same expressions and writes at its rank:
//
//   count   ndsmk_trace   the trace entry itself: ends, length, integral, status and n = nsteps of every line
//           npts_k        offsets[l] = npts(l) = 1 if n = 0, else (n - 1) / every + 2
//           scan64_k      in place: offsets[l] = the exclusive sum, offsets[nl] = the total; one workgroup, every lane
//                         sums a contiguous run (scan64.hpp's scan64_total, shared with skeleton.hip and
//                         separators.hip; the int64 sibling of nulls.hip's scan_k)
//   fill    paths_k       one lane per line, one wave per workgroup, as trace_k: line_walk.hpp's line_walk, the very
//                         loop trace_k runs - the same r and I -, with a visitor that stores the state before step
//                         0, every, 2 every, ... once that step is known to move the line, and the final state
//                         with one more interpolation at it.  Point j of line l goes to slot offsets[l] + j.
// A lane writes slot offsets[l] + j only for j < min(offsets[l + 1], max_points) - offsets[l]: its own count from the
// first pass and the capacity bound every store, whatever the second pass computes.  No atomic append, no guessed
// capacity, no result that depends on the launch geometry.  No vector is indexed with a run-time axis (the rule of
// squash.hip): the state stays in registers.
#include "line_walk.hpp"
#include "scan64.hpp"

namespace {

using namespace ndsm;

constexpr int kNptsBlock = 256;

__global__ __launch_bounds__(kNptsBlock) void npts_k(const int32_t *__restrict__ nsteps, size_t nl, int every,
                                                     i64 *__restrict__ npts) {
  const size_t l = (size_t)blockIdx.x * kNptsBlock + threadIdx.x;
  if (l >= nl) return;
  npts[l] = line_npts(nsteps[l], every);
}

// what the filling half adds to the walk: the running integral, and the sampled states into the lane's slots
template <bool kHasG>
struct PathVisitor {
  LineSlots &w;
  double I = 0.0;
  __device__ __forceinline__ void step(int it, const double r[3], const double bv[3], const double gv[3], double,
                                       double dI) {
    w.template sample<kHasG>(it, r, bv, gv, I);
    I = I + dI;
  }
  static constexpr int kArrived = 0;   // (never)
  __device__ __forceinline__ bool arrived(const double *) { return false; }
};

// lane l: seed l % nseeds, direction block l / nseeds, as trace_k; its points go to slots offsets[l] + j, j < room
template <bool kHasG>
__global__ __launch_bounds__(kLineBlock) void paths_k(const double *__restrict__ B, const double *__restrict__ G,
                                                      const double *__restrict__ seeds,
                                                      const i64 *__restrict__ offsets, i64 every, i64 max_points,
                                                      LinePts o, TrArgs p) {
  const size_t l = (size_t)blockIdx.x * kLineBlock + threadIdx.x;
  const size_t nl = (size_t)p.nseeds * (size_t)p.ndir;
  if (l >= nl) return;
  const size_t is = l % (size_t)p.nseeds;
  const double sgn = (l / (size_t)p.nseeds == 0) ? (double)p.sgn0 : -1.0;
  const size_t sy = (size_t)p.n[0], sz = (size_t)p.n[0] * (size_t)p.n[1];
  const size_t N = sz * (size_t)p.n[2];

  LineSlots w(o, offsets, l, every, max_points);
  if (w.room == 0) return;

  double r[3] = {seeds[3 * is], seeds[3 * is + 1], seeds[3 * is + 2]};
  double bv[3] = {0.0, 0.0, 0.0}, gv[3] = {0.0, 0.0, 0.0};
  PathVisitor<kHasG> v = {w};
  // OUTSIDE: no line, the seed's bits as given and nothing interpolated
  const bool run = line_inside(p, r);
  if (run) (void)line_walk<kHasG, true>(B, G, p, N, sy, sz, sgn, r, bv, gv, v);
  w.template last<kHasG>(B, G, p, N, sy, sz, sgn, run, r, bv, gv, v.I);
}

int path_args(const char *usage, bool own_ok, bool arrays_ok, const int32_t *n3, const double *lo3,
              const double *h_dq3, int nseeds, double step, int max_steps, int direction, TrArgs &p) {
  p.ndir = direction == 0 ? 2 : 1;
  p.sgn0 = direction < 0 ? -1 : 1;
  return line_args(usage, own_ok && direction >= -1 && direction <= 1, arrays_ok, n3, lo3, h_dq3, nseeds, step,
                   max_steps, p.ndir, p);
}

}  // namespace

// The counting half: ndsmk_trace with the same arguments (the five trace outputs are the trace entry's), then
// offsets (nl + 1, int64, DEVICE) = the exclusive sums of the lines' point counts for the stride `every`, offsets[nl]
// the total, which also comes back in *h_total (HOST).  max_points is the filling half's and only checked here: a call
// that the filling half would refuse launches nothing.  Blocks for the total.
extern "C" int ndsmk_paths_count(const double *B, const double *G, const int32_t *n3, const double *lo3,
                                 const double *h_dq3, int nseeds, const double *seeds, double step, int max_steps,
                                 int direction, int every, int64_t max_points, double *ends, double *length,
                                 double *integral, int32_t *status, int32_t *nsteps, int64_t *offsets,
                                 int64_t *h_total) {
  NDSM_REQUIRE_READY();
  if (h_total) *h_total = 0;
  TrArgs p;
  int rc = path_args("paths: step > 0 (finite), max_steps >= 1, direction in -1, 0, 1, every >= 1, max_points >= 0 and "
                     "nseeds >= 0",
                     every >= 1 && max_points >= 0, B && seeds && ends && length && integral && status && nsteps && offsets && h_total,
                     n3, lo3, h_dq3, nseeds, step, max_steps, direction, p);
  if (rc != 0 || nseeds == 0) return rc;
  rc = ndsmk_trace(B, G, n3, lo3, h_dq3, nseeds, seeds, step, max_steps, direction, ends, length, integral, status,
                   nsteps);
  if (rc != 0) return rc;
  const size_t nl = (size_t)nseeds * (size_t)p.ndir;
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(npts_k, dim3((unsigned)((nl + kNptsBlock - 1) / kNptsBlock)), dim3(kNptsBlock), 0, s, nsteps, nl,
                     every, (i64 *)offsets);
  NDSM_LAUNCH_CHECK();
  return scan64_total(offsets, nl, h_total, s);
}

// The filling half, after ndsmk_paths_count with the same arguments and its offsets: slot k < max_points of the
// concatenation into points (3 each) and, where given, bpt, gpt (3 each) and ipt (gpt, ipt are not looked at without
// G).  All DEVICE arrays.  max_points == 0 launches nothing.  Asynchronous.
extern "C" int ndsmk_paths_fill(const double *B, const double *G, const int32_t *n3, const double *lo3,
                                const double *h_dq3, int nseeds, const double *seeds, double step, int max_steps,
                                int direction, int every, int64_t max_points, const int64_t *offsets, double *points,
                                double *bpt, double *gpt, double *ipt) {
  NDSM_REQUIRE_READY();
  TrArgs p;
  const int rc = path_args("paths: step > 0 (finite), max_steps >= 1, direction in -1, 0, 1, every >= 1, "
                           "max_points >= 0 and nseeds >= 0",
                           every >= 1 && max_points >= 0, B && seeds && offsets && (max_points == 0 || points), n3,
                           lo3, h_dq3, nseeds, step, max_steps, direction, p);
  if (rc != 0 || nseeds == 0 || max_points == 0) return rc;
  const size_t nl = (size_t)nseeds * (size_t)p.ndir;
  const unsigned nb = (unsigned)((nl + kLineBlock - 1) / kLineBlock);
  const LinePts o = {points, bpt, G ? gpt : nullptr, G ? ipt : nullptr};
  hipStream_t s = ndsm::stream();
  if (G)
    hipLaunchKernelGGL(paths_k<true>, dim3(nb), dim3(kLineBlock), 0, s, B, G, seeds, (const i64 *)offsets, (i64)every,
                       (i64)max_points, o, p);
  else
    hipLaunchKernelGGL(paths_k<false>, dim3(nb), dim3(kLineBlock), 0, s, B, G, seeds, (const i64 *)offsets, (i64)every,
                       (i64)max_points, o, p);
  NDSM_LAUNCH_CHECK();
  return 0;
}
