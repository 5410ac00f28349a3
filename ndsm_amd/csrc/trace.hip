// Field-line tracing and line integrals on the device (DESIGN.md "Field-line tracing and field-line helicity").
// One lane per (seed, direction): a latency-bound gather with a data-dependent trip count per lane, unlike the
// plane-streaming kernels of the other files.  The arithmetic is fixed fp64 expressions in a fixed order (no
// contraction: -ffp-contract=off), so a numpy restatement matches bit for bit.  Interpolation, the first-face search
// and the snap of the exit point are line.hpp's (the specification is at the top of that file); here:
//
//   stage at p                  b = B(p), m = sqrt((bx bx + by by) + bz bz); not m > 0: the line ends "null";
//                               e = b / m, k = sgn e, q = (Gx ex + Gy ey) + Gz ez   (sgn = +1 forward, -1 backward;
//                               q has no sgn: the integral runs in the direction of B for both directions)
//   RK4 step of length s from r k1 = k(r), k2 = k(r + (0.5 s) k1), k3 = k(r + (0.5 s) k2), k4 = k(r + s k3),
//                               r' = r + (s / 6) (((k1 + 2 k2) + 2 k3) + k4), dI = (s / 6) (((q1 + 2 q2) + 2 q3) + q4)
//   exit                        r' outside [lo, hi]: the step is redone from r with s = t ds (k1, q1 kept), t of the
//                               first face; then the end is snapped onto that face.
// Every lane's loop is bounded by max_steps.  The stage and the step are trace_step.hpp's and the loop itself is
// line_walk.hpp's line_walk, shared with paths.hip, alphamap.hip and separators.hip; this entry adds the sums of the
// accepted steps.
#include "line_walk.hpp"

namespace {

using namespace ndsm;

// the sums of a line: formed for accepted steps only, so a null leaves them at the previous step's values
struct TraceSums {
  double len = 0.0, I = 0.0;
  int ns = 0;
  __device__ __forceinline__ void step(int it, const double *, const double *, const double *, double s, double dI) {
    len = len + s;
    I = I + dI;
    ns = it + 1;
  }
  static constexpr int kArrived = 0;   // (never)
  __device__ __forceinline__ bool arrived(const double *) { return false; }
};

// lane l: seed l % nseeds, direction block l / nseeds.  Outputs per lane: ends[3 l .. 3 l + 2], length[l],
// integral[l], status[l], nsteps[l].
template <bool kHasG>
__global__ __launch_bounds__(kLineBlock) void trace_k(const double *__restrict__ B, const double *__restrict__ G,
                                                      const double *__restrict__ seeds, double *__restrict__ ends,
                                                      double *__restrict__ length, double *__restrict__ integral,
                                                      int32_t *__restrict__ status, int32_t *__restrict__ nsteps,
                                                      TrArgs p) {
  const size_t l = (size_t)blockIdx.x * kLineBlock + threadIdx.x;
  const size_t nl = (size_t)p.nseeds * (size_t)p.ndir;
  if (l >= nl) return;
  const size_t is = l % (size_t)p.nseeds;
  const double sgn = (l / (size_t)p.nseeds == 0) ? (double)p.sgn0 : -1.0;
  const size_t sy = (size_t)p.n[0], sz = (size_t)p.n[0] * (size_t)p.n[1];
  const size_t N = sz * (size_t)p.n[2];

  double r[3] = {seeds[3 * is], seeds[3 * is + 1], seeds[3 * is + 2]};
  TraceSums v;
  int st = NDSMK_TRACE_OUTSIDE;
  if (line_inside(p, r)) st = line_walk<kHasG, false>(B, G, p, N, sy, sz, sgn, r, nullptr, nullptr, v);
  ends[3 * l] = r[0];
  ends[3 * l + 1] = r[1];
  ends[3 * l + 2] = r[2];
  length[l] = v.len;
  integral[l] = v.I;
  status[l] = st;
  nsteps[l] = v.ns;
}

}  // namespace

// Field lines of B (nx,ny,nz,3) from nseeds seeds (3 each, physical coordinates), with the line integral of G
// (nullptr: none, integrals 0).  lo3, h_dq3: the mesh's first point and spacing per axis.  step in units of
// min(h); direction +1 forward, -1 backward, 0 both (forward block, then backward block).  All arrays DEVICE
// arrays; the outputs hold nseeds (one direction) or 2 nseeds (both) lines.  Asynchronous.
extern "C" int ndsmk_trace(const double *B, const double *G, const int32_t *n3, const double *lo3, const double *h_dq3,
                           int nseeds, const double *seeds, double step, int max_steps, int direction, double *ends,
                           double *length, double *integral, int32_t *status, int32_t *nsteps) {
  NDSM_REQUIRE_READY();
  TrArgs p;
  p.ndir = direction == 0 ? 2 : 1;
  p.sgn0 = direction < 0 ? -1 : 1;
  const int rc = line_args("trace: step > 0 (finite), max_steps >= 1, direction in -1, 0, 1 and nseeds >= 0",
                           direction >= -1 && direction <= 1,
                           B && seeds && ends && length && integral && status && nsteps, n3, lo3, h_dq3, nseeds, step,
                           max_steps, p.ndir, p);
  if (rc != 0 || nseeds == 0) return rc;
  const size_t nl = (size_t)nseeds * (size_t)p.ndir;
  const unsigned nb = (unsigned)((nl + kLineBlock - 1) / kLineBlock);
  hipStream_t s = ndsm::stream();
  if (G)
    hipLaunchKernelGGL(trace_k<true>, dim3(nb), dim3(kLineBlock), 0, s, B, G, seeds, ends, length, integral, status,
                       nsteps, p);
  else
    hipLaunchKernelGGL(trace_k<false>, dim3(nb), dim3(kLineBlock), 0, s, B, G, seeds, ends, length, integral, status,
                       nsteps, p);
  NDSM_LAUNCH_CHECK();
  return 0;
}
