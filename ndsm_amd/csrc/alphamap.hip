// The alpha map of the Grad-Rubin iteration (DESIGN.md "Nonlinear force-free field"): a function given on the lower
// face, alpha0 (nx,ny), is carried along the field lines of B to every node of the grid.  One lane per node, x fastest,
// so a wave starts the 64 neighbouring lines of one row; there is no seed array and nothing but alpha (8 B/pt) and the
// optional status (4 B/pt) is written.  The line of a node is trace.hip's: the stage and the RK4 step are
// trace_step.hpp's, the cell, the first-face search and the snap line.hpp's, the loop line_walk.hpp's line_walk - the
// one trace_k walks with -, so the end point and the status of node l hold the bits of ndsmk_trace with the seed
//
//   r_d = lo_d + (double) i_d * h_d                 (on the last node hi_d's own expression: every node is inside)
//
// in the direction -polarity: polarity +1 follows the line against B, polarity -1 along B - back to where its current
// entered the box.  The result:
//
//   status == NDSMK_TRACE_ZLO   alpha = the bilinear interpolant of alpha0 at the end's (x, y): line_cell's cell and
//                               unclamped fractions, line_lerp3's operand order on two axes,
//                               c0 = v00 + fx (v10 - v00), c1 = v01 + fx (v11 - v01), alpha = c0 + fy (c1 - c0)
//   any other status            alpha = +0.0 (a line that leaves through a side or the top, ends at a null or does not
//                               finish carries no current)
//
// Fixed fp64 expressions in a fixed order (no contraction), no LDS; each node depends on its own line only.
#include "line_walk.hpp"

namespace {

using namespace ndsm;

// only the end and the status of the walk are wanted
struct LineEndOnly {
  __device__ __forceinline__ void step(int, const double *, const double *, const double *, double, double) {}
  static constexpr int kArrived = 0;   // (never)
  __device__ __forceinline__ bool arrived(const double *) { return false; }
};

__global__ __launch_bounds__(kLineBlock) void alpha_map_k(const double *__restrict__ B,
                                                          const double *__restrict__ alpha0,
                                                          double *__restrict__ alpha, int32_t *__restrict__ status,
                                                          TrArgs p) {
  const size_t l = (size_t)blockIdx.x * kLineBlock + threadIdx.x;
  const size_t sy = (size_t)p.n[0], sz = (size_t)p.n[0] * (size_t)p.n[1];
  const size_t N = sz * (size_t)p.n[2];
  if (l >= N) return;
  const size_t row = l / sy;
  const int i = (int)(l % sy), j = (int)(row % (size_t)p.n[1]), k = (int)(row / (size_t)p.n[1]);
  const double sgn = (double)p.sgn0;

  double r[3] = {p.lo[0] + (double)i * p.h[0], p.lo[1] + (double)j * p.h[1], p.lo[2] + (double)k * p.h[2]};
  LineEndOnly v;
  const int st = line_walk<false, false>(B, nullptr, p, N, sy, sz, sgn, r, nullptr, nullptr, v);
  double a = 0.0;
  if (st == NDSMK_TRACE_ZLO) {
    // (z = lo_z: the cell's z index is 0, so its base is the index into alpha0)
    const LineCell c = line_cell(p, r[0], r[1], p.lo[2]);
    const double *__restrict__ q = alpha0 + c.base;
    const double v00 = q[0], v10 = q[1], v01 = q[sy], v11 = q[sy + 1];
    const double c0 = v00 + c.fx * (v10 - v00);
    const double c1 = v01 + c.fx * (v11 - v01);
    a = c0 + c.fy * (c1 - c0);
  }
  alpha[l] = a;
  if (status) status[l] = st;
}

}  // namespace

// alpha (nx,ny,nz) = alpha0 (nx,ny; x fastest) carried along the lines of B (nx,ny,nz,3); status (nx,ny,nz; int32,
// may be NULL): the NDSMK_TRACE_* code of each node's line.  lo3, h_dq3: the mesh's first point and spacing per axis;
// step in units of min(h); polarity +1 / -1.  All arrays DEVICE arrays.  The lane index is a size_t: the shape is
// bounded by the launch (one wave per block, at most 2^31 - 1 blocks), not by line_args' 2^31 - 1 lanes.
// Asynchronous.
extern "C" int ndsmk_alpha_map(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3,
                               const double *alpha0, int polarity, double step, int max_steps, double *alpha,
                               int32_t *status) {
  NDSM_REQUIRE_READY();
  if (!(step > 0.0) || !(step <= 1.0e300) || max_steps < 1 || (polarity != 1 && polarity != -1))
    return fail(NDSMK_EVALUE, "alpha_map: step > 0 (finite), max_steps >= 1 and polarity +1 or -1", __FILE__, __LINE__);
  NDSM_CHECK_ARG(B && alpha0 && alpha && n3 && lo3 && h_dq3);
  NDSM_CHECK_ARG(n3[0] >= 2 && n3[1] >= 2 && n3[2] >= 2 && h_dq3[0] > 0.0 && h_dq3[1] > 0.0 && h_dq3[2] > 0.0);
  const size_t N = (size_t)n3[0] * (size_t)n3[1] * (size_t)n3[2];
  const size_t nb = (N + kLineBlock - 1) / kLineBlock;
  NDSM_CHECK_ARG(nb <= (size_t)0x7fffffff);
  TrArgs p;
  line_mesh(n3, lo3, h_dq3, step, max_steps, p);
  p.nseeds = 0;
  p.ndir = 1;
  p.sgn0 = -polarity;
  hipLaunchKernelGGL(alpha_map_k, dim3((unsigned)nb), dim3(kLineBlock), 0, ndsm::stream(), B, alpha0, alpha, status,
                     p);
  NDSM_LAUNCH_CHECK();
  return 0;
}
