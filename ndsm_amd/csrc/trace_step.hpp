// One stage and one RK4 step of a traced field line, shared by every line kernel (the expressions are written out at
// the top of trace.hip and in include/ndsm_hip.h; fixed fp64 operand order, no contraction).  line_walk.hpp builds the
// walk from these very functions, so a path's points carry the bits of the trace entry's states.
#pragma once

#include "line.hpp"

namespace ndsm {

struct TrArgs : LineArgs {
  int ndir;       // 1 or 2
  int sgn0;       // direction of the first block of lanes: +1 or -1 (both: +1, the second block is -1)
};

// one stage at (x,y,z): k[3] = sgn B/|B|, q = G . B/|B| (0 without G).  false: |B| is not > 0 (zero or NaN).
// kKeep: the interpolated B (and G) themselves go into bv[3] (gv[3]) as well, whatever |B| is.
template <bool kHasG, bool kKeep = false>
__device__ __forceinline__ bool tr_stage(const double *__restrict__ B, const double *__restrict__ G, const TrArgs &p,
                                         size_t N, size_t sy, size_t sz, double sgn, double x, double y, double z,
                                         double k[3], double &q, double *bv = nullptr, double *gv = nullptr) {
  const LineCell c = line_cell(p, x, y, z);
  double vb[3][8], vg[3][8];
  line_gather(B, N, sy, sz, c, vb);
  if (kHasG) line_gather(G, N, sy, sz, c, vg);
  const double bx = line_lerp3(vb[0], c), by = line_lerp3(vb[1], c), bz = line_lerp3(vb[2], c);
  if (kKeep) {
    bv[0] = bx, bv[1] = by, bv[2] = bz;
    if (kHasG) gv[0] = line_lerp3(vg[0], c), gv[1] = line_lerp3(vg[1], c), gv[2] = line_lerp3(vg[2], c);
  }
  const double m = sqrt((bx * bx + by * by) + bz * bz);
  q = 0.0;
  if (!(m > 0.0)) return false;
  const double ex = bx / m, ey = by / m, ez = bz / m;
  k[0] = sgn * ex;
  k[1] = sgn * ey;
  k[2] = sgn * ez;
  if (kHasG) {
    const double gx = line_lerp3(vg[0], c), gy = line_lerp3(vg[1], c), gz = line_lerp3(vg[2], c);
    q = (gx * ex + gy * ey) + gz * ez;
  }
  return true;
}

// stages 2-4 and the sums of one RK4 step of length s from r (k1, q1 given).  false: a stage met a null.
template <bool kHasG>
__device__ __forceinline__ bool tr_rk4(const double *__restrict__ B, const double *__restrict__ G, const TrArgs &p,
                                       size_t N, size_t sy, size_t sz, double sgn, const double r[3],
                                       const double k1[3], double q1, double s, double rn[3], double &dI) {
  const double hs = 0.5 * s, s6 = s / 6.0;
  double k2[3], k3[3], k4[3], q2, q3, q4;
  if (!tr_stage<kHasG>(B, G, p, N, sy, sz, sgn, r[0] + hs * k1[0], r[1] + hs * k1[1], r[2] + hs * k1[2], k2, q2))
    return false;
  if (!tr_stage<kHasG>(B, G, p, N, sy, sz, sgn, r[0] + hs * k2[0], r[1] + hs * k2[1], r[2] + hs * k2[2], k3, q3))
    return false;
  if (!tr_stage<kHasG>(B, G, p, N, sy, sz, sgn, r[0] + s * k3[0], r[1] + s * k3[1], r[2] + s * k3[2], k4, q4))
    return false;
#pragma unroll
  for (int d = 0; d < 3; ++d) rn[d] = r[d] + s6 * (((k1[d] + 2.0 * k2[d]) + 2.0 * k3[d]) + k4[d]);
  dI = s6 * (((q1 + 2.0 * q2) + 2.0 * q3) + q4);
  return true;
}

}  // namespace ndsm
