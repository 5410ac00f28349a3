// P = Omega x B and s = Omega.B at a node, and ddq's rows on values that are not in an array: shared by the force
// passes of the optimization method (optimize.hip, optimize_obs.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace ndsm {

// ddq's centred row on two values that are not in an array
__device__ __forceinline__ double dcen(double vm, double vp, double h) {
  const double half = 0.5;
  double d = 0.0;
  d = d + vm * (-1 * half / h);
  d = d + vp * (+1 * half / h);
  return d;
}

// ddq's one-sided row of the lower end plane on three values that are not in an array
__device__ __forceinline__ double dlow(double v0, double v1, double v2, double h) {
  const double half = 0.5;
  double d = 0.0;
  d = d + v0 * (-3 * half / h);
  d = d + v1 * (+4 * half / h);
  d = d + v2 * (-1 * half / h);
  return d;
}

struct PS {
  double px, py, pz, s;
};

// P = Omega x B and s = Omega.B at node c
__device__ __forceinline__ PS ps_at(const double *__restrict__ B, const double *__restrict__ O, size_t c, size_t N) {
  const double bx = B[c], by = B[c + N], bz = B[c + 2 * N];
  const double ox = O[c], oy = O[c + N], oz = O[c + 2 * N];
  PS r;
  r.px = oy * bz - oz * by;
  r.py = oz * bx - ox * bz;
  r.pz = ox * by - oy * bx;
  r.s = (ox * bx + oy * by) + oz * bz;
  return r;
}

}  // namespace ndsm
