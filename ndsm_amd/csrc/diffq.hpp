// Differences and weights shared by the field kernels (field.hip, project.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace ndsm {

// d/dq along one axis at index q of n (stride s): post.hip's ddq (derivq, ndsm_vector_potential.f90:852-870),
// the same operand order: centred inside, 3-point one-sided on the two end planes
__device__ __forceinline__ double ddq(const double *__restrict__ v, size_t c, int q, int n, size_t s, double h) {
  const double half = 0.5;
  double d = 0.0;
  if (q == 0) {
    d = d + v[c] * (-3 * half / h);
    d = d + v[c + s] * (+4 * half / h);
    d = d + v[c + 2 * s] * (-1 * half / h);
  } else if (q == n - 1) {
    d = d + v[c] * (+3 * half / h);
    d = d + v[c - s] * (-4 * half / h);
    d = d + v[c - 2 * s] * (+1 * half / h);
  } else {
    d = d + v[c - s] * (-1 * half / h);
    d = d + v[c + s] * (+1 * half / h);
  }
  return d;
}

// the same derivative with the one-sided rows written as differences from the end value,
//   q = 0:     (v1 - v0) * 2/h + (v2 - v0) * (-1/2h)       (= -3/2 v0 + 2 v1 - 1/2 v2, over h)
//   q = n - 1: (v-1 - v0) * (-2/h) + (v-2 - v0) * 1/2h
// and the centred rows of ddq bit for bit.  Equal to ddq in exact arithmetic; unlike ddq's three products it is
// exactly 0 wherever v is constant along the axis, so a field that is discretely solenoidal in exact
// arithmetic (each component independent of its own coordinate: the ABC field) has div_h = 0 in fp64 too.
__device__ __forceinline__ double ddq0(const double *__restrict__ v, size_t c, int q, int n, size_t s, double h) {
  const double half = 0.5;
  if (q == 0) {
    const double v0 = v[c];
    return (v[c + s] - v0) * (+4 * half / h) + (v[c + 2 * s] - v0) * (-1 * half / h);
  }
  if (q == n - 1) {
    const double v0 = v[c];
    return (v[c - s] - v0) * (-4 * half / h) + (v[c - 2 * s] - v0) * (+1 * half / h);
  }
  return ddq(v, c, q, n, s, h);
}

// trapezoid weight of index q of n along one axis: h inside, h/2 on both end planes
__device__ __forceinline__ double trap_w(int q, int n, double h) { return (q == 0 || q == n - 1) ? 0.5 * h : h; }

}  // namespace ndsm
