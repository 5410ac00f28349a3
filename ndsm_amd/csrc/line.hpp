// The field-line core shared by trace.hip and squash.hip: the mesh and box of a call, trilinear interpolation of a
// field (value, and value with gradient), the first face a chord meets and the snap of an exit point onto it, and the
// host-side checks and set-up common to the two entries.  The arithmetic is fixed fp64 expressions in a fixed order
// (no contraction: -ffp-contract=off), so the numpy restatement of the tests (tests/line_model.py) matches bit for
// bit:
//
//   cell, per axis d      u = (r_d - lo_d) / h_d,  c = clamp(floor(u), 0, n_d - 2),  f = u - c  (f is NOT clamped: a
//                         stage point outside the box extrapolates from the edge cell)
//   value, per component  d00 = v100 - v000, d10 = v110 - v010, d01 = v101 - v001, d11 = v111 - v011,
//                         c00 = v000 + fx d00, c10 = v010 + fx d10, c01 = v001 + fx d01, c11 = v011 + fx d11,
//                         e0 = c10 - c00, e1 = c11 - c01, c0 = c00 + fy e0, c1 = c01 + fy e1, dz = c1 - c0,
//                         v = c0 + fz dz
//   gradient              dx0 = d00 + fy (d10 - d00), dx1 = d01 + fy (d11 - d01),
//                         d/dx = (dx0 + fz (dx1 - dx0)) / hx, d/dy = (e0 + fz (e1 - e0)) / hy, d/dz = dz / hz
//   exit                  r' outside [lo, hi]: per axis that left, t_d = (face_d - r_d) / (r'_d - r_d); the smallest
//                         wins (x before y before z on a tie).  The kernel redoes the step from r with s = t ds; then
//                         r'_axis = face and the other two are clamped to the box.
//   box and step          hi_d = lo_d + (n_d - 1) h_d,  ds = step min(h)
#pragma once

#include <cmath>

#include "common.hpp"

namespace ndsm {

constexpr int kLineBlock = 64;           // one wave per block: a few thousand lanes spread over all CUs
constexpr int kLineMaxSteps = 1 << 24;   // the hard ceiling of max_steps

struct LineArgs {
  int n[3];
  double lo[3], hi[3], h[3];
  double ds;
  int max_steps;
  int nseeds;
};

struct LineCell {
  size_t base;
  double fx, fy, fz;
};

__device__ __forceinline__ LineCell line_cell(const LineArgs &p, double x, double y, double z) {
  const double ux = (x - p.lo[0]) / p.h[0];
  const double uy = (y - p.lo[1]) / p.h[1];
  const double uz = (z - p.lo[2]) / p.h[2];
  // (the points that reach here are within one step of the box, so the conversions cannot overflow)
  const double cx = fmin(fmax(floor(ux), 0.0), (double)(p.n[0] - 2));
  const double cy = fmin(fmax(floor(uy), 0.0), (double)(p.n[1] - 2));
  const double cz = fmin(fmax(floor(uz), 0.0), (double)(p.n[2] - 2));
  LineCell c;
  c.fx = ux - cx;
  c.fy = uy - cy;
  c.fz = uz - cz;
  c.base = (size_t)(int)cx + (size_t)p.n[0] * ((size_t)(int)cy + (size_t)p.n[1] * (size_t)(int)cz);
  return c;
}

// the 8 corners of the three components of F at cell c: all 24 loads are issued before the first use
__device__ __forceinline__ void line_gather(const double *__restrict__ F, size_t N, size_t sy, size_t sz,
                                            const LineCell &c, double v[3][8]) {
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const double *__restrict__ q = F + (size_t)m * N + c.base;
    v[m][0] = q[0];
    v[m][1] = q[1];
    v[m][2] = q[sy];
    v[m][3] = q[sy + 1];
    v[m][4] = q[sz];
    v[m][5] = q[sz + 1];
    v[m][6] = q[sz + sy];
    v[m][7] = q[sz + sy + 1];
  }
}

__device__ __forceinline__ double line_lerp3(const double v[8], const LineCell &c) {
  const double c00 = v[0] + c.fx * (v[1] - v[0]);
  const double c10 = v[2] + c.fx * (v[3] - v[2]);
  const double c01 = v[4] + c.fx * (v[5] - v[4]);
  const double c11 = v[6] + c.fx * (v[7] - v[6]);
  const double c0 = c00 + c.fy * (c10 - c00);
  const double c1 = c01 + c.fy * (c11 - c01);
  return c0 + c.fz * (c1 - c0);
}

// value (the bits of line_lerp3) and gradient of the trilinear interpolant of one component (the quotients by h are
// formed, not products by 1 / h)
__device__ __forceinline__ double line_lerp3_grad(const double v[8], const LineCell &c, const LineArgs &p,
                                                  double g[3]) {
  const double d00 = v[1] - v[0], d10 = v[3] - v[2], d01 = v[5] - v[4], d11 = v[7] - v[6];
  const double c00 = v[0] + c.fx * d00;
  const double c10 = v[2] + c.fx * d10;
  const double c01 = v[4] + c.fx * d01;
  const double c11 = v[6] + c.fx * d11;
  const double e0 = c10 - c00, e1 = c11 - c01;
  const double c0 = c00 + c.fy * e0;
  const double c1 = c01 + c.fy * e1;
  const double dz = c1 - c0;
  const double dx0 = d00 + c.fy * (d10 - d00);
  const double dx1 = d01 + c.fy * (d11 - d01);
  g[0] = (dx0 + c.fz * (dx1 - dx0)) / p.h[0];
  g[1] = (e0 + c.fz * (e1 - e0)) / p.h[1];
  g[2] = dz / p.h[2];
  return c0 + c.fz * dz;
}

// the same value and the gradient with respect to the cell's fractions (fx, fy, fz): line_lerp3_grad's expressions
// without the quotients by h (nulls.hip iterates in the fractions)
__device__ __forceinline__ double line_lerp3_fgrad(const double v[8], const LineCell &c, double g[3]) {
  const double d00 = v[1] - v[0], d10 = v[3] - v[2], d01 = v[5] - v[4], d11 = v[7] - v[6];
  const double c00 = v[0] + c.fx * d00;
  const double c10 = v[2] + c.fx * d10;
  const double c01 = v[4] + c.fx * d01;
  const double c11 = v[6] + c.fx * d11;
  const double e0 = c10 - c00, e1 = c11 - c01;
  const double c0 = c00 + c.fy * e0;
  const double c1 = c01 + c.fy * e1;
  const double dz = c1 - c0;
  const double dx0 = d00 + c.fy * (d10 - d00);
  const double dx1 = d01 + c.fy * (d11 - d01);
  g[0] = dx0 + c.fz * (dx1 - dx0);
  g[1] = e0 + c.fz * (e1 - e0);
  g[2] = dz;
  return c0 + c.fz * dz;
}

// the first face the chord r -> rn meets: its NDSMK_TRACE_* code and t, or 0 (t = 2) when rn is inside the box
__device__ __forceinline__ int line_first_face(const LineArgs &p, const double r[3], const double rn[3], double &t) {
  int face = 0;
  t = 2.0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    double td = 2.0;
    int fd = 0;
    if (rn[d] < p.lo[d]) {
      td = (p.lo[d] - r[d]) / (rn[d] - r[d]);
      fd = NDSMK_TRACE_XLO + 2 * d;
    } else if (rn[d] > p.hi[d]) {
      td = (p.hi[d] - r[d]) / (rn[d] - r[d]);
      fd = NDSMK_TRACE_XLO + 2 * d + 1;
    }
    if (td < t) {
      t = td;
      face = fd;
    }
  }
  return face;
}

// the exit point: rn on `face` exactly along the face's axis, clamped to the box along the other two
__device__ __forceinline__ void line_snap(const LineArgs &p, int face, const double rn[3], double r[3]) {
  const int ax = (face - NDSMK_TRACE_XLO) >> 1;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double fv = ((face - NDSMK_TRACE_XLO) & 1) ? p.hi[d] : p.lo[d];
    r[d] = (d == ax) ? fv : fmin(fmax(rn[d], p.lo[d]), p.hi[d]);
  }
}

// the basis (e1, e2) of the plane perpendicular to the unit vector w, from the axis j of the smallest |w_d| (the
// lowest on a tie): u = axis_j - w_j w, e1 = u / |u|, e2 = w x e1 (the fan of a null from its normal: skeleton.hip,
// separators.hip; squash.hip states the same rule for its seed frame)
__device__ __forceinline__ void line_fan_basis(const double w[3], double e1[3], double e2[3]) {
  int j = 0;
  double small = fabs(w[0]), wj = w[0];
  if (fabs(w[1]) < small) j = 1, small = fabs(w[1]), wj = w[1];
  if (fabs(w[2]) < small) j = 2, wj = w[2];
  double u[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) u[d] = (d == j ? 1.0 : 0.0) - wj * w[d];
  const double un = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
#pragma unroll
  for (int d = 0; d < 3; ++d) e1[d] = u[d] / un;
  e2[0] = w[1] * e1[2] - w[2] * e1[1];
  e2[1] = w[2] * e1[0] - w[0] * e1[2];
  e2[2] = w[0] * e1[1] - w[1] * e1[0];
}

// the mesh, the box and the step of a call into p (the shape and the spacings have been checked)
inline void line_mesh(const int32_t *n3, const double *lo3, const double *h_dq3, double step, int max_steps,
                      LineArgs &p) {
  for (int d = 0; d < 3; ++d) {
    p.n[d] = n3[d];
    p.lo[d] = lo3[d];
    p.h[d] = h_dq3[d];
    p.hi[d] = lo3[d] + (double)(n3[d] - 1) * h_dq3[d];
  }
  p.ds = step * fmin(fmin(h_dq3[0], h_dq3[1]), h_dq3[2]);
  p.max_steps = max_steps < kLineMaxSteps ? max_steps : kLineMaxSteps;
}

// The checks and the set-up common to the line entries, after NDSM_REQUIRE_READY: `usage` names the entry and its
// scalar ranges (own_ok: the entry's own scalar is in range), arrays_ok: every required array is there (looked at
// only with seeds), per_seed: lines per seed.  0 with p filled, or with nseeds == 0 (nothing to launch); else the
// error code.
inline int line_args(const char *usage, bool own_ok, bool arrays_ok, const int32_t *n3, const double *lo3,
                     const double *h_dq3, int nseeds, double step, int max_steps, int per_seed, LineArgs &p) {
  if (!(step > 0.0) || !(step <= 1.0e300) || max_steps < 1 || !own_ok || nseeds < 0)
    return fail(NDSMK_EVALUE, usage, __FILE__, __LINE__);
  if (nseeds == 0) return 0;
  NDSM_CHECK_ARG(arrays_ok);
  NDSM_CHECK_ARG(n3[0] >= 2 && n3[1] >= 2 && n3[2] >= 2 && h_dq3[0] > 0.0 && h_dq3[1] > 0.0 && h_dq3[2] > 0.0);
  NDSM_CHECK_ARG((size_t)nseeds * (size_t)per_seed <= (size_t)0x7fffffff);
  line_mesh(n3, lo3, h_dq3, step, max_steps, p);
  p.nseeds = nseeds;
  return 0;
}

}  // namespace ndsm
