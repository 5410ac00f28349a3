// Field-line tracing and line integrals on the device (DESIGN.md "Field-line tracing and field-line helicity").
// One lane per (seed, direction): a latency-bound gather with a data-dependent trip count per lane, unlike the
// plane-streaming kernels of the other files.  The arithmetic is fixed fp64 expressions in a fixed order (no
// contraction: -ffp-contract=off), so a numpy restatement matches bit for bit:
//
//   interpolation, per axis d   u = (r_d - lo_d) / h_d,  c = clamp(floor(u), 0, n_d - 2),  f = u - c  (f is NOT
//                               clamped: a stage point outside the box extrapolates from the edge cell)
//                per component  c00 = v000 + fx (v100 - v000), c10 = v010 + fx (v110 - v010),
//                               c01 = v001 + fx (v101 - v001), c11 = v011 + fx (v111 - v011),
//                               c0 = c00 + fy (c10 - c00), c1 = c01 + fy (c11 - c01), v = c0 + fz (c1 - c0)
//   stage at p                  b = B(p), m = sqrt((bx bx + by by) + bz bz); not m > 0: the line ends "null";
//                               e = b / m, k = sgn e, q = (Gx ex + Gy ey) + Gz ez   (sgn = +1 forward, -1 backward;
//                               q has no sgn: the integral runs in the direction of B for both directions)
//   RK4 step of length s from r k1 = k(r), k2 = k(r + (0.5 s) k1), k3 = k(r + (0.5 s) k2), k4 = k(r + s k3),
//                               r' = r + (s / 6) (((k1 + 2 k2) + 2 k3) + k4), dI = (s / 6) (((q1 + 2 q2) + 2 q3) + q4)
//   exit                        r' outside [lo, hi]: per axis that left, t_d = (face_d - r_d) / (r'_d - r_d); the
//                               smallest wins (x before y before z on a tie); the step is redone from r with
//                               s = t ds (k1, q1 kept), then r'_axis = face and the other two are clamped.
// Every lane's loop is bounded by max_steps.
#include "common.hpp"

namespace {

constexpr int kTrBlock = 64;             // one wave per block: a few thousand lanes spread over all CUs
constexpr int kTrMaxSteps = 1 << 24;     // the hard ceiling of max_steps

struct TrArgs {
  int n[3];
  double lo[3], hi[3], h[3];
  double ds;
  int max_steps;
  int nseeds;
  int ndir;       // 1 or 2
  int sgn0;       // direction of the first block of lanes: +1 or -1 (both: +1, the second block is -1)
};

struct TrCell {
  size_t base;
  double fx, fy, fz;
};

__device__ __forceinline__ TrCell tr_cell(const TrArgs &p, double x, double y, double z) {
  const double ux = (x - p.lo[0]) / p.h[0];
  const double uy = (y - p.lo[1]) / p.h[1];
  const double uz = (z - p.lo[2]) / p.h[2];
  // (the points that reach here are within one step of the box, so the conversions cannot overflow)
  const double cx = fmin(fmax(floor(ux), 0.0), (double)(p.n[0] - 2));
  const double cy = fmin(fmax(floor(uy), 0.0), (double)(p.n[1] - 2));
  const double cz = fmin(fmax(floor(uz), 0.0), (double)(p.n[2] - 2));
  TrCell c;
  c.fx = ux - cx;
  c.fy = uy - cy;
  c.fz = uz - cz;
  c.base = (size_t)(int)cx + (size_t)p.n[0] * ((size_t)(int)cy + (size_t)p.n[1] * (size_t)(int)cz);
  return c;
}

// the 8 corners of the three components of F at cell c: all 24 loads are issued before the first use
__device__ __forceinline__ void tr_gather(const double *__restrict__ F, size_t N, size_t sy, size_t sz, const TrCell &c,
                                          double v[3][8]) {
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

__device__ __forceinline__ double tr_lerp3(const double v[8], const TrCell &c) {
  const double c00 = v[0] + c.fx * (v[1] - v[0]);
  const double c10 = v[2] + c.fx * (v[3] - v[2]);
  const double c01 = v[4] + c.fx * (v[5] - v[4]);
  const double c11 = v[6] + c.fx * (v[7] - v[6]);
  const double c0 = c00 + c.fy * (c10 - c00);
  const double c1 = c01 + c.fy * (c11 - c01);
  return c0 + c.fz * (c1 - c0);
}

// one stage at (x,y,z): k[3] = sgn B/|B|, q = G . B/|B| (0 without G).  false: |B| is not > 0 (zero or NaN).
template <bool kHasG>
__device__ __forceinline__ bool tr_stage(const double *__restrict__ B, const double *__restrict__ G, const TrArgs &p,
                                         size_t N, size_t sy, size_t sz, double sgn, double x, double y, double z,
                                         double k[3], double &q) {
  const TrCell c = tr_cell(p, x, y, z);
  double vb[3][8], vg[3][8];
  tr_gather(B, N, sy, sz, c, vb);
  if (kHasG) tr_gather(G, N, sy, sz, c, vg);
  const double bx = tr_lerp3(vb[0], c), by = tr_lerp3(vb[1], c), bz = tr_lerp3(vb[2], c);
  const double m = sqrt((bx * bx + by * by) + bz * bz);
  q = 0.0;
  if (!(m > 0.0)) return false;
  const double ex = bx / m, ey = by / m, ez = bz / m;
  k[0] = sgn * ex;
  k[1] = sgn * ey;
  k[2] = sgn * ez;
  if (kHasG) {
    const double gx = tr_lerp3(vg[0], c), gy = tr_lerp3(vg[1], c), gz = tr_lerp3(vg[2], c);
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

// lane l: seed l % nseeds, direction block l / nseeds.  Outputs per lane: ends[3 l .. 3 l + 2], length[l],
// integral[l], status[l], nsteps[l].
template <bool kHasG>
__global__ __launch_bounds__(kTrBlock) void trace_k(const double *__restrict__ B, const double *__restrict__ G,
                                                    const double *__restrict__ seeds, double *__restrict__ ends,
                                                    double *__restrict__ length, double *__restrict__ integral,
                                                    int32_t *__restrict__ status, int32_t *__restrict__ nsteps,
                                                    TrArgs p) {
  const size_t l = (size_t)blockIdx.x * kTrBlock + threadIdx.x;
  const size_t nl = (size_t)p.nseeds * (size_t)p.ndir;
  if (l >= nl) return;
  const size_t is = l % (size_t)p.nseeds;
  const double sgn = (l / (size_t)p.nseeds == 0) ? (double)p.sgn0 : -1.0;
  const size_t sy = (size_t)p.n[0], sz = (size_t)p.n[0] * (size_t)p.n[1];
  const size_t N = sz * (size_t)p.n[2];

  double r[3] = {seeds[3 * is], seeds[3 * is + 1], seeds[3 * is + 2]};
  double len = 0.0, I = 0.0;
  int st = NDSMK_TRACE_UNFINISHED, ns = 0;
  bool inside = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) inside = inside && (r[d] >= p.lo[d]) && (r[d] <= p.hi[d]);
  if (!inside) {
    st = NDSMK_TRACE_OUTSIDE;
  } else {
    for (int it = 0; it < p.max_steps; ++it) {
      double k1[3], q1, rn[3], dI;
      if (!tr_stage<kHasG>(B, G, p, N, sy, sz, sgn, r[0], r[1], r[2], k1, q1) ||
          !tr_rk4<kHasG>(B, G, p, N, sy, sz, sgn, r, k1, q1, p.ds, rn, dI)) {
        st = NDSMK_TRACE_NULL;
        break;
      }
      // the first face the chord r -> rn meets, if rn is outside
      double t = 2.0;
      int face = 0;
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
      if (face == 0) {
        r[0] = rn[0], r[1] = rn[1], r[2] = rn[2];
        len = len + p.ds;
        I = I + dI;
        ns = it + 1;
        continue;
      }
      // the step is redone with the length that reaches the face; stage 1 is the same
      const double s = t * p.ds;
      if (!tr_rk4<kHasG>(B, G, p, N, sy, sz, sgn, r, k1, q1, s, rn, dI)) {
        st = NDSMK_TRACE_NULL;
        break;
      }
      const int ax = (face - NDSMK_TRACE_XLO) >> 1;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double fv = ((face - NDSMK_TRACE_XLO) & 1) ? p.hi[d] : p.lo[d];
        r[d] = (d == ax) ? fv : fmin(fmax(rn[d], p.lo[d]), p.hi[d]);
      }
      len = len + s;
      I = I + dI;
      ns = it + 1;
      st = face;
      break;
    }
  }
  ends[3 * l] = r[0];
  ends[3 * l + 1] = r[1];
  ends[3 * l + 2] = r[2];
  length[l] = len;
  integral[l] = I;
  status[l] = st;
  nsteps[l] = ns;
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
  if (!(step > 0.0) || !(step <= 1.0e300) || max_steps < 1 || direction < -1 || direction > 1 || nseeds < 0)
    return ndsm::fail(NDSMK_EVALUE, "trace: step > 0 (finite), max_steps >= 1, direction in -1, 0, 1 and nseeds >= 0",
                      __FILE__, __LINE__);
  if (nseeds == 0) return 0;
  NDSM_CHECK_ARG(B && seeds && ends && length && integral && status && nsteps);
  NDSM_CHECK_ARG(n3[0] >= 2 && n3[1] >= 2 && n3[2] >= 2 && h_dq3[0] > 0.0 && h_dq3[1] > 0.0 && h_dq3[2] > 0.0);
  TrArgs p;
  for (int d = 0; d < 3; ++d) {
    p.n[d] = n3[d];
    p.lo[d] = lo3[d];
    p.h[d] = h_dq3[d];
    p.hi[d] = lo3[d] + (double)(n3[d] - 1) * h_dq3[d];
  }
  p.ds = step * fmin(fmin(h_dq3[0], h_dq3[1]), h_dq3[2]);
  p.max_steps = max_steps < kTrMaxSteps ? max_steps : kTrMaxSteps;
  p.nseeds = nseeds;
  p.ndir = direction == 0 ? 2 : 1;
  p.sgn0 = direction < 0 ? -1 : 1;
  const size_t nl = (size_t)nseeds * (size_t)p.ndir;
  NDSM_CHECK_ARG(nl <= (size_t)0x7fffffff);
  const unsigned nb = (unsigned)((nl + kTrBlock - 1) / kTrBlock);
  hipStream_t s = ndsm::stream();
  if (G)
    hipLaunchKernelGGL(trace_k<true>, dim3(nb), dim3(kTrBlock), 0, s, B, G, seeds, ends, length, integral, status,
                       nsteps, p);
  else
    hipLaunchKernelGGL(trace_k<false>, dim3(nb), dim3(kTrBlock), 0, s, B, G, seeds, ends, length, integral, status,
                       nsteps, p);
  NDSM_LAUNCH_CHECK();
  return 0;
}
