// Squashing factor Q and line integrals (twist) on the device (DESIGN.md "Squashing factor and twist").  The method of
// Scott, Pontin & Hornig (2017): two deviation vectors U, V are carried along the field line with the gradient of
// the field, and Q at the seed follows from them at the two feet of the one line through it.  One lane per (seed,
// direction), the two lanes of a seed next to each other in a wave; the forward lane combines the two ends.  As in
// trace.hip the arithmetic is fixed fp64 expressions in a fixed order (-ffp-contract=off), restated in numpy by the
// tests bit for bit.  The cell, gather, value and gradient of the trilinear interpolant, the first-face search and the
// snap of the exit point are line.hpp's (the specification is at the top of that file); here:
//
//   stage at (p, U, V)    b = B(p), M = grad B(p), m = sqrt((bx bx + by by) + bz bz); not m > 0: "null";
//                         e = b / m, k_r = sgn e, k_U,c = sgn (((M_c0 U_0 + M_c1 U_1) + M_c2 U_2) / m), k_V likewise,
//                         q = (Gx ex + Gy ey) + Gz ez, divided by m for integrand 1 (no sgn)
//   RK4 step of length s  stage 2 at y + (0.5 s) k1, 3 at y + (0.5 s) k2, 4 at y + s k3 for all of y = (r, U, V);
//                         y' = y + (s / 6) (((k1 + 2 k2) + 2 k3) + k4), dI likewise, the sum formed as the stages
//                         complete
//   exit                  r' outside: the step is redone with s = t ds, t of the first face, then twice
//                         s = s (face - r_ax) / (r'_ax - r_ax) (skipped when r'_ax == r_ax) and redone; snap, clamp
// Every lane's loop is bounded by max_steps (and by four passes over a step).
//
// The perpendicular squashing factor (DESIGN.md "Perpendicular squashing factor"; kPerp) differs in the epilogue only:
// the same U, V at the same two ends are projected onto the plane perpendicular to B at the end instead of onto the
// face along B, and |B| at the two ends takes the place of |B_n|:
//   end                   me = sqrt((Bx Bx + By By) + Bz Bz) of B at the end, e = B / me; du = (U_x e_x + U_y e_y) +
//                         U_z e_z, dv likewise; Up = U - du e, Vp = V - dv e; puu, pvv, puv their dot products
//   seed                  Qperp = (((puu_F pvv_B + puu_B pvv_F) - 2 (puv_F puv_B)) me_F) me_B / |B_s|^2
#include "line.hpp"

namespace {

using namespace ndsm;

struct SqArgs : LineArgs {
  int integrand;
};

// the state of a line and its slopes: r, U, V and the integral
struct SqVec {
  double r[3], U[3], V[3], I;
};

// one stage at y = (r, U, V): the ten slopes k; b[3] and m2 = |B|^2 there.  false: |B| is not > 0 (zero or NaN).
template <bool kHasG>
__device__ __forceinline__ bool sq_stage(const double *__restrict__ B, const double *__restrict__ G, const SqArgs &p,
                                         size_t N, size_t sy, size_t sz, double sgn, const double r[3],
                                         const double U[3], const double V[3], SqVec &k, double b[3], double &m2) {
  const LineCell c = line_cell(p, r[0], r[1], r[2]);
  double vb[3][8], vg[3][8];
  line_gather(B, N, sy, sz, c, vb);
  if (kHasG) line_gather(G, N, sy, sz, c, vg);
  double M[3][3];
#pragma unroll
  for (int d = 0; d < 3; ++d) b[d] = line_lerp3_grad(vb[d], c, p, M[d]);
  m2 = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
  const double m = sqrt(m2);
  k.I = 0.0;
  if (!(m > 0.0)) return false;
  const double ex = b[0] / m, ey = b[1] / m, ez = b[2] / m;
  k.r[0] = sgn * ex;
  k.r[1] = sgn * ey;
  k.r[2] = sgn * ez;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    k.U[d] = sgn * (((M[d][0] * U[0] + M[d][1] * U[1]) + M[d][2] * U[2]) / m);
    k.V[d] = sgn * (((M[d][0] * V[0] + M[d][1] * V[1]) + M[d][2] * V[2]) / m);
  }
  if (kHasG) {
    const double gx = line_lerp3(vg[0], c), gy = line_lerp3(vg[1], c), gz = line_lerp3(vg[2], c);
    double q = (gx * ex + gy * ey) + gz * ez;
    if (p.integrand == 1) q = q / m;
    k.I = q;
  }
  return true;
}

// stages 2-4 and the sums of one RK4 step of length s from y (k1 given): yn = y + (s / 6) (((k1 + 2 k2) + 2 k3) + k4),
// the sum formed as the stages complete; yn.I is the increment of the integral.  false: a stage met a null.
template <bool kHasG>
__device__ __forceinline__ bool sq_rk4(const double *__restrict__ B, const double *__restrict__ G, const SqArgs &p,
                                       size_t N, size_t sy, size_t sz, double sgn, const SqVec &y, const SqVec &k1,
                                       double s, SqVec &yn) {
  const double hs = 0.5 * s, s6 = s / 6.0;
  SqVec k, acc;
  double t[9], b[3], m2;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    t[d] = y.r[d] + hs * k1.r[d];
    t[3 + d] = y.U[d] + hs * k1.U[d];
    t[6 + d] = y.V[d] + hs * k1.V[d];
  }
  if (!sq_stage<kHasG>(B, G, p, N, sy, sz, sgn, t, t + 3, t + 6, k, b, m2)) return false;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    acc.r[d] = k1.r[d] + 2.0 * k.r[d];
    acc.U[d] = k1.U[d] + 2.0 * k.U[d];
    acc.V[d] = k1.V[d] + 2.0 * k.V[d];
    t[d] = y.r[d] + hs * k.r[d];
    t[3 + d] = y.U[d] + hs * k.U[d];
    t[6 + d] = y.V[d] + hs * k.V[d];
  }
  acc.I = k1.I + 2.0 * k.I;
  if (!sq_stage<kHasG>(B, G, p, N, sy, sz, sgn, t, t + 3, t + 6, k, b, m2)) return false;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    acc.r[d] = acc.r[d] + 2.0 * k.r[d];
    acc.U[d] = acc.U[d] + 2.0 * k.U[d];
    acc.V[d] = acc.V[d] + 2.0 * k.V[d];
    t[d] = y.r[d] + s * k.r[d];
    t[3 + d] = y.U[d] + s * k.U[d];
    t[6 + d] = y.V[d] + s * k.V[d];
  }
  acc.I = acc.I + 2.0 * k.I;
  if (!sq_stage<kHasG>(B, G, p, N, sy, sz, sgn, t, t + 3, t + 6, k, b, m2)) return false;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    yn.r[d] = y.r[d] + s6 * (acc.r[d] + k.r[d]);
    yn.U[d] = y.U[d] + s6 * (acc.U[d] + k.U[d]);
    yn.V[d] = y.V[d] + s6 * (acc.V[d] + k.V[d]);
  }
  yn.I = s6 * (acc.I + k.I);
  return true;
}

// a[ax] of a 3-vector without dynamic indexing (dynamic indexing would put the vector into scratch memory)
__device__ __forceinline__ double sq_pick(const double a[3], int ax) { return ax == 0 ? a[0] : (ax == 1 ? a[1] : a[2]); }

// lane l: seed l / 2, direction l % 2 (0 forward, 1 backward).  Line j = direction * nseeds + seed of the outputs:
// ends[3 j .. 3 j + 2], length[j], integral[j], status[j], nsteps[j]; q[seed] (kPerp: and qperp[seed]) from the forward
// lane.  kPerp false: qperp is not looked at.
template <bool kHasG, bool kPerp>
__global__ __launch_bounds__(kLineBlock) void squash_k(const double *__restrict__ B, const double *__restrict__ G,
                                                       const double *__restrict__ seeds, double *__restrict__ qout,
                                                       double *__restrict__ ends, double *__restrict__ length,
                                                       double *__restrict__ integral, int32_t *__restrict__ status,
                                                       int32_t *__restrict__ nsteps, SqArgs p,
                                                       double *__restrict__ qperp) {
  const size_t l = (size_t)blockIdx.x * kLineBlock + threadIdx.x;
  const bool live = l < 2 * (size_t)p.nseeds;
  const size_t is = live ? l >> 1 : 0;            // (a lane past the end follows seed 0 and writes nothing)
  const int back = (int)(l & 1);
  const double sgn = back ? -1.0 : 1.0;
  const size_t sy = (size_t)p.n[0], sz = (size_t)p.n[0] * (size_t)p.n[1];
  const size_t N = sz * (size_t)p.n[2];

  SqVec y;
  y.r[0] = seeds[3 * is], y.r[1] = seeds[3 * is + 1], y.r[2] = seeds[3 * is + 2];
#pragma unroll
  for (int d = 0; d < 3; ++d) y.U[d] = y.V[d] = 0.0;
  y.I = 0.0;
  double len = 0.0, bs2 = 0.0;
  int st = NDSMK_TRACE_UNFINISHED, ns = 0;
  bool inside = live;
#pragma unroll
  for (int d = 0; d < 3; ++d) inside = inside && (y.r[d] >= p.lo[d]) && (y.r[d] <= p.hi[d]);
  if (!inside) {
    st = NDSMK_TRACE_OUTSIDE;
  } else {
    {
      // the frame at the seed: U0 perpendicular to e = B/|B| from the axis of the smallest |e_d|, V0 = e x U0 (at a
      // null they stay 0 and the first stage below ends the line)
      const LineCell c = line_cell(p, y.r[0], y.r[1], y.r[2]);
      double vb[3][8];
      line_gather(B, N, sy, sz, c, vb);
      const double b[3] = {line_lerp3(vb[0], c), line_lerp3(vb[1], c), line_lerp3(vb[2], c)};
      bs2 = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
      const double m = sqrt(bs2);
      if (m > 0.0) {
        const double e[3] = {b[0] / m, b[1] / m, b[2] / m};
        int j = 0;
        double small = fabs(e[0]);
        if (fabs(e[1]) < small) j = 1, small = fabs(e[1]);
        if (fabs(e[2]) < small) j = 2;
        const double ej = sq_pick(e, j);
        double w[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) w[d] = (d == j ? 1.0 : 0.0) - ej * e[d];
        const double wn = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
        for (int d = 0; d < 3; ++d) y.U[d] = w[d] / wn;
        y.V[0] = e[1] * y.U[2] - e[2] * y.U[1];
        y.V[1] = e[2] * y.U[0] - e[0] * y.U[2];
        y.V[2] = e[0] * y.U[1] - e[1] * y.U[0];
      }
    }
    for (int it = 0; it < p.max_steps; ++it) {
      SqVec k1, yn;
      double b[3], m2;
      const bool ok = sq_stage<kHasG>(B, G, p, N, sy, sz, sgn, y.r, y.U, y.V, k1, b, m2);
      if (!ok) {
        st = NDSMK_TRACE_NULL;
        break;
      }
      // pass 0: the full step; if its end is outside, pass 1 redoes it with s = t ds, passes 2 and 3 refine s
      double s = p.ds, fv = 0.0;
      int face = 0, ax = 0;
      bool null = false;
      for (int pass = 0; pass < 4; ++pass) {
        if (!sq_rk4<kHasG>(B, G, p, N, sy, sz, sgn, y, k1, s, yn)) {
          null = true;
          break;
        }
        if (pass == 0) {
          double t;
          face = line_first_face(p, y.r, yn.r, t);
          if (face == 0) break;
          ax = (face - NDSMK_TRACE_XLO) >> 1;
          fv = ((face - NDSMK_TRACE_XLO) & 1) ? sq_pick(p.hi, ax) : sq_pick(p.lo, ax);
          s = t * p.ds;
        } else if (pass < 3) {
          const double r0 = sq_pick(y.r, ax);
          const double den = sq_pick(yn.r, ax) - r0;
          if (den == 0.0) break;          // nothing to refine with (a later pass would meet the same)
          s = s * (fv - r0) / den;
        }
      }
      if (null) {
        st = NDSMK_TRACE_NULL;
        break;
      }
      y.I = y.I + yn.I;
      ns = it + 1;
#pragma unroll
      for (int d = 0; d < 3; ++d) y.U[d] = yn.U[d], y.V[d] = yn.V[d];
      if (face == 0) {
        y.r[0] = yn.r[0], y.r[1] = yn.r[1], y.r[2] = yn.r[2];
        len = len + p.ds;
        continue;
      }
      line_snap(p, face, yn.r, y.r);
      len = len + s;
      st = face;
      break;
    }
  }
  // this end's part of Q: the deviation vectors projected onto the face along B there
  const bool onface = st >= NDSMK_TRACE_XLO && st <= NDSMK_TRACE_ZHI;
  double uu = 0.0, vv = 0.0, uv = 0.0, bn = 0.0;
  double puu = 0.0, pvv = 0.0, puv = 0.0, me = 0.0;
  if (onface) {
    const int ax = (st - NDSMK_TRACE_XLO) >> 1;
    const LineCell c = line_cell(p, y.r[0], y.r[1], y.r[2]);
    double vb[3][8];
    line_gather(B, N, sy, sz, c, vb);
    const double be[3] = {line_lerp3(vb[0], c), line_lerp3(vb[1], c), line_lerp3(vb[2], c)};
    const double bax = sq_pick(be, ax);
    const double fu = sq_pick(y.U, ax) / bax, fw = sq_pick(y.V, ax) / bax;
    double Ut[3], Vt[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      Ut[d] = y.U[d] - fu * be[d];
      Vt[d] = y.V[d] - fw * be[d];
    }
    uu = (Ut[0] * Ut[0] + Ut[1] * Ut[1]) + Ut[2] * Ut[2];
    vv = (Vt[0] * Vt[0] + Vt[1] * Vt[1]) + Vt[2] * Vt[2];
    uv = (Ut[0] * Vt[0] + Ut[1] * Vt[1]) + Ut[2] * Vt[2];
    bn = fabs(bax);
    if (kPerp) {
      // and of Qperp: the same vectors projected onto the plane perpendicular to B there
      me = sqrt((be[0] * be[0] + be[1] * be[1]) + be[2] * be[2]);
      const double e[3] = {be[0] / me, be[1] / me, be[2] / me};
      const double du = (y.U[0] * e[0] + y.U[1] * e[1]) + y.U[2] * e[2];
      const double dv = (y.V[0] * e[0] + y.V[1] * e[1]) + y.V[2] * e[2];
      double Up[3], Vp[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        Up[d] = y.U[d] - du * e[d];
        Vp[d] = y.V[d] - dv * e[d];
      }
      puu = (Up[0] * Up[0] + Up[1] * Up[1]) + Up[2] * Up[2];
      pvv = (Vp[0] * Vp[0] + Vp[1] * Vp[1]) + Vp[2] * Vp[2];
      puv = (Up[0] * Vp[0] + Up[1] * Vp[1]) + Up[2] * Vp[2];
    }
  }
  // the partner lane (the other direction of the same seed) is the neighbour in the wave: every lane of the wave
  // arrives here, whatever its line did
  const double uuo = __shfl_xor(uu, 1), vvo = __shfl_xor(vv, 1), uvo = __shfl_xor(uv, 1), bno = __shfl_xor(bn, 1);
  const int sto = __shfl_xor(st, 1);
  double puuo = 0.0, pvvo = 0.0, puvo = 0.0, meo = 0.0;
  if (kPerp) puuo = __shfl_xor(puu, 1), pvvo = __shfl_xor(pvv, 1), puvo = __shfl_xor(puv, 1), meo = __shfl_xor(me, 1);
  if (!live) return;
  const size_t j = (size_t)back * (size_t)p.nseeds + is;
  ends[3 * j] = y.r[0];
  ends[3 * j + 1] = y.r[1];
  ends[3 * j + 2] = y.r[2];
  length[j] = len;
  integral[j] = y.I;
  status[j] = st;
  nsteps[j] = ns;
  if (!back) {
    // this lane holds the forward end F, the partner the backward end B
    double q = __builtin_nan("");
    const bool oface = sto >= NDSMK_TRACE_XLO && sto <= NDSMK_TRACE_ZHI;
    if (onface && oface && bn > 0.0 && bno > 0.0) {
      const double num = (uu * vvo + uuo * vv) - 2.0 * (uv * uvo);
      q = ((num * bn) * bno) / bs2;
    }
    qout[is] = q;
    if (kPerp) {
      // (no b_n > 0 here: a line that arrives tangent to its face has a Qperp but no Q)
      double qp = __builtin_nan("");
      if (onface && oface && me > 0.0 && meo > 0.0) {
        const double num = (puu * pvvo + puuo * pvv) - 2.0 * (puv * puvo);
        qp = ((num * me) * meo) / bs2;
      }
      qperp[is] = qp;
    }
  }
}

}  // namespace

// Squashing factor Q of B (nx,ny,nz,3) at nseeds seeds (3 each, physical coordinates), with the two ends of the line
// through each seed and the line integral of G (nullptr: none, integrals 0; integrand 0: G.B/|B|, 1: G.B/|B|^2) per
// direction.  lo3, h_dq3: the mesh's first point and spacing per axis; step in units of min(h).  All arrays DEVICE
// arrays; q holds nseeds values, the others 2 nseeds lines (the forward block, then the backward block).
// Asynchronous.
extern "C" int ndsmk_squash(const double *B, const double *G, int integrand, const int32_t *n3, const double *lo3,
                            const double *h_dq3, int nseeds, const double *seeds, double step, int max_steps,
                            double *q, double *ends, double *length, double *integral, int32_t *status,
                            int32_t *nsteps) {
  NDSM_REQUIRE_READY();
  SqArgs p;
  p.integrand = integrand;
  const int rc = line_args("squash: step > 0 (finite), max_steps >= 1, integrand in 0, 1 and nseeds >= 0",
                           integrand >= 0 && integrand <= 1,
                           B && seeds && q && ends && length && integral && status && nsteps, n3, lo3, h_dq3, nseeds,
                           step, max_steps, 2, p);
  if (rc != 0 || nseeds == 0) return rc;
  const size_t nl = 2 * (size_t)nseeds;
  const unsigned nb = (unsigned)((nl + kLineBlock - 1) / kLineBlock);
  hipStream_t s = ndsm::stream();
  double *const none = nullptr;
  if (G)
    hipLaunchKernelGGL((squash_k<true, false>), dim3(nb), dim3(kLineBlock), 0, s, B, G, seeds, q, ends, length,
                       integral, status, nsteps, p, none);
  else
    hipLaunchKernelGGL((squash_k<false, false>), dim3(nb), dim3(kLineBlock), 0, s, B, G, seeds, q, ends, length,
                       integral, status, nsteps, p, none);
  NDSM_LAUNCH_CHECK();
  return 0;
}

// The same with the perpendicular squashing factor Qperp (qperp: nseeds values, DEVICE) next to Q; every other output
// holds ndsmk_squash's bits.  The same checks and launch shape.  Asynchronous.
extern "C" int ndsmk_squash_perp(const double *B, const double *G, int integrand, const int32_t *n3, const double *lo3,
                                 const double *h_dq3, int nseeds, const double *seeds, double step, int max_steps,
                                 double *q, double *qperp, double *ends, double *length, double *integral,
                                 int32_t *status, int32_t *nsteps) {
  NDSM_REQUIRE_READY();
  SqArgs p;
  p.integrand = integrand;
  const int rc = line_args("squash_perp: step > 0 (finite), max_steps >= 1, integrand in 0, 1 and nseeds >= 0",
                           integrand >= 0 && integrand <= 1,
                           B && seeds && q && qperp && ends && length && integral && status && nsteps, n3, lo3, h_dq3,
                           nseeds, step, max_steps, 2, p);
  if (rc != 0 || nseeds == 0) return rc;
  const size_t nl = 2 * (size_t)nseeds;
  const unsigned nb = (unsigned)((nl + kLineBlock - 1) / kLineBlock);
  hipStream_t s = ndsm::stream();
  if (G)
    hipLaunchKernelGGL((squash_k<true, true>), dim3(nb), dim3(kLineBlock), 0, s, B, G, seeds, q, ends, length,
                       integral, status, nsteps, p, qperp);
  else
    hipLaunchKernelGGL((squash_k<false, true>), dim3(nb), dim3(kLineBlock), 0, s, B, G, seeds, q, ends, length,
                       integral, status, nsteps, p, qperp);
  NDSM_LAUNCH_CHECK();
  return 0;
}
