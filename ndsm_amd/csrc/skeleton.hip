// The spine-fan skeleton of the nulls on the device (DESIGN.md "Spine-fan skeleton"): the type of each null from its
// Jacobian, then the two spine lines and a ring of fan lines from it, each traced away from its null and ended where
// it comes within the capture radius of another null.  The semantics - every operand order of the typing, the seeds,
// the capture test - are written out in include/ndsm_hip.h (ndsm_hip_vecpot_skeleton) and restated in numpy by
// tests/skeleton_model.py bit for bit (-ffp-contract=off).  Here:
//
//   type    skel_type_k      one lane per null: sign of det M, the lone eigenvalue by Newton on the characteristic
//                            cubic, the spine and the fan normal from the adjugate of N - mu I, the fan basis; the
//                            L = 2 + nring seeds of the null and the direction of each lane go to scratch (direction 0:
//                            the null has no type and its lanes trace nothing)
//   count   skel_line_k<0>   one lane per line, one wave per workgroup, as trace_k: trace_step.hpp's stage and step
//                            with the lane's own direction, the capture test after every accepted full step; ends,
//                            length, status, nsteps, hit, and offsets[l] = npts(l)
//           scan64_total     scan64.hpp: the scan in place and the total, as paths.hip
//   fill    skel_line_k<1>   the same loop - the same expressions, so the same bits - which stores the points as
//                            paths_k does: point j of line l goes to slot offsets[l] + j
// skel_line_k keeps its own text of the loop that line_walk.hpp's line_walk states for every other line kernel
// (null_line there is this kernel's body with the capture test as a policy, and serves separators.hip): on the shared
// walk the filling kernel with capture came out 7 % slower on an MI355X for no reason found in its instructions
// (DESIGN.md "Shared line machinery").  A fix to line_walk is made here too.
// The seeds and directions pass from the counting to the filling half in g_skel, a line_scratch.hpp LineScratch.
// A lane writes slot offsets[l] + j only for j < min(offsets[l + 1], max_points) - offsets[l].  No atomic append, no
// guessed capacity, no vector indexed with a run-time axis.  In the capture loop every lane reads the same null
// positions in the same order: plain global loads at a lane-independent address, served by the caches (DESIGN.md
// says why they are not staged in LDS).
#include "line_scratch.hpp"
#include "line_walk.hpp"
#include "scan64.hpp"

namespace {

using namespace ndsm;

constexpr int kTypeBlock = 64;
constexpr int kSkelNewtonIters = 40;             // iterations of the Newton descent on the cubic (a choice)
constexpr double kSkelConverged = 0x1p-40;       // |delta| <= this |mu|: converged

// det J by the nulls entry's expansion (nulls.hip det3)
__device__ __forceinline__ double skel_det3(const double J[3][3]) {
  const double a00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  const double a10 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
  const double a20 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  return (J[0][0] * a00 + J[0][1] * a10) + J[0][2] * a20;
}

// of the three vectors (x0,y0,z0), (x1,y1,z1), (x2,y2,z2) the one with the largest sum of squares (the lowest index on
// a tie), normalised, its component of largest modulus (the lowest index on a tie) positive.  false: the largest sum
// of squares is not > 0.
__device__ __forceinline__ bool skel_pick(double x0, double y0, double z0, double x1, double y1, double z1, double x2,
                                          double y2, double z2, double v[3]) {
  const double s0 = (x0 * x0 + y0 * y0) + z0 * z0;
  const double s1 = (x1 * x1 + y1 * y1) + z1 * z1;
  const double s2 = (x2 * x2 + y2 * y2) + z2 * z2;
  double best = s0, x = x0, y = y0, z = z0;
  if (s1 > best) best = s1, x = x1, y = y1, z = z1;
  if (s2 > best) best = s2, x = x2, y = y2, z = z2;
  if (!(best > 0.0)) return false;
  const double nrm = sqrt(best);
  x = x / nrm, y = y / nrm, z = z / nrm;
  double big = fabs(x), lead = x;
  if (fabs(y) > big) big = fabs(y), lead = y;
  if (fabs(z) > big) lead = z;
  if (lead < 0.0) x = -x, y = -y, z = -z;
  v[0] = x, v[1] = y, v[2] = z;
  return true;
}

struct SkelTypeOut {
  int32_t *kind;
  double *eig, *spine, *normal;     // 3 each
  double *seeds, *sgn;              // scratch: 3 per lane, 1 per lane
};

// lane m: null m.  rho = radius min(h); ring: (c_j, s_j), nring of them.
__global__ __launch_bounds__(kTypeBlock) void skel_type_k(const double *__restrict__ pos,
                                                          const double *__restrict__ jac, int nnulls, int nring,
                                                          const double *__restrict__ ring, double rho, SkelTypeOut o) {
  const int m = (int)(blockIdx.x * kTypeBlock + threadIdx.x);
  if (m >= nnulls) return;
  double M[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int d = 0; d < 3; ++d) M[a][d] = jac[9 * (size_t)m + 3 * a + d];
  }
  const double r0[3] = {pos[3 * (size_t)m], pos[3 * (size_t)m + 1], pos[3 * (size_t)m + 2]};
  const double det = skel_det3(M);
  const double s = det > 0.0 ? 1.0 : (det < 0.0 ? -1.0 : 0.0);
  bool ok = s != 0.0;
  double N[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int d = 0; d < 3; ++d) N[a][d] = s * M[a][d];
  }
  // the monic characteristic cubic of N: mu^3 - a mu^2 + b mu - c
  const double ca = (N[0][0] + N[1][1]) + N[2][2];
  const double cb = ((N[0][0] * N[1][1] - N[0][1] * N[1][0]) + (N[0][0] * N[2][2] - N[0][2] * N[2][0])) +
                    (N[1][1] * N[2][2] - N[1][2] * N[2][1]);
  const double cc = skel_det3(N);
  double ss = N[0][0] * N[0][0];
  ss = ss + N[0][1] * N[0][1];
  ss = ss + N[0][2] * N[0][2];
  ss = ss + N[1][0] * N[1][0];
  ss = ss + N[1][1] * N[1][1];
  ss = ss + N[1][2] * N[1][2];
  ss = ss + N[2][0] * N[2][0];
  ss = ss + N[2][1] * N[2][1];
  ss = ss + N[2][2] * N[2][2];
  double mu = sqrt(ss);
  bool conv = false;
  if (ok) {
#pragma unroll 1
    for (int it = 0; it < kSkelNewtonIters; ++it) {
      const double pv = ((mu - ca) * mu + cb) * mu - cc;
      const double dp = (3.0 * mu - 2.0 * ca) * mu + cb;
      const double delta = pv / dp;
      mu = mu - delta;
      if (fabs(delta) <= kSkelConverged * fabs(mu)) {
        conv = true;
        break;
      }
    }
  }
  ok = ok && conv && mu > 0.0;
  const double t = ca - mu;
  ok = ok && t < 0.0;
  double v[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0}, e1[3] = {0.0, 0.0, 0.0}, e2[3] = {0.0, 0.0, 0.0};
  if (ok) {
    // C = adj(N - mu I), the nulls entry's nine expressions: its columns are multiples of the spine vector, its rows
    // of the fan normal
    double J[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int d = 0; d < 3; ++d) J[a][d] = a == d ? N[a][d] - mu : N[a][d];
    }
    const double a00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    const double a01 = J[0][2] * J[2][1] - J[0][1] * J[2][2];
    const double a02 = J[0][1] * J[1][2] - J[0][2] * J[1][1];
    const double a10 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    const double a11 = J[0][0] * J[2][2] - J[0][2] * J[2][0];
    const double a12 = J[0][2] * J[1][0] - J[0][0] * J[1][2];
    const double a20 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double a21 = J[0][1] * J[2][0] - J[0][0] * J[2][1];
    const double a22 = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    const bool okv = skel_pick(a00, a10, a20, a01, a11, a21, a02, a12, a22, v);
    const bool okw = skel_pick(a00, a01, a02, a10, a11, a12, a20, a21, a22, w);
    ok = okv && okw;
  }
  if (ok) {
    // the fan basis, the squash entry's start rule with w in place of e
    line_fan_basis(w, e1, e2);
  }
  const double p2 = cc / mu;
  const double disc = t * t - 4.0 * p2;
  int kind = 0;
  if (ok) kind = (s > 0.0 ? -1 : 1) * (disc < 0.0 ? 2 : 1);
  o.kind[m] = kind;
  o.eig[3 * (size_t)m] = ok ? s * mu : 0.0;
  o.eig[3 * (size_t)m + 1] = ok ? s * t : 0.0;
  o.eig[3 * (size_t)m + 2] = ok ? p2 : 0.0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    o.spine[3 * (size_t)m + d] = ok ? v[d] : 0.0;
    o.normal[3 * (size_t)m + d] = ok ? w[d] : 0.0;
  }
  // the seeds and directions of the null's lanes: spine lanes run with s, fan lanes against it; no type: the null's
  // own position and direction 0
  const size_t L = 2 + (size_t)nring;
  const size_t l0 = (size_t)m * L;
  for (size_t q = 0; q < L; ++q) {
    double sd[3] = {r0[0], r0[1], r0[2]}, sg = 0.0;
    if (ok) {
      if (q == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) sd[d] = r0[d] + rho * v[d];
        sg = s;
      } else if (q == 1) {
#pragma unroll
        for (int d = 0; d < 3; ++d) sd[d] = r0[d] - rho * v[d];
        sg = s;
      } else {
        const double c = ring[2 * (q - 2)], sn = ring[2 * (q - 2) + 1];
#pragma unroll
        for (int d = 0; d < 3; ++d) sd[d] = r0[d] + rho * (c * e1[d] + sn * e2[d]);
        sg = -s;
      }
    }
    o.seeds[3 * (l0 + q)] = sd[0];
    o.seeds[3 * (l0 + q) + 1] = sd[1];
    o.seeds[3 * (l0 + q) + 2] = sd[2];
    o.sgn[l0 + q] = sg;
  }
}

struct SkelLineOut {
  double *ends, *length;            // the counting pass
  int32_t *status, *nsteps, *hit;
  i64 *npts;                        // offsets before the scan
  double *points, *bpt;             // the filling pass (bpt may be nullptr)
};

__device__ __forceinline__ void skel_put(const SkelLineOut &o, i64 k, const double r[3], const double bv[3]) {
  o.points[3 * k] = r[0];
  o.points[3 * k + 1] = r[1];
  o.points[3 * k + 2] = r[2];
  if (o.bpt) {
    o.bpt[3 * k] = bv[0];
    o.bpt[3 * k + 1] = bv[1];
    o.bpt[3 * k + 2] = bv[2];
  }
}

// lane l = m L + q: line q of null m, from seeds[l] in the direction sgn[l].  p.nseeds = nnulls.  cap2 = (capture
// min(h))^2, 0: no capture test.  kFill false: the line's outputs and its point count; true: its points into the slots
// offsets[l] + j, j < room.
template <bool kFill>
__global__ __launch_bounds__(kLineBlock) void skel_line_k(const double *__restrict__ B,
                                                          const double *__restrict__ seeds,
                                                          const double *__restrict__ sgns,
                                                          const double *__restrict__ pos, size_t L, double cap2,
                                                          const i64 *__restrict__ offsets, i64 every, i64 max_points,
                                                          SkelLineOut o, TrArgs p) {
  const size_t l = (size_t)blockIdx.x * kLineBlock + threadIdx.x;
  const size_t nl = (size_t)p.nseeds * L;
  if (l >= nl) return;
  const int own = (int)(l / L);
  const double sgn = sgns[l];
  const size_t sy = (size_t)p.n[0], sz = (size_t)p.n[0] * (size_t)p.n[1];
  const size_t N = sz * (size_t)p.n[2];

  i64 base = 0, room = 0;
  if (kFill) {
    // the slots of this lane: [base, min(offsets[l + 1], max_points)) and nothing else
    base = offsets[l];
    const i64 next_base = offsets[l + 1];
    const i64 stop = next_base < max_points ? next_base : max_points;
    room = (base >= 0 && stop > base) ? stop - base : 0;
    if (room == 0) return;
  }

  double r[3] = {seeds[3 * l], seeds[3 * l + 1], seeds[3 * l + 2]};
  double len = 0.0;
  double bv[3] = {0.0, 0.0, 0.0};
  int st = NDSMK_TRACE_UNFINISHED, ns = 0, hit = -1;
  i64 j = 0, due = 0;
  bool inside = true, run = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) inside = inside && (r[d] >= p.lo[d]) && (r[d] <= p.hi[d]);
  if (sgn == 0.0) {
    st = NDSMK_SKEL_NONE;
    run = false;
  } else if (!inside) {
    st = NDSMK_TRACE_OUTSIDE;
    run = false;
  }
  if (run) {
    for (int it = 0; it < p.max_steps; ++it) {
      double k1[3], q1, rn[3], dI;
      if (!tr_stage<false, true>(B, nullptr, p, N, sy, sz, sgn, r[0], r[1], r[2], k1, q1, bv, nullptr) ||
          !tr_rk4<false>(B, nullptr, p, N, sy, sz, sgn, r, k1, q1, p.ds, rn, dI)) {
        st = NDSMK_TRACE_NULL;
        break;
      }
      double t;
      const int face = line_first_face(p, r, rn, t);
      double s = p.ds;
      if (face != 0) {
        s = t * p.ds;
        if (!tr_rk4<false>(B, nullptr, p, N, sy, sz, sgn, r, k1, q1, s, rn, dI)) {
          st = NDSMK_TRACE_NULL;
          break;
        }
      }
      // step `it` moves the line: the state before it is a point when `it` is a multiple of every
      if ((i64)it == due) {
        if (kFill && j < room) skel_put(o, base + j, r, bv);
        j = j + 1;
        due = due + every;
      }
      len = len + s;
      ns = it + 1;
      if (face != 0) {
        line_snap(p, face, rn, r);
        st = face;
        break;
      }
      r[0] = rn[0], r[1] = rn[1], r[2] = rn[2];
      if (cap2 > 0.0) {
        // the first other null within the capture radius, in ascending order
        for (int mm = 0; mm < p.nseeds; ++mm) {
          if (mm == own) continue;
          const double dx = r[0] - pos[3 * (size_t)mm], dy = r[1] - pos[3 * (size_t)mm + 1],
                       dz = r[2] - pos[3 * (size_t)mm + 2];
          if ((dx * dx + dy * dy) + dz * dz <= cap2) {
            hit = mm;
            break;
          }
        }
        if (hit >= 0) {
          st = NDSMK_SKEL_CAPTURED;
          break;
        }
      }
    }
  }
  if (kFill) {
    // the final state, with B interpolated at it (after the snap); nothing is interpolated where no line ran
    if (j < room) {
      if (run) {
        double k1[3], q1;
        (void)tr_stage<false, true>(B, nullptr, p, N, sy, sz, sgn, r[0], r[1], r[2], k1, q1, bv, nullptr);
      }
      skel_put(o, base + j, r, bv);
    }
  } else {
    o.ends[3 * l] = r[0];
    o.ends[3 * l + 1] = r[1];
    o.ends[3 * l + 2] = r[2];
    o.length[l] = len;
    o.status[l] = st;
    o.nsteps[l] = ns;
    o.hit[l] = hit;
    o.npts[l] = ns <= 0 ? 1 : (i64)((ns - 1) / (int)every) + 2;
  }
}

void skel_release();
LineScratch g_skel = {0, skel_release};
void skel_release() { g_skel.release(); }

const char *kSkelUsage = "skeleton: step > 0 (finite), max_steps >= 1, radius > 0 (finite), capture >= 0 (finite), "
                         "every >= 1, max_points >= 0, nring >= 0 and nnulls >= 0";

// the scalar checks and the set-up of both halves; cap2 = (capture min(h))^2
int skel_args(bool arrays_ok, const int32_t *n3, const double *lo3, const double *h_dq3, int nnulls, int nring,
              double radius, double capture, double step, int max_steps, int every, int64_t max_points, TrArgs &p,
              double &rho, double &cap2) {
  const bool own_ok = nring >= 0 && every >= 1 && max_points >= 0 && radius > 0.0 && radius <= 1.0e300 &&
                      capture >= 0.0 && capture <= 1.0e300;
  p.ndir = 1;
  p.sgn0 = 1;
  if (own_ok && nnulls > 0) NDSM_CHECK_ARG(nring <= 0x7ffffff0);
  const int rc = line_args(kSkelUsage, own_ok, arrays_ok, n3, lo3, h_dq3, nnulls, step, max_steps,
                           own_ok ? 2 + nring : 1, p);
  if (rc != 0 || nnulls == 0) return rc;
  null_line_radii(h_dq3, radius, capture, rho, cap2);
  return 0;
}

}  // namespace

// The typing and the counting half (see ndsm_kernels.h).  Blocks for the total.
extern "C" int ndsmk_skel_count(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, int nnulls,
                                const double *pos, const double *jac, int nring, const double *ring, double radius,
                                double capture, double step, int max_steps, int every, int64_t max_points,
                                int32_t *kind, double *eig, double *spine, double *normal, double *ends,
                                double *length, int32_t *status, int32_t *nsteps, int32_t *hit, int64_t *offsets,
                                int64_t *h_total) {
  NDSM_REQUIRE_READY();
  if (h_total) *h_total = 0;
  TrArgs p;
  double rho = 0.0, cap2 = 0.0;
  int rc = skel_args(B && pos && jac && (nring <= 0 || ring) && kind && eig && spine && normal && ends && length &&
                         status && nsteps && hit && offsets && h_total,
                     n3, lo3, h_dq3, nnulls, nring, radius, capture, step, max_steps, every, max_points, p, rho, cap2);
  if (rc != 0 || nnulls == 0) return rc;
  const size_t L = 2 + (size_t)nring;
  const size_t nl = (size_t)nnulls * L;
  rc = g_skel.grow(nl);
  if (rc != 0) return rc;
  double *seeds = g_skel.seeds(), *sgns = g_skel.sgns(nl);
  hipStream_t s = ndsm::stream();
  const SkelTypeOut to = {kind, eig, spine, normal, seeds, sgns};
  hipLaunchKernelGGL(skel_type_k, dim3((unsigned)((nnulls + kTypeBlock - 1) / kTypeBlock)), dim3(kTypeBlock), 0, s, pos,
                     jac, nnulls, nring, ring, rho, to);
  NDSM_LAUNCH_CHECK();
  const SkelLineOut o = {ends, length, status, nsteps, hit, (i64 *)offsets, nullptr, nullptr};
  hipLaunchKernelGGL(skel_line_k<false>, dim3((unsigned)((nl + kLineBlock - 1) / kLineBlock)), dim3(kLineBlock), 0, s, B,
                     seeds, sgns, pos, L, cap2, (const i64 *)nullptr, (i64)every, (i64)max_points, o, p);
  NDSM_LAUNCH_CHECK();
  rc = scan64_total(offsets, nl, h_total, s);
  if (rc != 0) return rc;
  g_skel.lanes = nl;
  return 0;
}

// The filling half, after ndsmk_skel_count with the same arguments and its offsets.  Asynchronous.
extern "C" int ndsmk_skel_fill(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, int nnulls,
                               const double *pos, int nring, double radius, double capture, double step,
                               int max_steps, int every, int64_t max_points, const int64_t *offsets, double *points,
                               double *bpt) {
  NDSM_REQUIRE_READY();
  TrArgs p;
  double rho = 0.0, cap2 = 0.0;
  const int rc = skel_args(B && pos && offsets && (max_points == 0 || points), n3, lo3, h_dq3, nnulls, nring, radius,
                           capture, step, max_steps, every, max_points, p, rho, cap2);
  if (rc != 0 || nnulls == 0 || max_points == 0) return rc;
  const size_t L = 2 + (size_t)nring;
  const size_t nl = (size_t)nnulls * L;
  // (the seeds and directions are those the counting half of this call left in the scratch)
  NDSM_CHECK_ARG(g_skel.buf && g_skel.lanes == nl);
  const double *seeds = g_skel.seeds(), *sgns = g_skel.sgns(nl);
  const SkelLineOut o = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, points, bpt};
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(skel_line_k<true>, dim3((unsigned)((nl + kLineBlock - 1) / kLineBlock)), dim3(kLineBlock), 0, s, B,
                     seeds, sgns, pos, L, cap2, (const i64 *)offsets, (i64)every, (i64)max_points, o, p);
  NDSM_LAUNCH_CHECK();
  return 0;
}
