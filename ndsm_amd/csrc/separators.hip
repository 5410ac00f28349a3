// Separator lines on the device (DESIGN.md "Separator lines"): a bracket is an arc of the fan ring of a null m, given by
// two ring coefficient pairs a and b, and a null m' of the opposite sign.  The fan line that ends at m' - the separator -
// lies where the fan lines of the arc change the side of the fan of m' on which they pass it.  The semantics - every
// operand order of the lane directions, the seeds, the closest-approach test, the narrowing - are written out in
// include/ndsm_hip.h (ndsm_hip_vecpot_separators) and restated in numpy by tests/separator_model.py bit for bit
// (-ffp-contract=off).  Here:
//
//   check   sep_check_k      one lane per bracket: a pair index outside 0 .. nnulls - 1 raises the flag the host reads
//   refine  sep_refine_k     one wave per bracket, all rounds inside the launch: lane i traces the fan line of the
//                            direction ((1 - t) a + t b) / |.|, t = i / 63, with line_walk.hpp's line_walk and keeps
//                            the side of the fan of m' at its closest approach; a ballot finds the lowest lane whose side
//                            differs from lane 0's, shuffles fetch the two directions round the change, and the arc
//                            shrinks by 63 per round.  The per-bracket outputs, and the seed and the direction of the
//                            bracket's line, go to scratch.
//   count   sep_line_k<0>    one lane per bracket: line_walk.hpp's null_line, the body of skel_line_k, with the capture
//                            test against m' alone: ends, length, status, nsteps, and offsets[l] = npts(l)
//           scan64_total     scan64.hpp: the scan in place and the total, as paths.hip
//   fill    sep_line_k<1>    the same call, so the same bits, which stores the points
// The flag of the check, the seeds and the directions live in g_sep, a line_scratch.hpp LineScratch with one leading
// slot.
// A lane writes slot offsets[l] + j only for j < min(offsets[l + 1], max_points) - offsets[l].  No wave ever leaves
// sep_refine_k's round loop with part of its lanes: the exits are decided from ballots and lane 0's values, which every
// lane holds.
#include "line_scratch.hpp"
#include "line_walk.hpp"
#include "scan64.hpp"

namespace {

using namespace ndsm;

enum { kSepNone = 0, kSepFound = 1, kSepFar = 2, kSepNoCrossing = 3, kSepGap = 4, kSepUnresolved = 5 };
constexpr int kCheckBlock = 256;

__global__ __launch_bounds__(kCheckBlock) void sep_check_k(const int32_t *__restrict__ pair, int nbr, int nnulls,
                                                           int32_t *flag) {
  const int l = (int)(blockIdx.x * kCheckBlock + threadIdx.x);
  if (l >= nbr) return;
  const int m = pair[2 * (size_t)l], m2 = pair[2 * (size_t)l + 1];
  if (m < 0 || m >= nnulls || m2 < 0 || m2 >= nnulls) *flag = 1;
}

struct SepOut {
  int32_t *state, *nrounds, *side;
  double *coef, *width, *dmin;      // 4, 1, 2 per bracket
  double *seeds, *sgn;              // scratch: 3 per bracket, 1 per bracket
};

// The closest approach of a fan line to the null at tp: the smallest d2 over the points after the accepted full steps
// (the first of them on a tie), g = w' . (r - tp) there; the walk ends where the null captures the line.
struct SepApproach {
  const double *tp, *tw;
  double cap2;
  double best = INFINITY, g = 0.0;
  __device__ __forceinline__ void step(int, const double *, const double *, const double *, double, double) {}
  static constexpr int kArrived = NDSMK_SKEL_CAPTURED;
  __device__ __forceinline__ bool arrived(const double r[3]) {
    const double dx = r[0] - tp[0], dy = r[1] - tp[1], dz = r[2] - tp[2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 < best) {
      best = d2;
      g = (tw[0] * dx + tw[1] * dy) + tw[2] * dz;
    }
    return d2 <= cap2;
  }
};

// workgroup = wave = bracket br.  rho = radius min(h), cap2 = (capture min(h))^2 > 0.
__global__ __launch_bounds__(kLineBlock) void sep_refine_k(const double *__restrict__ B, const double *__restrict__ pos,
                                                           const int32_t *__restrict__ kind,
                                                           const double *__restrict__ normal,
                                                           const int32_t *__restrict__ pair,
                                                           const double *__restrict__ arc, double rho, double cap2,
                                                           int rounds, double tol, SepOut o, TrArgs p) {
  const size_t br = blockIdx.x;
  const int lane = (int)threadIdx.x;
  const size_t sy = (size_t)p.n[0], sz = (size_t)p.n[0] * (size_t)p.n[1];
  const size_t N = sz * (size_t)p.n[2];
  const int m = pair[2 * br], m2 = pair[2 * br + 1];
  const int k0 = kind[m], k1 = kind[m2];
  const double r0[3] = {pos[3 * (size_t)m], pos[3 * (size_t)m + 1], pos[3 * (size_t)m + 2]};
  const double tp[3] = {pos[3 * (size_t)m2], pos[3 * (size_t)m2 + 1], pos[3 * (size_t)m2 + 2]};
  const double tw[3] = {normal[3 * (size_t)m2], normal[3 * (size_t)m2 + 1], normal[3 * (size_t)m2 + 2]};
  const double w[3] = {normal[3 * (size_t)m], normal[3 * (size_t)m + 1], normal[3 * (size_t)m + 2]};
  const bool valid = m != m2 && ((k0 > 0 && k1 < 0) || (k0 < 0 && k1 > 0));
  const double sg = k0 > 0 ? 1.0 : -1.0;

  // the fan basis of m from its normal, as skel_type_k forms it
  double e1[3], e2[3];
  line_fan_basis(w, e1, e2);

  double ca = arc[4 * br], sa = arc[4 * br + 1], cb = arc[4 * br + 2], sb = arc[4 * br + 3];
  int state = kSepNone, nr = 0, side = 0;
  double dlo = 0.0, dhi = 0.0;
  if (valid) {
    const double t = (double)lane / 63.0;
    for (int rnd = 0; rnd < rounds; ++rnd) {
      // this lane's direction, seed and line
      double c = (1.0 - t) * ca + t * cb, s = (1.0 - t) * sa + t * sb;
      const double nrm = sqrt(c * c + s * s);
      bool ok = nrm > 0.0;
      c = c / nrm, s = s / nrm;
      if (lane == 0) c = ca, s = sa, ok = true;
      if (lane == kLineBlock - 1) c = cb, s = sb, ok = true;
      double seed[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) seed[d] = r0[d] + rho * (c * e1[d] + s * e2[d]);
      // (the walk without its exit step: nothing is stored, so the step that leaves the box is not redone)
      SepApproach v = {tp, tw, cap2};
      bool captured = false;
      if (ok && line_inside(p, seed))
        captured = line_walk<false, false, false>(B, nullptr, p, N, sy, sz, sg, seed, nullptr, nullptr, v) ==
                   NDSMK_SKEL_CAPTURED;
      const double best = v.best, g = v.g;
      const int cls = best < INFINITY ? (g >= 0.0 ? 1 : (g < 0.0 ? -1 : 0)) : 0;

      // the lowest lane >= 1 on another side than lane 0, and the two lanes round the change
      const int c0 = __shfl(cls, 0);
      const unsigned long long differ = __ballot(cls != c0) & ~1ull;
      const bool has = differ != 0ull;
      const int hi = has ? __ffsll((long long)differ) - 1 : kLineBlock - 1;
      const int lo = has ? hi - 1 : 0;
      const int chi = __shfl(cls, hi);
      const double clo_c = __shfl(c, lo), clo_s = __shfl(s, lo), chi_c = __shfl(c, hi), chi_s = __shfl(s, hi);
      const unsigned long long caught = __ballot(captured);
      dlo = sqrt(__shfl(best, lo));
      dhi = sqrt(__shfl(best, hi));
      nr = rnd + 1;
      side = c0;
      if (c0 == 0) {
        state = kSepGap;
        break;
      }
      if (!has) {
        state = kSepNoCrossing;
        break;
      }
      if (chi == 0) {
        state = kSepGap;
        break;
      }
      ca = clo_c, sa = clo_s, cb = chi_c, sb = chi_s;
      const double wd = sqrt((ca - cb) * (ca - cb) + (sa - sb) * (sa - sb));
      if (wd <= tol) {
        state = ((caught >> lo) & (caught >> hi) & 1ull) ? kSepFound : kSepFar;
        break;
      }
      state = kSepUnresolved;
    }
  }
  if (lane != 0) return;
  const bool line = state == kSepFound || state == kSepFar || state == kSepUnresolved;
  o.state[br] = state;
  o.nrounds[br] = nr;
  o.side[br] = side;
  o.coef[4 * br] = ca;
  o.coef[4 * br + 1] = sa;
  o.coef[4 * br + 2] = cb;
  o.coef[4 * br + 3] = sb;
  o.width[br] = valid ? sqrt((ca - cb) * (ca - cb) + (sa - sb) * (sa - sb)) : 0.0;
  o.dmin[2 * br] = dlo;
  o.dmin[2 * br + 1] = dhi;
#pragma unroll
  for (int d = 0; d < 3; ++d) o.seeds[3 * br + d] = line ? r0[d] + rho * (ca * e1[d] + sa * e2[d]) : r0[d];
  o.sgn[br] = line ? sg : 0.0;
}

// the capture test of a separator: the one target null, always tested
struct SepCapture {
  static constexpr bool kHit = false;
  double tp[3], cap2;
  __device__ __forceinline__ bool test(const double r[3]) const {
    const double dx = r[0] - tp[0], dy = r[1] - tp[1], dz = r[2] - tp[2];
    return (dx * dx + dy * dy) + dz * dz <= cap2;
  }
};

// lane l: the line of bracket l, from seeds[l] in the direction sgn[l] (0: no line, one point), captured by the null
// pair[2 l + 1] alone.  p.nseeds = nbr.  The body is line_walk.hpp's null_line: skel_line_k's loop with this capture
// test, on the shared walk.
template <bool kFill>
__global__ __launch_bounds__(kLineBlock) void sep_line_k(const double *__restrict__ B,
                                                         const double *__restrict__ seeds,
                                                         const double *__restrict__ sgns,
                                                         const double *__restrict__ pos,
                                                         const int32_t *__restrict__ pair, double cap2,
                                                         const i64 *__restrict__ offsets, i64 every, i64 max_points,
                                                         NullLineOut o, TrArgs p) {
  const size_t l = (size_t)blockIdx.x * kLineBlock + threadIdx.x;
  if (l >= (size_t)p.nseeds) return;
  const size_t m2 = (size_t)pair[2 * l + 1];
  SepCapture cap = {{pos[3 * m2], pos[3 * m2 + 1], pos[3 * m2 + 2]}, cap2};
  null_line<kFill>(B, seeds, sgns, l, cap, offsets, every, max_points, o, p);
}

// (the leading slot is the flag of the check)
void sep_release();
LineScratch g_sep = {1, sep_release};
void sep_release() { g_sep.release(); }

const char *kSepUsage = "separators: step > 0 (finite), max_steps >= 1, radius > 0 (finite), capture > 0 (finite), "
                        "rounds >= 1, tol >= 0 (finite), every >= 1, max_points >= 0, nnulls >= 0, nbr >= 0 and every "
                        "pair index in 0 .. nnulls - 1";

// the scalar checks and the set-up of both halves; cap2 = (capture min(h))^2
int sep_args(bool arrays_ok, const int32_t *n3, const double *lo3, const double *h_dq3, int nnulls, int nbr,
             double radius, double capture, double step, int max_steps, int rounds, double tol, int every,
             int64_t max_points, TrArgs &p, double &rho, double &cap2) {
  const bool own_ok = nnulls >= 0 && (nbr <= 0 || nnulls >= 1) && rounds >= 1 && tol >= 0.0 && tol <= 1.0e300 &&
                      every >= 1 && max_points >= 0 && radius > 0.0 && radius <= 1.0e300 && capture > 0.0 &&
                      capture <= 1.0e300;
  p.ndir = 1;
  p.sgn0 = 1;
  // (kLineBlock lanes per bracket in the refinement)
  const int rc = line_args(kSepUsage, own_ok, arrays_ok, n3, lo3, h_dq3, nbr, step, max_steps, kLineBlock, p);
  if (rc != 0 || nbr == 0) return rc;
  null_line_radii(h_dq3, radius, capture, rho, cap2);
  // (a capture whose square underflows would switch the test off)
  if (!(cap2 > 0.0)) return fail(NDSMK_EVALUE, kSepUsage, __FILE__, __LINE__);
  return 0;
}

}  // namespace

// The check, the refinement and the counting half (see ndsm_kernels.h).  Blocks for the flag and for the total.
extern "C" int ndsmk_sep_count(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, int nnulls,
                               const double *pos, const int32_t *kind, const double *normal, int nbr,
                               const int32_t *pair, const double *arc, double radius, double capture, double step,
                               int max_steps, int rounds, double tol, int every, int64_t max_points, int32_t *state,
                               int32_t *nrounds, double *coef, double *width, int32_t *side, double *dmin,
                               double *ends, double *length, int32_t *status, int32_t *nsteps, int64_t *offsets,
                               int64_t *h_total) {
  NDSM_REQUIRE_READY();
  if (h_total) *h_total = 0;
  TrArgs p;
  double rho = 0.0, cap2 = 0.0;
  int rc = sep_args(B && pos && kind && normal && pair && arc && state && nrounds && coef && width && side && dmin &&
                        ends && length && status && nsteps && offsets && h_total,
                    n3, lo3, h_dq3, nnulls, nbr, radius, capture, step, max_steps, rounds, tol, every, max_points, p,
                    rho, cap2);
  if (rc != 0 || nbr == 0) return rc;
  const size_t nb = (size_t)nbr;
  rc = g_sep.grow(nb);
  if (rc != 0) return rc;
  int32_t *flag = (int32_t *)g_sep.buf;
  double *seeds = g_sep.seeds(), *sgns = g_sep.sgns(nb);
  hipStream_t s = ndsm::stream();
  // no pair index is used before all of them are known to be in range
  int32_t bad = 0;
  NDSM_HIP(hipMemsetAsync(flag, 0, sizeof(double), s));
  hipLaunchKernelGGL(sep_check_k, dim3((unsigned)((nb + kCheckBlock - 1) / kCheckBlock)), dim3(kCheckBlock), 0, s, pair,
                     nbr, nnulls, flag);
  NDSM_LAUNCH_CHECK();
  NDSM_HIP(hipMemcpyAsync(&bad, flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  NDSM_HIP(hipStreamSynchronize(s));
  if (bad != 0) return fail(NDSMK_EVALUE, kSepUsage, __FILE__, __LINE__);
  const SepOut ro = {state, nrounds, side, coef, width, dmin, seeds, sgns};
  hipLaunchKernelGGL(sep_refine_k, dim3((unsigned)nb), dim3(kLineBlock), 0, s, B, pos, kind, normal, pair, arc, rho, cap2,
                     rounds, tol, ro, p);
  NDSM_LAUNCH_CHECK();
  const NullLineOut o = {ends, length, status, nsteps, nullptr, (i64 *)offsets, {nullptr, nullptr, nullptr, nullptr}};
  hipLaunchKernelGGL(sep_line_k<false>, dim3((unsigned)((nb + kLineBlock - 1) / kLineBlock)), dim3(kLineBlock), 0, s, B,
                     seeds, sgns, pos, pair, cap2, (const i64 *)nullptr, (i64)every, (i64)max_points, o, p);
  NDSM_LAUNCH_CHECK();
  rc = scan64_total(offsets, nb, h_total, s);
  if (rc != 0) return rc;
  g_sep.lanes = nb;
  return 0;
}

// The filling half, after ndsmk_sep_count with the same arguments and its offsets.  Asynchronous.
extern "C" int ndsmk_sep_fill(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, int nnulls,
                              const double *pos, int nbr, const int32_t *pair, double radius, double capture,
                              double step, int max_steps, int rounds, double tol, int every, int64_t max_points,
                              const int64_t *offsets, double *points, double *bpt) {
  NDSM_REQUIRE_READY();
  TrArgs p;
  double rho = 0.0, cap2 = 0.0;
  const int rc = sep_args(B && pos && pair && offsets && (max_points == 0 || points), n3, lo3, h_dq3, nnulls, nbr,
                          radius, capture, step, max_steps, rounds, tol, every, max_points, p, rho, cap2);
  if (rc != 0 || nbr == 0 || max_points == 0) return rc;
  const size_t nb = (size_t)nbr;
  // (the seeds and directions are those the counting half of this call left in the scratch; it checked the pairs)
  NDSM_CHECK_ARG(g_sep.buf && g_sep.lanes == nb);
  const double *seeds = g_sep.seeds(), *sgns = g_sep.sgns(nb);
  const NullLineOut o = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, {points, bpt, nullptr, nullptr}};
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(sep_line_k<true>, dim3((unsigned)((nb + kLineBlock - 1) / kLineBlock)), dim3(kLineBlock), 0, s, B,
                     seeds, sgns, pos, pair, cap2, (const i64 *)offsets, (i64)every, (i64)max_points, o, p);
  NDSM_LAUNCH_CHECK();
  return 0;
}
