// Patch connectivity fluxes on the device (DESIGN.md "Flux partitioning and connectivity"): one field line from every
// labelled pixel of the lower face, the class of the place where it ends, and per (patch, class) pair the number of
// lines and the flux at their feet.  The semantics are written out in include/ndsm_hip.h (ndsm_hip_vecpot_connect) and
// restated in numpy by tests/connect_model.py bit for bit (-ffp-contract=off).  Here:
//
//   lines   conn_trace_k   one lane per pixel of the lower face: line_walk.hpp's loop with the sign of B_z at the
//                          node as the lane's direction and a visitor that adds the length alone - the trace entry's
//                          expressions, so its bits -, then the nearest pixel of a line that comes back to the face,
//                          and the sort's key (a (K + 9) + (c + 8); 0: no line)
//   pairs   keysum.hpp     the stable sort of (key, pixel) and the runs; conn_pair_k: one wave per pair
// No atomics anywhere: the same input gives the same bits.
#include "diffq.hpp"
#include "keysum.hpp"
#include "line_walk.hpp"

namespace {

using namespace ndsm;

constexpr int kConnectNone = -9;        // NDSM_HIP_CONNECT_NONE

struct LengthOnly {
  double len = 0.0;
  __device__ __forceinline__ void step(int, const double *, const double *, const double *, double s, double) {
    len = len + s;
  }
  static constexpr int kArrived = 0;   // (never)
  __device__ __forceinline__ bool arrived(const double *) { return false; }
};

// a label outside 1 .. K counts as 0
__device__ __forceinline__ int conn_class(int32_t l, int K) { return (l >= 1 && l <= K) ? (int)l : 0; }

// the nearest node of the axis to the coordinate v
__device__ __forceinline__ int conn_nearest(double v, double lo, double h, int n) {
  const int q = (int)floor((v - lo) / h + 0.5);
  return q < 0 ? 0 : (q > n - 1 ? n - 1 : q);
}

__global__ __launch_bounds__(kLineBlock) void conn_trace_k(const double *__restrict__ B, const double *__restrict__ xs,
                                                           const double *__restrict__ ys,
                                                           const int32_t *__restrict__ label, int K, TrArgs p,
                                                           int32_t *__restrict__ dest, double *__restrict__ ends,
                                                           double *__restrict__ length, int32_t *__restrict__ status,
                                                           u64 *__restrict__ key, unsigned *__restrict__ idx) {
  const size_t l = (size_t)blockIdx.x * kLineBlock + threadIdx.x;
  const size_t sy = (size_t)p.n[0], sz = (size_t)p.n[0] * (size_t)p.n[1];
  if (l >= sz) return;
  const size_t N = sz * (size_t)p.n[2];
  const size_t j = l / sy;
  const int i = (int)(l - j * sy);
  const int a = conn_class(label[l], K);
  const double bzn = B[2 * N + l];
  double r[3] = {xs[i], ys[j], p.lo[2]};
  LengthOnly v;
  int st = NDSMK_TRACE_OUTSIDE, c = kConnectNone;
  u64 k = 0;
  if (a != 0 && (bzn > 0.0 || bzn < 0.0) && line_inside(p, r)) {
    const double sgn = bzn > 0.0 ? 1.0 : -1.0;
    st = line_walk<false, false>(B, nullptr, p, N, sy, sz, sgn, r, nullptr, nullptr, v);
    if (st == NDSMK_TRACE_ZLO) {
      const int i2 = conn_nearest(r[0], p.lo[0], p.h[0], p.n[0]), j2 = conn_nearest(r[1], p.lo[1], p.h[1], p.n[1]);
      c = conn_class(label[(size_t)j2 * sy + (size_t)i2], K);
    } else {
      c = -st;
    }
    k = (u64)a * ((u64)K + 9ull) + (u64)(c + 8);
  }
  dest[l] = c;
  ends[3 * l] = r[0];
  ends[3 * l + 1] = r[1];
  ends[3 * l + 2] = r[2];
  length[l] = v.len;
  status[l] = st;
  key[l] = k;
  idx[l] = (unsigned)l;
}

struct ConnTerm {
  const double *__restrict__ bz;        // B_z on the lower face
  int nx, ny;
  double hx, hy;
  __device__ __forceinline__ void operator()(unsigned c, double t[1]) const {
    const unsigned j = c / (unsigned)nx;
    const int i = (int)(c - j * (unsigned)nx);
    const double w = trap_w(i, nx, hx) * trap_w((int)j, ny, hy);
    t[0] = fabs(bz[c]) * w;
  }
};

// one wave per pair m < limit
__global__ __launch_bounds__(256) void conn_pair_k(const u64 *__restrict__ sk, const unsigned *__restrict__ sidx,
                                                   const i64 *__restrict__ start, i64 nruns, i64 limit, size_t n, int K,
                                                   ConnTerm term, int32_t *__restrict__ pa, int32_t *__restrict__ pc,
                                                   long long *__restrict__ nlines, double *__restrict__ pflux) {
  const i64 m = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= limit) return;
  const int lane = (int)(threadIdx.x & (kWave - 1));
  const i64 s0 = start[m], s1 = m + 1 < nruns ? start[m + 1] : (i64)n;
  if (s0 < 0 || s1 > (i64)n || s0 >= s1) return;   // (a run is never empty: never taken)
  double v[1];
  ks_wave_sum<1>(sidx, s0, s1, lane, term, v);
  if (lane != 0) return;
  const u64 k = sk[s0], base = ((u64)K + 9ull);
  pa[m] = (int32_t)(k / base);
  pc[m] = (int32_t)(k % base) - 8;
  nlines[m] = s1 - s0;
  pflux[m] = v[0];
}

}  // namespace

// The connectivity (semantics: include/ndsm_hip.h, ndsm_hip_vecpot_connect).  B (nx,ny,nz,3), label (nx,ny; int32), the
// per-pixel outputs dest, ends (3 each), length, status and the pair records pa, pc (int32), nlines (int64), pflux are
// DEVICE arrays; lo3, h_dq3, the mesh vectors h_x (nx), h_y (ny) and h_counts2 on the HOST.  Blocks for the two counts;
// the records are written asynchronously.
extern "C" int ndsmk_connect(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3,
                             const double *h_x, const double *h_y, const int32_t *label, int K, double step,
                             int max_steps, int64_t max_pairs, int64_t *h_counts2, int32_t *dest, double *ends,
                             double *length, int32_t *status, int32_t *pa, int32_t *pc, int64_t *nlines,
                             double *pflux) {
  NDSM_REQUIRE_READY();
  if (h_counts2) h_counts2[0] = h_counts2[1] = 0;
  NDSM_CHECK_ARG(n3 && lo3 && h_dq3 && h_x && h_y && h_counts2);
  NDSM_CHECK_ARG(n3[0] >= 2 && n3[1] >= 2 && n3[2] >= 2);
  const size_t n = (size_t)n3[0] * (size_t)n3[1];
  NDSM_CHECK_ARG(n <= (size_t)0x7fffffff);
  TrArgs p;
  p.ndir = 1;
  p.sgn0 = 1;
  int rc = line_args("connect: step > 0 (finite), max_steps >= 1, K >= 0 and max_pairs >= 0", K >= 0 && max_pairs >= 0,
                     B && label && dest && ends && length && status &&
                         (max_pairs == 0 || (pa && pc && nlines && pflux)),
                     n3, lo3, h_dq3, (int)n, step, max_steps, 1, p);
  if (rc != 0) return rc;
  const size_t b_mesh = ks_up256(((size_t)n3[0] + (size_t)n3[1]) * sizeof(double));
  rc = ks_grow(ks_bytes(n) + b_mesh);
  if (rc != 0) return rc;
  KsBuf b;
  ks_carve(g_ks.a, n, b);
  double *d_x = (double *)((uint8_t *)g_ks.a + ks_bytes(n)), *d_y = d_x + n3[0];

  hipStream_t s = ndsm::stream();
  NDSM_HIP(hipMemcpyAsync(d_x, h_x, (size_t)n3[0] * sizeof(double), hipMemcpyHostToDevice, s));
  NDSM_HIP(hipMemcpyAsync(d_y, h_y, (size_t)n3[1] * sizeof(double), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(conn_trace_k, dim3((unsigned)((n + kLineBlock - 1) / kLineBlock)), dim3(kLineBlock), 0, s, B, d_x,
                     d_y, label, K, p, dest, ends, length, status, b.key[0], b.idx[0]);
  NDSM_LAUNCH_CHECK();
  const u64 max_key = (u64)K * ((u64)K + 9ull) + ((u64)K + 8ull);
  int fin = 0;
  rc = ks_sort_runs(b, n, max_key, s, &fin);
  if (rc != 0) return rc;
  NDSM_HIP(hipMemcpyAsync(g_ks.h_pin, b.flag + n, sizeof(long long), hipMemcpyDeviceToHost, s));
  NDSM_HIP(hipMemcpyAsync(g_ks.h_pin + 1, b.start, sizeof(long long), hipMemcpyDeviceToHost, s));
  NDSM_HIP(hipStreamSynchronize(s));
  const long long M = g_ks.h_pin[0];
  // (key 0 sorts first: the first run starts after the pixels without a line)
  h_counts2[0] = M > 0 ? (long long)n - g_ks.h_pin[1] : 0;
  h_counts2[1] = M;
  const size_t limit = (unsigned long long)max_pairs < (unsigned long long)M ? (size_t)max_pairs : (size_t)M;
  if (limit == 0) return 0;
  const ConnTerm term = {B + 2 * n * (size_t)n3[2], n3[0], n3[1], h_dq3[0], h_dq3[1]};
  hipLaunchKernelGGL(conn_pair_k, dim3((unsigned)((limit + 3) / 4)), dim3(256), 0, s, b.key[fin], b.idx[fin], b.start,
                     (i64)M, (i64)limit, n, K, term, pa, pc, (long long *)nlines, pflux);
  NDSM_LAUNCH_CHECK();
  return 0;
}
