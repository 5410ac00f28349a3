// Flux partitioning of a magnetogram on the device (DESIGN.md "Flux partitioning and connectivity").  The semantics -
// the pixels that are in, the pointer and its tie rule, the numbering, the weights, the table and every operand order -
// are written out in include/ndsm_hip.h (ndsm_hip_partition) and restated in numpy by tests/connect_model.py bit for
// bit (-ffp-contract=off).  Here:
//
//   pointer  part_ptr_k    one lane per pixel: the 3 x 3 read of bz (the caches serve the neighbours), the candidates
//                          in ascending pixel index with a strict >, so equal values stay with the smallest index;
//                          -1 for a pixel that is not in
//   root     part_jump_k   ptr <- ptr[ptr] between two buffers, as many rounds as npix has bits: decided on the host,
//                          no convergence flag is read back
//   number   part_flag_k   per pixel (root ? 1 : 0) + 2^32 (in ? 1 : 0) in one int64, so that ONE scan64_k gives the
//                          roots before a pixel (low word) and both totals: K and the pixels in
//            part_label_k  label = 1 + the roots before the pixel's root; the sort's keys and items
//   table    keysum.hpp    the stable sort of (label, pixel) and the runs; part_table_k: one wave per patch
// No atomics anywhere: the same input gives the same bits.
#include "diffq.hpp"
#include "keysum.hpp"

#include <cmath>

namespace {

using namespace ndsm;

struct PartArgs {
  int nsx, nsy;
  size_t npix;
  double hx, hy, thr;
};

__device__ __forceinline__ bool part_in(double b, double thr) { return fabs(b) > thr; }   // (false for a NaN)

__global__ __launch_bounds__(256) void part_ptr_k(const double *__restrict__ bz, PartArgs p, int32_t *__restrict__ ptr) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= p.npix) return;
  const double b = bz[c];
  if (!part_in(b, p.thr)) {
    ptr[c] = -1;
    return;
  }
  const size_t j = c / (size_t)p.nsx;
  const int i = (int)(c - j * (size_t)p.nsx);
  const bool pos = b > 0.0;
  double best = -1.0;
  size_t at = c;
#pragma unroll
  for (int dj = -1; dj <= 1; ++dj) {
#pragma unroll
    for (int di = -1; di <= 1; ++di) {
      const int ii = i + di;
      const long long jj = (long long)j + dj;
      if (ii < 0 || ii >= p.nsx || jj < 0 || jj >= (long long)p.nsy) continue;
      const size_t q = (size_t)jj * (size_t)p.nsx + (size_t)ii;
      const double v = bz[q];
      if (!part_in(v, p.thr) || (v > 0.0) != pos) continue;
      const double a = fabs(v);
      if (a > best) {           // (ascending q: an equal value stays with the smallest index)
        best = a;
        at = q;
      }
    }
  }
  ptr[c] = (int32_t)at;
}

__global__ __launch_bounds__(256) void part_jump_k(const int32_t *__restrict__ in, int32_t *__restrict__ out, size_t npix) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= npix) return;
  const int32_t q = in[c];
  out[c] = q < 0 ? -1 : in[q];
}

constexpr i64 kInUnit = (i64)1 << 32;

__global__ __launch_bounds__(256) void part_flag_k(const int32_t *__restrict__ root, size_t npix, i64 *__restrict__ flag) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= npix) return;
  const int32_t q = root[c];
  flag[c] = q < 0 ? 0 : kInUnit + ((size_t)q == c ? 1 : 0);
}

// before: flag after the scan
__global__ __launch_bounds__(256) void part_label_k(const int32_t *__restrict__ root, const i64 *__restrict__ before,
                                                    size_t npix, int32_t *__restrict__ label, u64 *__restrict__ key,
                                                    unsigned *__restrict__ idx) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= npix) return;
  const int32_t q = root[c];
  const int32_t k = q < 0 ? 0 : (int32_t)(before[q] & (kInUnit - 1)) + 1;
  label[c] = k;
  if (key) {
    key[c] = (u64)k;
    idx[c] = (unsigned)c;
  }
}

struct PartOut {
  long long *root, *npix;
  int32_t *sign;
  double *flux, *sx, *sy;
};

struct PartTerm {
  const double *__restrict__ bz, *__restrict__ xs, *__restrict__ ys;
  PartArgs p;
  __device__ __forceinline__ void operator()(unsigned c, double t[3]) const {
    const unsigned j = c / (unsigned)p.nsx;
    const int i = (int)(c - j * (unsigned)p.nsx);
    const double w = trap_w(i, p.nsx, p.hx) * trap_w((int)j, p.nsy, p.hy);
    const double f = bz[c] * w;
    t[0] = f;
    t[1] = f * xs[i];
    t[2] = f * ys[j];
  }
};

// one wave per patch m < limit: run m of the sorted labels is patch m + 1
__global__ __launch_bounds__(256) void part_table_k(const unsigned *__restrict__ sidx, const i64 *__restrict__ start,
                                                    i64 nruns, i64 limit, size_t n, const int32_t *__restrict__ root,
                                                    PartTerm term, PartOut o) {
  const i64 m = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= limit) return;
  const int lane = (int)(threadIdx.x & (kWave - 1));
  const i64 s0 = start[m], s1 = m + 1 < nruns ? start[m + 1] : (i64)n;
  if (s0 < 0 || s1 > (i64)n || s0 >= s1) return;   // (a run is never empty: never taken)
  double v[3];
  ks_wave_sum<3>(sidx, s0, s1, lane, term, v);
  if (lane != 0) return;
  const int32_t r = root[sidx[s0]];
  o.root[m] = r;
  o.sign[m] = term.bz[r] > 0.0 ? 1 : -1;
  o.npix[m] = s1 - s0;
  o.flux[m] = v[0];
  o.sx[m] = v[1];
  o.sy[m] = v[2];
}

// the two pointer buffers and the mesh vectors, after the sort's arrays
size_t part_own_bytes(size_t npix, int nsx, int nsy) {
  return 2 * ks_up256(npix * sizeof(int32_t)) + ks_up256(((size_t)nsx + (size_t)nsy) * sizeof(double));
}

}  // namespace

// 0, or 9001 when the device cannot hold a call's arrays: caller_bytes of the caller's side (staged host arrays) plus
// the scratch, against the device's TOTAL memory - ndsmk_flow_fits' screen, all in doubles
extern "C" int ndsmk_partition_fits(const int32_t *nsrc2, double caller_bytes) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(nsrc2);
  size_t fr = 0, tot = 0;
  const int rc = ndsmk_mem_info(&fr, &tot);
  if (rc != 0) return rc;
  // per pixel: two keys (16), two items (8), the flags (8), the starts (8), two pointers (8), the digit counts (2)
  if (caller_bytes + 50.0 * (double)nsrc2[0] * (double)nsrc2[1] > (double)tot)
    return ndsmk_note_error(NDSMK_ENODEV, "partition: the arrays and the scratch need more device memory than the "
                                          "device has");
  return 0;
}

// The partition (semantics: include/ndsm_hip.h, ndsm_hip_partition).  bz and label (nsx,nsy; int32) and the record
// arrays are DEVICE arrays; h_xs, h_ys and h_counts2 on the HOST.  Blocks for the two counts; the records are written
// asynchronously.
extern "C" int ndsmk_partition(const int32_t *nsrc2, const double *h_xs, const double *h_ys, const double *bz, double thr,
                               int64_t max_patches, int64_t *h_counts2, int32_t *label, int64_t *root, int32_t *sign,
                               int64_t *npix, double *flux, double *sx, double *sy) {
  NDSM_REQUIRE_READY();
  if (h_counts2) h_counts2[0] = h_counts2[1] = 0;
  NDSM_CHECK_ARG(nsrc2 && h_xs && h_ys && bz && h_counts2 && label &&
                 (max_patches <= 0 || (root && sign && npix && flux && sx && sy)));
  if (nsrc2[0] < 2 || nsrc2[1] < 2 || !(h_xs[1] - h_xs[0] > 0.0) || !(h_ys[1] - h_ys[0] > 0.0) || !(thr >= 0.0) ||
      !(thr <= 1.7976931348623157e308) || max_patches < 0)
    return ndsmk_note_error(NDSMK_EVALUE, "partition: at least 2 nodes per axis, spacings > 0, a finite thr >= 0 and "
                                          "max_patches >= 0");
  PartArgs p;
  p.nsx = nsrc2[0];
  p.nsy = nsrc2[1];
  p.npix = (size_t)p.nsx * (size_t)p.nsy;
  p.hx = h_xs[1] - h_xs[0];
  p.hy = h_ys[1] - h_ys[0];
  p.thr = thr;
  NDSM_CHECK_ARG(p.npix <= (size_t)0x7fffffff);
  const size_t n = p.npix;
  int rc = ks_grow(ks_bytes(n) + part_own_bytes(n, p.nsx, p.nsy));
  if (rc != 0) return rc;
  KsBuf b;
  ks_carve(g_ks.a, n, b);
  uint8_t *at = (uint8_t *)g_ks.a + ks_bytes(n);
  int32_t *ptr[2];
  for (int c = 0; c < 2; ++c) ptr[c] = (int32_t *)at, at += ks_up256(n * sizeof(int32_t));
  double *d_xs = (double *)at, *d_ys = d_xs + p.nsx;

  hipStream_t s = ndsm::stream();
  const unsigned ng = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(part_ptr_k, dim3(ng), dim3(256), 0, s, bz, p, ptr[0]);
  NDSM_LAUNCH_CHECK();
  int rounds = 0;
  for (size_t v = n; v; v >>= 1) ++rounds;
  int cur = 0;
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(part_jump_k, dim3(ng), dim3(256), 0, s, ptr[cur], ptr[1 - cur], n);
    NDSM_LAUNCH_CHECK();
    cur = 1 - cur;
  }
  const int32_t *root_of = ptr[cur];
  hipLaunchKernelGGL(part_flag_k, dim3(ng), dim3(256), 0, s, root_of, n, b.flag);
  NDSM_LAUNCH_CHECK();
  rc = scan64_total((int64_t *)b.flag, n, (int64_t *)g_ks.h_pin, s);
  if (rc != 0) return rc;
  const long long K = g_ks.h_pin[0] & (kInUnit - 1), nin = g_ks.h_pin[0] >> 32;
  h_counts2[0] = nin;
  h_counts2[1] = K;
  const size_t limit = (unsigned long long)max_patches < (unsigned long long)K ? (size_t)max_patches : (size_t)K;
  hipLaunchKernelGGL(part_label_k, dim3(ng), dim3(256), 0, s, root_of, b.flag, n, label, limit ? b.key[0] : nullptr,
                     b.idx[0]);
  NDSM_LAUNCH_CHECK();
  if (limit == 0) return 0;

  NDSM_HIP(hipMemcpyAsync(d_xs, h_xs, (size_t)p.nsx * sizeof(double), hipMemcpyHostToDevice, s));
  NDSM_HIP(hipMemcpyAsync(d_ys, h_ys, (size_t)p.nsy * sizeof(double), hipMemcpyHostToDevice, s));
  int fin = 0;
  rc = ks_sort_runs(b, n, (u64)K, s, &fin);
  if (rc != 0) return rc;
  // (every label 1 .. K has a pixel: the runs are the patches, K of them)
  const PartTerm term = {bz, d_xs, d_ys, p};
  const PartOut o = {(long long *)root, (long long *)npix, sign, flux, sx, sy};
  hipLaunchKernelGGL(part_table_k, dim3((unsigned)((limit + 3) / 4)), dim3(256), 0, s, b.idx[fin], b.start, (i64)K,
                     (i64)limit, n, root_of, term, o);
  NDSM_LAUNCH_CHECK();
  // the mesh vectors are the caller's pageable memory: the copies above have read them when this returns
  NDSM_HIP(hipStreamSynchronize(s));
  return 0;
}
