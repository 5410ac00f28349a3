// Magnetic nulls of a field on the device (DESIGN.md "Null points"): a screen over every cell of the mesh, then a
// Newton iteration per surviving cell on the trilinear interpolant of line.hpp.  The semantics - the screen, the
// starts, the guards, the tolerances, the record and every operand order - are written out in include/ndsm_hip.h
// (ndsm_hip_vecpot_nulls) and restated in numpy by tests/null_model.py bit for bit (-ffp-contract=off).  Here:
//
//   screen    node_code_k   one streaming pass over the three components: a 7-bit code per node (bit m: B_m > 0,
//                           bit 3 + m: B_m < 0, bit 6: no NaN).  A cell is a candidate when the AND of its eight
//                           corners' codes is exactly bit 6: no component with one strict sign, no NaN.
//             cell_mask_k   the AND per cell, read back through the caches (1 B per node), as one bit per node index
//                           (a wave's ballot) and a count per workgroup
//   order     scan_k        exclusive sums of the workgroup counts and their total, one workgroup
//             compact_k     bit q set -> out[rank of q] = q (or src[q]): ascending whatever the launch geometry
//   Newton    newton_k      one lane per candidate, the 24 corner values in registers over all starts and iterations.
//                           <false>: one accepted-bit per candidate (mask and counts as above); after the second scan
//                           and compaction <true> repeats the iteration of the first max_nulls accepted cells - the
//                           same expressions, so the same bits - and writes their records.
// Nothing is appended atomically and no buffer's capacity is guessed: both lists are sized from their counts.
#include "line.hpp"

namespace {

using namespace ndsm;

constexpr int kCodeBlock = 256;        // node_code_k: two nodes per lane
constexpr int kMaskBlock = 1024;       // cell_mask_k: 16 mask words per workgroup
constexpr int kNewtonBlock = 256;      // newton_k: 4 mask words per workgroup
constexpr int kScanBlock = 1024;
constexpr int kCompactBlock = 256;

constexpr int kNullIters = 20;                       // Newton iterations per start
constexpr double kNullWander = 2.5;                  // |f_d - 1/2| beyond this: the start fails
constexpr double kNullConverged = 0x1p-40;           // max |delta_d| at or below this: converged
constexpr double kNullAcceptLo = -0x1p-30;           // accepted range of the converged fractions
constexpr double kNullAcceptHi = 1.0 + 0x1p-30;
constexpr unsigned kCodeClean = 64u;                 // bit 6: no NaN; bits 0-5: the strict signs

typedef unsigned long long u64;

__device__ __forceinline__ unsigned node_code(double a, double b, double c) {
  unsigned k = (a > 0.0 ? 1u : 0u) | (b > 0.0 ? 2u : 0u) | (c > 0.0 ? 4u : 0u) | (a < 0.0 ? 8u : 0u) |
               (b < 0.0 ? 16u : 0u) | (c < 0.0 ? 32u : 0u);
  if (a == a && b == b && c == c) k |= kCodeClean;
  return k;
}

// two neighbouring values in one load: the components start at B + m N, so only 8-byte alignment can be promised
struct __attribute__((aligned(8))) Pair {
  double a, b;
};

__global__ __launch_bounds__(kCodeBlock) void node_code_k(const double *__restrict__ B, size_t N,
                                                          uint8_t *__restrict__ code) {
  const size_t q = 2 * ((size_t)blockIdx.x * kCodeBlock + threadIdx.x);
  if (q + 1 < N) {
    const Pair x = *reinterpret_cast<const Pair *>(B + q);
    const Pair y = *reinterpret_cast<const Pair *>(B + N + q);
    const Pair z = *reinterpret_cast<const Pair *>(B + 2 * N + q);
    const unsigned k = node_code(x.a, y.a, z.a) | (node_code(x.b, y.b, z.b) << 8);
    *reinterpret_cast<uint16_t *>(code + q) = (uint16_t)k;
  } else if (q < N) {
    code[q] = (uint8_t)node_code(B[q], B[N + q], B[2 * N + q]);
  }
}

// one bit per lane into the mask word of the lane's wave, and the workgroup's count: every lane of the workgroup calls
// it (words holds gridDim.x kBlock / 64 words)
template <int kBlock>
__device__ __forceinline__ void put_mask(bool bit, size_t t, u64 *__restrict__ words, unsigned *__restrict__ counts) {
  __shared__ unsigned wc[kBlock / kWave];
  const u64 w = __ballot(bit);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    words[t >> 6] = w;
    wc[threadIdx.x >> 6] = (unsigned)__popcll(w);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned s = 0;
#pragma unroll
    for (int i = 0; i < kBlock / kWave; ++i) s += wc[i];
    counts[blockIdx.x] = s;
  }
}

struct MaskArgs {
  size_t N, sy, sz;
  int n[3];
};

__global__ __launch_bounds__(kMaskBlock) void cell_mask_k(const uint8_t *__restrict__ code, MaskArgs p,
                                                          u64 *__restrict__ words, unsigned *__restrict__ counts) {
  const size_t t = (size_t)blockIdx.x * kMaskBlock + threadIdx.x;
  bool cand = false;
  if (t < p.N) {
    bool inner;
    if (p.N <= (size_t)0xffffffffu) {          // (32-bit divisions where they suffice)
      const unsigned r = (unsigned)t / (unsigned)p.n[0], i = (unsigned)t - r * (unsigned)p.n[0];
      const unsigned k = r / (unsigned)p.n[1], j = r - k * (unsigned)p.n[1];
      inner = i + 1 < (unsigned)p.n[0] && j + 1 < (unsigned)p.n[1] && k + 1 < (unsigned)p.n[2];
    } else {
      const size_t r = t / (size_t)p.n[0], i = t - r * (size_t)p.n[0];
      const size_t k = r / (size_t)p.n[1], j = r - k * (size_t)p.n[1];
      inner = i + 1 < (size_t)p.n[0] && j + 1 < (size_t)p.n[1] && k + 1 < (size_t)p.n[2];
    }
    if (inner) {
      const uint8_t *__restrict__ q = code + t;
      const unsigned c = (unsigned)q[0] & q[1] & q[p.sy] & q[p.sy + 1] & q[p.sz] & q[p.sz + 1] & q[p.sz + p.sy] &
                         q[p.sz + p.sy + 1];
      cand = c == kCodeClean;
    }
  }
  put_mask<kMaskBlock>(cand, t, words, counts);
}

// offs[g] = counts[0] + ... + counts[g - 1], *total = the sum of all ng counts.  One workgroup: every lane sums a
// contiguous run, the kScanBlock run totals are scanned in LDS.
__global__ __launch_bounds__(kScanBlock) void scan_k(const unsigned *__restrict__ counts, size_t ng,
                                                     u64 *__restrict__ offs, long long *__restrict__ total) {
  __shared__ u64 part[kScanBlock];
  const size_t per = (ng + kScanBlock - 1) / kScanBlock;
  const size_t a = threadIdx.x * per < ng ? threadIdx.x * per : ng;
  const size_t b = a + per < ng ? a + per : ng;
  u64 s = 0;
  for (size_t q = a; q < b; ++q) s += counts[q];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int d = 1; d < kScanBlock; d <<= 1) {
    const u64 v = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  u64 run = part[threadIdx.x] - s;
  for (size_t q = a; q < b; ++q) {
    offs[q] = run;
    run += counts[q];
  }
  if (threadIdx.x == kScanBlock - 1) *total = (long long)part[kScanBlock - 1];
}

// every set bit q < m of the mask: out[rank] = src ? src[q] : q for rank < limit, rank = the number of set bits
// before q (offs: per group of wpg words)
__global__ __launch_bounds__(kCompactBlock) void compact_k(const u64 *__restrict__ words,
                                                           const u64 *__restrict__ offs, int wpg, size_t m,
                                                           const long long *__restrict__ src,
                                                           long long *__restrict__ out, size_t limit) {
  const size_t q = (size_t)blockIdx.x * kCompactBlock + threadIdx.x;
  if (q >= m) return;
  const size_t iw = q >> 6;
  const u64 w = words[iw];
  const int lane = (int)(q & 63);
  if (!((w >> lane) & 1ull)) return;
  const size_t g = iw / (size_t)wpg;
  u64 rank = offs[g];
  for (size_t ww = g * (size_t)wpg; ww < iw; ++ww) rank += (u64)__popcll(words[ww]);
  rank += (u64)__popcll(w & ((1ull << lane) - 1ull));
  if (rank < limit) out[rank] = src ? src[q] : (long long)q;
}

// det J by cofactor expansion along the first row, from the first column of the adjugate
__device__ __forceinline__ double det3(const double J[3][3], double &a00, double &a10, double &a20) {
  a00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  a10 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
  a20 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  return (J[0][0] * a00 + J[0][1] * a10) + J[0][2] * a20;
}

// The Newton iteration of one cell from its 24 corner values: true with the accepted fractions and
// iters = 32 start + iterations, or false.
__device__ __forceinline__ bool newton(const double v[3][8], double &fx, double &fy, double &fz, int &iters) {
#pragma unroll 1
  for (int s = 0; s < 9; ++s) {
    LineCell c;
    c.base = 0;
    c.fx = s == 0 ? 0.5 : (((s - 1) & 1) ? 0.75 : 0.25);
    c.fy = s == 0 ? 0.5 : (((s - 1) & 2) ? 0.75 : 0.25);
    c.fz = s == 0 ? 0.5 : (((s - 1) & 4) ? 0.75 : 0.25);
    bool converged = false;
    int it = 1;
#pragma unroll 1
    for (; it <= kNullIters; ++it) {
      double J[3][3], b[3];
#pragma unroll
      for (int m = 0; m < 3; ++m) b[m] = line_lerp3_fgrad(v[m], c, J[m]);
      double a00, a10, a20;
      const double det = det3(J, a00, a10, a20);
      if (!(fabs(det) > 0.0)) break;
      const double a01 = J[0][2] * J[2][1] - J[0][1] * J[2][2];
      const double a02 = J[0][1] * J[1][2] - J[0][2] * J[1][1];
      const double a11 = J[0][0] * J[2][2] - J[0][2] * J[2][0];
      const double a12 = J[0][2] * J[1][0] - J[0][0] * J[1][2];
      const double a21 = J[0][1] * J[2][0] - J[0][0] * J[2][1];
      const double a22 = J[0][0] * J[1][1] - J[0][1] * J[1][0];
      const double dx = ((a00 * b[0] + a01 * b[1]) + a02 * b[2]) / det;
      const double dy = ((a10 * b[0] + a11 * b[1]) + a12 * b[2]) / det;
      const double dz = ((a20 * b[0] + a21 * b[1]) + a22 * b[2]) / det;
      c.fx = c.fx - dx;
      c.fy = c.fy - dy;
      c.fz = c.fz - dz;
      if (!(fabs(c.fx - 0.5) <= kNullWander) || !(fabs(c.fy - 0.5) <= kNullWander) ||
          !(fabs(c.fz - 0.5) <= kNullWander))
        break;
      if (fmax(fmax(fabs(dx), fabs(dy)), fabs(dz)) <= kNullConverged) {
        converged = true;
        break;
      }
    }
    if (converged && c.fx >= kNullAcceptLo && c.fx <= kNullAcceptHi && c.fy >= kNullAcceptLo &&
        c.fy <= kNullAcceptHi && c.fz >= kNullAcceptLo && c.fz <= kNullAcceptHi) {
      fx = c.fx, fy = c.fy, fz = c.fz;
      iters = 32 * s + it;
      return true;
    }
  }
  return false;
}

struct NullOut {
  long long *cell;
  double *pos, *jac, *det, *resid;
  int32_t *sign, *iters;
};

// lane t: the cell cells[t] of m.  kEmit false: its accepted-bit into words / counts; true: its record into slot t
// (every cell of the list was accepted by the <false> pass).
template <bool kEmit>
__global__ __launch_bounds__(kNewtonBlock) void newton_k(const double *__restrict__ B,
                                                         const long long *__restrict__ cells, size_t m, LineArgs p,
                                                         u64 *__restrict__ words, unsigned *__restrict__ counts,
                                                         NullOut o) {
  const size_t t = (size_t)blockIdx.x * kNewtonBlock + threadIdx.x;
  const size_t sy = (size_t)p.n[0], sz = (size_t)p.n[0] * (size_t)p.n[1];
  const size_t N = sz * (size_t)p.n[2];
  bool ok = false;
  double fx = 0.0, fy = 0.0, fz = 0.0;
  int iters = 0;
  LineCell c;
  c.base = 0;
  double v[3][8];
  if (t < m) {
    c.base = (size_t)cells[t];
    line_gather(B, N, sy, sz, c, v);
    ok = newton(v, fx, fy, fz, iters);
  }
  if constexpr (!kEmit) {
    put_mask<kNewtonBlock>(ok, t, words, counts);
    return;
  }
  if (t >= m) return;
  c.fx = fx, c.fy = fy, c.fz = fz;
  double M[3][3], b[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) b[d] = line_lerp3_grad(v[d], c, p, M[d]);
  double a00, a10, a20;
  const double det = det3(M, a00, a10, a20);
  const size_t r = c.base / sy;
  const double ci = (double)(c.base - r * sy), cj = (double)(r % (size_t)p.n[1]), ck = (double)(r / (size_t)p.n[1]);
  o.cell[t] = (long long)c.base;
  o.pos[3 * t] = p.lo[0] + (ci + fx) * p.h[0];
  o.pos[3 * t + 1] = p.lo[1] + (cj + fy) * p.h[1];
  o.pos[3 * t + 2] = p.lo[2] + (ck + fz) * p.h[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int d = 0; d < 3; ++d) o.jac[9 * t + 3 * a + d] = M[a][d];
  }
  o.det[t] = det;
  o.resid[t] = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
  o.sign[t] = det < 0.0 ? 1 : (det > 0.0 ? -1 : 0);
  o.iters[t] = iters;
}

// scratch of the call, kept between calls and grown on demand (no result depends on its size): a the screen's
// arrays, b the lists of the Newton stage; two pinned counts
struct NullScratch {
  void *a = nullptr, *b = nullptr;
  size_t cap_a = 0, cap_b = 0;
  long long *d_tot = nullptr, *h_pin = nullptr;
  bool registered = false;     // nul_release is queued for the next reset
};
NullScratch g_nul;

void nul_release() {
  if (g_nul.a) (void)hipFree(g_nul.a);
  if (g_nul.b) (void)hipFree(g_nul.b);
  if (g_nul.d_tot) (void)hipFree(g_nul.d_tot);
  if (g_nul.h_pin) (void)hipHostFree(g_nul.h_pin);
  g_nul = NullScratch();
}

int nul_grow(void *&p, size_t &cap, size_t bytes) {
  if (!g_nul.registered) {
    ndsm::at_reset(nul_release);
    g_nul.registered = true;
  }
  if (!g_nul.d_tot) NDSM_HIP(hipMalloc((void **)&g_nul.d_tot, 2 * sizeof(long long)));
  if (!g_nul.h_pin) NDSM_HIP(hipHostMalloc((void **)&g_nul.h_pin, 2 * sizeof(long long), hipHostMallocDefault));
  if (bytes <= cap) return 0;
  if (p) {
    const int rc = ndsmk_free(p);      // (drains the streams first)
    p = nullptr;
    cap = 0;
    if (rc != 0) return rc;
  }
  const int rc = ndsmk_alloc(&p, bytes);
  if (rc != 0) return rc;
  cap = bytes;
  return 0;
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the count a scan left in d_tot[which], on the host (blocking)
int nul_count(int which, long long &out) {
  hipStream_t s = ndsm::stream();
  NDSM_HIP(hipMemcpyAsync(g_nul.h_pin + which, g_nul.d_tot + which, sizeof(long long), hipMemcpyDeviceToHost, s));
  NDSM_HIP(hipStreamSynchronize(s));
  out = g_nul.h_pin[which];
  return 0;
}

}  // namespace

// Nulls of B (nx,ny,nz,3), a DEVICE array.  lo3, h_dq3: the mesh's first point and spacing per axis.  h_counts2 (HOST):
// candidates of the screen, nulls found.  The first min(found, max_nulls) records in ascending cell order go into the
// DEVICE arrays cell (int64), pos (3 each), jac (9 each), det, resid, sign, iters (not looked at with max_nulls == 0).
// Blocks for the two counts; the records are written asynchronously.
extern "C" int ndsmk_nulls(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, int max_nulls,
                           int64_t *h_counts2, int64_t *cell, double *pos, double *jac, double *det, double *resid,
                           int32_t *sign, int32_t *iters) {
  NDSM_REQUIRE_READY();
  if (max_nulls < 0) return fail(NDSMK_EVALUE, "nulls: max_nulls >= 0", __FILE__, __LINE__);
  NDSM_CHECK_ARG(B && h_counts2 && (max_nulls == 0 || (cell && pos && jac && det && resid && sign && iters)));
  NDSM_CHECK_ARG(n3[0] >= 2 && n3[1] >= 2 && n3[2] >= 2 && h_dq3[0] > 0.0 && h_dq3[1] > 0.0 && h_dq3[2] > 0.0);
  h_counts2[0] = h_counts2[1] = 0;
  LineArgs p;
  for (int d = 0; d < 3; ++d) {
    p.n[d] = n3[d];
    p.lo[d] = lo3[d];
    p.h[d] = h_dq3[d];
    p.hi[d] = lo3[d] + (double)(n3[d] - 1) * h_dq3[d];
  }
  p.ds = 0.0;
  p.max_steps = 0;
  p.nseeds = 0;
  MaskArgs q;
  q.sy = (size_t)n3[0];
  q.sz = q.sy * (size_t)n3[1];
  q.N = q.sz * (size_t)n3[2];
  for (int d = 0; d < 3; ++d) q.n[d] = n3[d];
  const size_t N = q.N;
  const size_t nbc = (N + 2 * kCodeBlock - 1) / (2 * kCodeBlock);
  const size_t nbm = (N + kMaskBlock - 1) / kMaskBlock;
  NDSM_CHECK_ARG(nbc <= (size_t)0x7fffffff);

  // the screen: codes, mask words, workgroup counts, their exclusive sums
  const size_t b_code = up256(N + 2), b_words = up256(nbm * (kMaskBlock / kWave) * sizeof(u64));
  const size_t b_cnt = up256(nbm * sizeof(unsigned)), b_offs = up256(nbm * sizeof(u64));
  int rc = nul_grow(g_nul.a, g_nul.cap_a, b_code + b_words + b_cnt + b_offs);
  if (rc != 0) return rc;
  uint8_t *code = (uint8_t *)g_nul.a;
  u64 *words = (u64 *)(code + b_code);
  unsigned *counts = (unsigned *)((uint8_t *)words + b_words);
  u64 *offs = (u64 *)((uint8_t *)counts + b_cnt);
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(node_code_k, dim3((unsigned)nbc), dim3(kCodeBlock), 0, s, B, N, code);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(cell_mask_k, dim3((unsigned)nbm), dim3(kMaskBlock), 0, s, code, q, words, counts);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(scan_k, dim3(1), dim3(kScanBlock), 0, s, counts, nbm, offs, g_nul.d_tot);
  NDSM_LAUNCH_CHECK();
  long long ncand = 0;
  rc = nul_count(0, ncand);
  if (rc != 0) return rc;
  h_counts2[0] = ncand;
  if (ncand == 0) return 0;

  // the Newton stage: the candidate list, its accepted-mask, counts and sums, the accepted list
  const size_t nc = (size_t)ncand;
  const size_t nbn = (nc + kNewtonBlock - 1) / kNewtonBlock;
  const size_t lim = (size_t)max_nulls < nc ? (size_t)max_nulls : nc;
  const size_t b_cand = up256(nc * sizeof(long long)), b_w2 = up256(nbn * (kNewtonBlock / kWave) * sizeof(u64));
  const size_t b_c2 = up256(nbn * sizeof(unsigned)), b_o2 = up256(nbn * sizeof(u64));
  const size_t b_acc = up256((lim + 1) * sizeof(long long));
  rc = nul_grow(g_nul.b, g_nul.cap_b, b_cand + b_w2 + b_c2 + b_o2 + b_acc);
  if (rc != 0) return rc;
  long long *cand = (long long *)g_nul.b;
  u64 *words2 = (u64 *)((uint8_t *)cand + b_cand);
  unsigned *counts2 = (unsigned *)((uint8_t *)words2 + b_w2);
  u64 *offs2 = (u64 *)((uint8_t *)counts2 + b_c2);
  long long *acc = (long long *)((uint8_t *)offs2 + b_o2);
  const NullOut none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(compact_k, dim3((unsigned)((N + kCompactBlock - 1) / kCompactBlock)), dim3(kCompactBlock), 0, s,
                     words, offs, kMaskBlock / kWave, N, (const long long *)nullptr, cand, nc);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(newton_k<false>, dim3((unsigned)nbn), dim3(kNewtonBlock), 0, s, B, cand, nc, p, words2, counts2,
                     none);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(scan_k, dim3(1), dim3(kScanBlock), 0, s, counts2, nbn, offs2, g_nul.d_tot + 1);
  NDSM_LAUNCH_CHECK();
  long long nfound = 0;
  rc = nul_count(1, nfound);
  if (rc != 0) return rc;
  h_counts2[1] = nfound;
  const size_t nout = (size_t)nfound < lim ? (size_t)nfound : lim;
  if (nout == 0) return 0;
  hipLaunchKernelGGL(compact_k, dim3((unsigned)((nc + kCompactBlock - 1) / kCompactBlock)), dim3(kCompactBlock), 0, s,
                     words2, offs2, kNewtonBlock / kWave, nc, cand, acc, nout);
  NDSM_LAUNCH_CHECK();
  const NullOut o = {(long long *)cell, pos, jac, det, resid, sign, iters};
  hipLaunchKernelGGL(newton_k<true>, dim3((unsigned)((nout + kNewtonBlock - 1) / kNewtonBlock)), dim3(kNewtonBlock), 0,
                     s, B, acc, nout, p, (u64 *)nullptr, (unsigned *)nullptr, o);
  NDSM_LAUNCH_CHECK();
  return 0;
}
