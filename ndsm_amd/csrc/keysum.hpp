// Keyed sums (DESIGN.md "Flux partitioning and connectivity", include/ndsm_hip.h "keyed sum"): sums grouped by a key
// that the data decide, with the same bits on every run.  Shared by partition.hip and connect.hip.
//
// Item p = 0 .. n - 1 (a pixel) carries a 64-bit key; key 0 means "no key" and is summed nowhere.  The run of a key is
// the segment of its items after a STABLE sort of (key, item) by key, so inside a run the items ascend.  That order is
// unique: any correct stable sort gives it, and the sums below are specified on it alone.
//
//   sort    ks_count_k    LSD radix, 8 bits a pass, 1024 items per workgroup, one item per lane.  The lanes of a wave
//                         with a lane's digit are its match mask, from eight ballots; the number of them below the lane
//                         is its rank in the wave (stable: lanes ascend with the items).  The lowest lane of a mask is
//                         the one writer of its (wave, digit) count in LDS.  Counts go out digit-major, block-minor.
//           scan64_k      the exclusive sums of that array: where each (digit, block) starts
//           ks_scatter_k  the same ranks again; item -> start of its (digit, block) + the waves before + its rank
//   runs    ks_flag_k     1 where a key other than 0 differs from the one before, scan64_k numbers the runs and counts
//           ks_head_k     them, start[m] = where run m begins; run m ends where run m + 1 begins, the last at n
//   sums    ks_wave_sum   one wave per run: lane l adds the ranks l, l + 64, ... in that order from 0.0, then
//                         v[l] = v[l] + v[l + d] for l < d, d = 32, 16, ... 1; the sum is v[0]
// No atomics anywhere: the launch shape fixes every order.  The passes are decided on the host from the largest key.
#pragma once

#include "scan64.hpp"

namespace ndsm {
namespace {

typedef unsigned long long u64;

constexpr int kKsBlock = 1024;
constexpr int kKsWaves = kKsBlock / kWave;
constexpr int kKsDigits = 256;

// the lanes of the wave that hold digit d (looked at by valid lanes only)
__device__ __forceinline__ u64 ks_match(unsigned d, bool valid) {
  u64 m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = ((d >> b) & 1u) != 0u;
    const u64 w = __ballot(valid && bit);
    m &= bit ? w : ~w;
  }
  return m;
}

// item t of the pass: its digit, its rank among the lanes of its wave with that digit, and wc[wave][digit] <- how many
// of those there are.  wc is cleared here; a barrier follows the writes.
__device__ __forceinline__ void ks_rank(const u64 *__restrict__ key, size_t n, int shift, unsigned (*wc)[kKsDigits],
                                        size_t t, bool &valid, unsigned &d, unsigned &rank) {
  for (int q = threadIdx.x; q < kKsWaves * kKsDigits; q += kKsBlock) (&wc[0][0])[q] = 0u;
  __syncthreads();
  valid = t < n;
  d = valid ? (unsigned)((key[t] >> shift) & 255ull) : 0u;
  const u64 m = ks_match(d, valid);
  const int lane = (int)(threadIdx.x & (kWave - 1));
  rank = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
  if (valid && rank == 0u) wc[threadIdx.x >> 6][d] = (unsigned)__popcll(m);
  __syncthreads();
}

// cnt[d nb + block] <- the items of the block with digit d
__global__ __launch_bounds__(kKsBlock) void ks_count_k(const u64 *__restrict__ key, size_t n, int shift,
                                                       i64 *__restrict__ cnt, size_t nb) {
  __shared__ unsigned wc[kKsWaves][kKsDigits];
  bool valid;
  unsigned d, rank;
  ks_rank(key, n, shift, wc, (size_t)blockIdx.x * kKsBlock + threadIdx.x, valid, d, rank);
  if (threadIdx.x < kKsDigits) {
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < kKsWaves; ++w) s += wc[w][threadIdx.x];
    cnt[(size_t)threadIdx.x * nb + blockIdx.x] = (i64)s;
  }
}

// offs: cnt after the scan
__global__ __launch_bounds__(kKsBlock) void ks_scatter_k(const u64 *__restrict__ key, const unsigned *__restrict__ idx,
                                                         size_t n, int shift, const i64 *__restrict__ offs, size_t nb,
                                                         u64 *__restrict__ key_out, unsigned *__restrict__ idx_out) {
  __shared__ unsigned wc[kKsWaves][kKsDigits];
  bool valid;
  unsigned d, rank;
  const size_t t = (size_t)blockIdx.x * kKsBlock + threadIdx.x;
  ks_rank(key, n, shift, wc, t, valid, d, rank);
  if (threadIdx.x < kKsDigits) {
    unsigned run = 0;
#pragma unroll
    for (int w = 0; w < kKsWaves; ++w) {
      const unsigned c = wc[w][threadIdx.x];
      wc[w][threadIdx.x] = run;
      run += c;
    }
  }
  __syncthreads();
  if (!valid) return;
  const size_t pos = (size_t)offs[(size_t)d * nb + blockIdx.x] + wc[threadIdx.x >> 6][d] + rank;
  if (pos >= n) return;               // (the counts add up to n: never taken)
  key_out[pos] = key[t];
  idx_out[pos] = idx[t];
}

__device__ __forceinline__ bool ks_is_head(const u64 *__restrict__ sk, size_t q) {
  const u64 k = sk[q];
  return k != 0ull && (q == 0 || sk[q - 1] != k);
}

__global__ __launch_bounds__(256) void ks_flag_k(const u64 *__restrict__ sk, size_t n, i64 *__restrict__ flag) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q < n) flag[q] = ks_is_head(sk, q) ? 1 : 0;
}

// runid: flag after the scan
__global__ __launch_bounds__(256) void ks_head_k(const u64 *__restrict__ sk, size_t n, const i64 *__restrict__ runid,
                                                 i64 *__restrict__ start) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q < n && ks_is_head(sk, q)) start[runid[q]] = (i64)q;
}

// The keyed sums of NV values over the sorted items [s0, s1) of one run, by one whole wave: term(item, t) gives the NV
// terms of an item.  Every lane returns; lane 0 holds the sums.
template <int NV, class F>
__device__ __forceinline__ void ks_wave_sum(const unsigned *__restrict__ sidx, i64 s0, i64 s1, int lane, const F &term,
                                            double v[NV]) {
#pragma unroll
  for (int c = 0; c < NV; ++c) v[c] = 0.0;
  for (i64 q = s0 + lane; q < s1; q += kWave) {
    double t[NV];
    term(sidx[q], t);
#pragma unroll
    for (int c = 0; c < NV; ++c) v[c] = v[c] + t[c];
  }
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
#pragma unroll
    for (int c = 0; c < NV; ++c) v[c] = v[c] + __shfl_down(v[c], (unsigned)d, kWave);   // (lanes >= d: not read again)
  }
}

// the arrays of a sort of n items, carved from one allocation
struct KsBuf {
  u64 *key[2];
  unsigned *idx[2];
  i64 *cnt;        // [256 nb + 1]
  i64 *flag;       // [n + 1]
  i64 *start;      // [n + 1]
};

inline size_t ks_up256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t ks_blocks(size_t n) { return (n + kKsBlock - 1) / kKsBlock; }

inline size_t ks_bytes(size_t n) {
  return 2 * ks_up256(n * sizeof(u64)) + 2 * ks_up256(n * sizeof(unsigned)) +
         ks_up256((kKsDigits * ks_blocks(n) + 1) * sizeof(i64)) + 2 * ks_up256((n + 1) * sizeof(i64));
}

inline void ks_carve(void *base, size_t n, KsBuf &b) {
  uint8_t *at = (uint8_t *)base;
  for (int c = 0; c < 2; ++c) b.key[c] = (u64 *)at, at += ks_up256(n * sizeof(u64));
  for (int c = 0; c < 2; ++c) b.idx[c] = (unsigned *)at, at += ks_up256(n * sizeof(unsigned));
  b.cnt = (i64 *)at, at += ks_up256((kKsDigits * ks_blocks(n) + 1) * sizeof(i64));
  b.flag = (i64 *)at, at += ks_up256((n + 1) * sizeof(i64));
  b.start = (i64 *)at;
}

// The scratch of a translation unit's entry, kept between calls and grown on demand (no result depends on its size):
// one allocation for the sort's arrays and what the entry adds behind them, and two pinned counts.
struct KsScratch {
  void *a = nullptr;
  size_t cap = 0;
  long long *h_pin = nullptr;  // [2]
  bool registered = false;     // ks_release is queued for the next reset
};
KsScratch g_ks;

void ks_release() {
  if (g_ks.a) (void)hipFree(g_ks.a);
  if (g_ks.h_pin) (void)hipHostFree(g_ks.h_pin);
  g_ks = KsScratch();
}

int ks_grow(size_t bytes) {
  if (!g_ks.registered) {
    ndsm::at_reset(ks_release);
    g_ks.registered = true;
  }
  if (!g_ks.h_pin) NDSM_HIP(hipHostMalloc((void **)&g_ks.h_pin, 2 * sizeof(long long), hipHostMallocDefault));
  if (bytes <= g_ks.cap) return 0;
  if (g_ks.a) {
    const int rc = ndsmk_free(g_ks.a);      // (drains the streams first)
    g_ks.a = nullptr;
    g_ks.cap = 0;
    if (rc != 0) return rc;
  }
  const int rc = ndsmk_alloc(&g_ks.a, bytes);
  if (rc != 0) return rc;
  g_ks.cap = bytes;
  return 0;
}

// the digit passes that keys up to max_key need (at least one)
inline int ks_passes(u64 max_key) {
  int bits = 0;
  while (max_key) ++bits, max_key >>= 1;
  return bits <= 8 ? 1 : (bits + 7) / 8;
}

// key[0], idx[0] sorted stably by key; *fin: the pair of arrays that holds the result.  Then the runs: flag scanned,
// start filled, flag[n] = the number of runs.  Asynchronous.
inline int ks_sort_runs(const KsBuf &b, size_t n, u64 max_key, hipStream_t s, int *fin) {
  const size_t nb = ks_blocks(n);
  const int passes = ks_passes(max_key);
  int cur = 0;
  for (int pass = 0; pass < passes; ++pass) {
    hipLaunchKernelGGL(ks_count_k, dim3((unsigned)nb), dim3(kKsBlock), 0, s, b.key[cur], n, 8 * pass, b.cnt, nb);
    NDSM_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan64_k, dim3(1), dim3(kScanBlock), 0, s, b.cnt, (size_t)kKsDigits * nb);
    NDSM_LAUNCH_CHECK();
    hipLaunchKernelGGL(ks_scatter_k, dim3((unsigned)nb), dim3(kKsBlock), 0, s, b.key[cur], b.idx[cur], n, 8 * pass,
                       b.cnt, nb, b.key[1 - cur], b.idx[1 - cur]);
    NDSM_LAUNCH_CHECK();
    cur = 1 - cur;
  }
  *fin = cur;
  const unsigned ng = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(ks_flag_k, dim3(ng), dim3(256), 0, s, b.key[cur], n, b.flag);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(scan64_k, dim3(1), dim3(kScanBlock), 0, s, b.flag, n);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(ks_head_k, dim3(ng), dim3(256), 0, s, b.key[cur], n, b.flag, b.start);
  NDSM_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace ndsm
