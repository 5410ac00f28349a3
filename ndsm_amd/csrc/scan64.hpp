// The in-place int64 exclusive scan of one workgroup and the tail of a counting half built on it, shared by paths.hip,
// skeleton.hip and separators.hip (count, scan, fill: the offsets of variable-length results come from their counts).
#pragma once

#include "common.hpp"

namespace ndsm {
namespace {

constexpr int kScanBlock = 1024;

// in place: a[q] <- a[0] + ... + a[q - 1] for q < ng, a[ng] <- the sum of all.  One workgroup: every lane sums a
// contiguous run and rewrites that run alone; the kScanBlock run totals are scanned in LDS.
__global__ __launch_bounds__(kScanBlock) void scan64_k(i64 *a, size_t ng) {
  __shared__ i64 part[kScanBlock];
  const size_t per = (ng + kScanBlock - 1) / kScanBlock;
  const size_t lo = threadIdx.x * per < ng ? threadIdx.x * per : ng;
  const size_t hi = lo + per < ng ? lo + per : ng;
  i64 s = 0;
  for (size_t q = lo; q < hi; ++q) s += a[q];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int d = 1; d < kScanBlock; d <<= 1) {
    const i64 v = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  i64 run = part[threadIdx.x] - s;
  for (size_t q = lo; q < hi; ++q) {
    const i64 c = a[q];
    a[q] = run;
    run += c;
  }
  if (threadIdx.x == kScanBlock - 1) a[ng] = part[kScanBlock - 1];
}

// the tail of a counting half: offsets (ng counts, DEVICE) scanned in place, the total offsets[ng] into *h_total
// (HOST).  Blocks for the total.
[[maybe_unused]] int scan64_total(int64_t *offsets, size_t ng, int64_t *h_total, hipStream_t s) {
  hipLaunchKernelGGL(scan64_k, dim3(1), dim3(kScanBlock), 0, s, (i64 *)offsets, ng);
  NDSM_LAUNCH_CHECK();
  NDSM_HIP(hipMemcpyAsync(h_total, offsets + ng, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  NDSM_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // namespace
}  // namespace ndsm
