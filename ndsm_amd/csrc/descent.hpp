// What the pseudo-time descents that decide their steps on the device share (DESIGN.md "Shared descent machinery"):
// optimize.hip, optimize_obs.hip and preprocess.hip.  Four pieces:
//
//   block_part / block_final : the deterministic two-stage reduction of NV values per thread, the first NS of them sums,
//                              the others maxima.  A part kernel ends with block_part (fill, 256-wide halving tree, one
//                              row of block partials); a one-block final kernel starts with block_final (thread t folds
//                              the partials of blocks t, t + 256, ... in that order, then the same tree).  field.hip's
//                              and project.hip's reductions are the same two calls.
//   DescentState             : the device-resident state of a descent, all doubles: one history row, then the control
//                              words.  [tries, L, terms.., dt, accepted, extras.., cur, stop, tail..]
//   descent_decide           : the accept/reject rule, run by the one deciding thread of a final kernel.
//   descent_begin, descent_row, descent_work_bytes : the host side of the state.
//
// No atomics anywhere: the order of every sum is fixed by the launch shape, so the same input gives the same bits.
#pragma once

#include "common.hpp"

namespace ndsm {

constexpr int kRedBlock = 256;
constexpr int kRedMaxBlocks = 2048;   // 256 CUs x 8 blocks; rows beyond that are strided

// the blocks of a part kernel that walks nrows rows
inline int red_blocks(size_t nrows) { return (int)(nrows < (size_t)kRedMaxBlocks ? nrows : (size_t)kRedMaxBlocks); }

// halving tree over the block: sh[q][t] = sh[q][t] (+ or fmax) sh[q][t + o] for o = 128 .. 1; sh[q][0] is the result
template <int NV, int NS>
__device__ __forceinline__ void block_tree(double (*sh)[kRedBlock], const double *v) {
  const int t = threadIdx.x;
  for (int q = 0; q < NV; ++q) sh[q][t] = v[q];
  __syncthreads();
  for (int o = kRedBlock / 2; o > 0; o >>= 1) {
    if (t < o) {   // (all rows are read before one is written: the LDS reads of a step then go out together)
      double a[NV];
      for (int q = 0; q < NS; ++q) a[q] = sh[q][t] + sh[q][t + o];
      for (int q = NS; q < NV; ++q) a[q] = fmax(sh[q][t], sh[q][t + o]);
      for (int q = 0; q < NV; ++q) sh[q][t] = a[q];
    }
    __syncthreads();
  }
}

// the end of a part kernel: the tree over the threads' v, then this block's row of partials (stride doubles per row)
template <int NV, int NS>
__device__ __forceinline__ void block_part(double (*sh)[kRedBlock], const double *v, double *__restrict__ part,
                                           int stride = NV) {
  block_tree<NV, NS>(sh, v);
  if (threadIdx.x < NV) part[(size_t)blockIdx.x * stride + threadIdx.x] = sh[threadIdx.x][0];
}

// the start of a one-block final kernel: thread t folds the partials of blocks t, t + 256, ... in that order, then the
// tree; every thread may read sh[q][0] afterwards
template <int NV, int NS>
__device__ __forceinline__ void block_final(double (*sh)[kRedBlock], const double *__restrict__ part, int nb,
                                            int stride = NV) {
  double v[NV];
  for (int q = 0; q < NV; ++q) v[q] = 0.0;
  for (int b = threadIdx.x; b < nb; b += kRedBlock) {
    for (int q = 0; q < NS; ++q) v[q] = v[q] + part[(size_t)b * stride + q];
    for (int q = NS; q < NV; ++q) v[q] = fmax(v[q], part[(size_t)b * stride + q]);
  }
  block_tree<NV, NS>(sh, v);
}

// The state of a descent with NT reported terms of L, NX further words of the history row and NTAIL words behind the
// control words.  The first ROW doubles are a history row as the host hands it out.
template <int NT, int NX = 0, int NTAIL = 0>
struct DescentState {
  enum {
    TRIES = 0, L = 1, TERM = 2, DT = 2 + NT, ACCEPTED = 3 + NT, EXTRA = 4 + NT, ROW = 4 + NT + NX,
    CUR = ROW,          // which of the two buffers is current (0 or 1)
    STOP = ROW + 1,     // raised once dt < dt_min: every later launch returns at once
    TAIL = ROW + 2, LEN = ROW + 2 + NTAIL
  };
};

// The decision, by one thread: l is L of the field just evaluated - the start field (trial = false: it is current by
// definition) or the trial field of a try.  L_T < L accepts: the buffer index flips, dt grows by 1.01; anything else -
// a NaN on either side included - rejects: dt halves.  A dt below dt_min raises the stop flag.  Returns whether the
// evaluated field is now the current one; L is stored here, the caller stores its own terms.
template <class S>
__device__ __forceinline__ bool descent_decide(double *__restrict__ state, double l, bool trial, double dt_min) {
  double dt = state[S::DT];
  bool keep = !trial;
  if (trial) {
    state[S::TRIES] = state[S::TRIES] + 1.0;
    if (l < state[S::L]) {
      keep = true;
      state[S::CUR] = 1.0 - state[S::CUR];
      state[S::ACCEPTED] = state[S::ACCEPTED] + 1.0;
      dt = dt * 1.01;
    } else {
      dt = dt * 0.5;
    }
    state[S::DT] = dt;
  }
  if (keep) state[S::L] = l;
  if (dt < dt_min) state[S::STOP] = 1.0;
  return keep;
}

template <class S>
__global__ void descent_state_k(double *__restrict__ state, double dt0) {
  if (threadIdx.x < S::LEN) state[threadIdx.x] = threadIdx.x == S::DT ? dt0 : 0.0;
}

// the work area of a descent: the state, then kRedMaxBlocks rows of NSUMS block partials
template <class S, int NSUMS>
constexpr size_t descent_work_bytes() {
  return sizeof(double) * (S::LEN + (size_t)kRedMaxBlocks * NSUMS);
}

// the state of a call that begins: tries 0, dt0, buffer 0 current.  Asynchronous.
template <class S>
int descent_begin(double *work, double dt0) {
  static_assert(S::LEN <= 64, "descent_state_k is launched with 64 threads");
  hipLaunchKernelGGL(descent_state_k<S>, dim3(1), dim3(64), 0, stream(), work, dt0);
  NDSM_LAUNCH_CHECK();
  return 0;
}

// Blocking.  h_row (host) = the S::LEN doubles of the state
template <class S>
int descent_row(const double *work, double *h_row) {
  hipStream_t s = stream();
  NDSM_HIP(hipMemcpyAsync(h_row, work, S::LEN * sizeof(double), hipMemcpyDeviceToHost, s));
  NDSM_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // namespace ndsm
