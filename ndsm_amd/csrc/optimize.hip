// The optimization-method force-free solver on the device (DESIGN.md "Optimization-method force-free field";
// Wheatland, Sturrock & Roumeliotis 2000; Wiegelmann 2004).  One try of the iteration is three launches:
//
//   opt_force_k : optimize_core.hpp's force pass without the measurement flag: the TRIAL field T = B + dt F~ on the
//                 interior nodes, T = B on the six faces.  Streaming, one thread per node: 56 B/pt in (B, Omega, w),
//                 24 out.
//   opt_omega_k : optimize_core.hpp's Omega pass without the flag: Omega of the trial (at the start: the current) field
//                 and the block partials of L_f and L_d: 24 B/pt in (+ 8 of w), 24 out.
//   opt_final_k : one block: descent.hpp's fold and tree over the partials, then ONE thread forms L = L_f + L_d and
//                 runs descent.hpp's decision: L_T < L accepts (the buffer index flips, dt grows by 1.01), anything
//                 else - a NaN included - rejects (dt halves).
//
// Which of the two B and the two Omega buffers is "current" is a number in the device-resident state (descent.hpp's
// DescentState), and so are dt, L and the counters: the kernels of the next try read them from there, and the host
// reads nothing back between two checks.  A dt below dt_min raises the state's stop flag; the launches already queued
// behind it return at once.  Every step is deterministic and the library is built without contraction:
// tests/optimize_model.py restates the iteration in numpy bit for bit.
#include "optimize_core.hpp"

namespace {

using ndsm::kRedBlock;
using ndsm::OptArgs;

constexpr int kOptSums = 2;                 // L_f, L_d
using OptState = ndsm::DescentState<2>;     // the state: one history row of 6 doubles, the buffer index, the stop flag

// which = 0: Omega and the sums of the current field (the start); which = 1: of the trial field
__global__ __launch_bounds__(kRedBlock) void opt_omega_k(const double *__restrict__ B0, const double *__restrict__ B1,
                                                        double *__restrict__ O0, double *__restrict__ O1,
                                                        const double *__restrict__ wt, double *__restrict__ part,
                                                        const double *__restrict__ state, int which, OptArgs p) {
  __shared__ double sh[kOptSums][kRedBlock];
  ndsm::omega_pass<OptState, false>(sh, B0, B1, O0, O1, wt, nullptr, nullptr, part, state, which, p);
}

// one block: the fold and tree over the partials of opt_omega_k, then thread 0 decides
__global__ __launch_bounds__(kRedBlock) void opt_final_k(const double *__restrict__ part, int nb,
                                                        double *__restrict__ state, int which, double dt_min) {
  __shared__ double sh[kOptSums][kRedBlock];
  if (state[OptState::STOP] != 0.0) return;
  ndsm::block_final<kOptSums, kOptSums>(sh, part, nb);
  if (threadIdx.x != 0) return;
  const double lf = sh[0][0], ld = sh[1][0];
  if (ndsm::descent_decide<OptState>(state, lf + ld, which != 0, dt_min)) {
    state[OptState::TERM] = lf;
    state[OptState::TERM + 1] = ld;
  }
}

// T = B + dt F~ inside, T = B on the faces; B, Omega: the current buffers, T: the other B buffer
__global__ __launch_bounds__(256) void opt_force_k(double *__restrict__ B0, double *__restrict__ B1,
                                                   const double *__restrict__ O0, const double *__restrict__ O1,
                                                   const double *__restrict__ wt, const double *__restrict__ state,
                                                   OptArgs p) {
  ndsm::force_pass<OptState, false>(B0, B1, O0, O1, wt, nullptr, nullptr, state, p, 0.0, 0);
}

int opt_evaluate(double *B0, double *B1, double *O, const double *w, double *work, const OptArgs &p, int which,
                 double dt_min) {
  const size_t N3 = 3 * (size_t)p.n[0] * (size_t)p.n[1] * (size_t)p.n[2];
  const int nb = ndsm::red_blocks(p.nrows);
  double *state = work, *part = work + OptState::LEN;
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(opt_omega_k, dim3(nb), dim3(kRedBlock), 0, s, B0, B1, O, O + N3, w, part, state, which, p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(opt_final_k, dim3(1), dim3(kRedBlock), 0, s, part, nb, state, which, dt_min);
  NDSM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" size_t ndsmk_optimize_work_bytes(void) { return ndsm::descent_work_bytes<OptState, kOptSums>(); }

// The start: the state (tries 0, dt0, buffer 0 current), then Omega and L of B0.  Asynchronous.
extern "C" int ndsmk_optimize_begin(double *B0, double *B1, double *O, const double *w, double *work,
                                    const int32_t *n3, const double *h_dq3, double dt0, double dt_min) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B0 && B1 && O && work);
  OptArgs p;
  if (int rc = ndsm::opt_args(n3, h_dq3, p)) return rc;
  if (int rc = ndsm::descent_begin<OptState>(work, dt0)) return rc;
  return opt_evaluate(B0, B1, O, w, work, p, 0, dt_min);
}

// ntries tries, each the force-and-update pass, the Omega pass of the trial field and the decision.  Asynchronous:
// nothing is read back.
extern "C" int ndsmk_optimize_tries(double *B0, double *B1, double *O, const double *w, double *work,
                                    const int32_t *n3, const double *h_dq3, double dt_min, int ntries) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B0 && B1 && O && work && ntries >= 0);
  OptArgs p;
  if (int rc = ndsm::opt_args(n3, h_dq3, p)) return rc;
  const size_t N3 = 3 * (size_t)n3[0] * (size_t)n3[1] * (size_t)n3[2];
  dim3 grid, block;
  ndsm::force_shape(p, grid, block);
  for (int it = 0; it < ntries; ++it) {
    hipLaunchKernelGGL(opt_force_k, grid, block, 0, ndsm::stream(), B0, B1, O, O + N3, w, work, p);
    NDSM_LAUNCH_CHECK();
    if (int rc = opt_evaluate(B0, B1, O, w, work, p, 1, dt_min)) return rc;
  }
  return 0;
}

// Blocking.  h_row8 (host) = [tries, L, L_f, L_d, dt, accepted, current buffer (0: B0, 1: B1), stop flag (dt < dt_min)]
extern "C" int ndsmk_optimize_row(const double *work, double *h_row8) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(work && h_row8);
  return ndsm::descent_row<OptState>(work, h_row8);
}
