// The optimization method with a measurement term and a freed lower face (DESIGN.md "Measurement errors and a freed
// lower face"; Wiegelmann & Inhester 2010, Wiegelmann et al. 2012): optimize.hip's three launches per try with
// optimize_core.hpp's passes instantiated WITH the measurement flag:
//
//   obs_force_k : the k = 0 plane is a branch (k is blockIdx.z: uniform per block).  Its rim is copied; with free = 1
//                 its other nodes get T = B + dt H,  H = (F~ + c G) - c (nu (wm (B - Bobs))),  c = 2 / h_z.  Every other
//                 node is optimize.hip's: T = B + dt F~ inside, T = B on the five other faces.
//   obs_omega_k : a third sum through the same row walk and tree: the threads of the rows with k = 0 add
//                 W2 ((wm_x dx dx + wm_y dy dy) + wm_z dz dz), d = B - Bobs, W2 = w_x w_y; the others add nothing.
//   obs_final_k : L = (L_f + L_d) + nu L_m, formed by the deciding thread; the decision is descent.hpp's.
//
// The state is one history row (7 doubles) plus the buffer index and the stop flag.  No atomics; every step is
// deterministic and the library is built without contraction: tests/optimize_obs_model.py restates the iteration in
// numpy bit for bit.
#include "optimize_core.hpp"

namespace {

using ndsm::kRedBlock;
using ndsm::OptArgs;

constexpr int kObsSums = 3;                 // L_f, L_d, L_m
using ObsState = ndsm::DescentState<3>;

// which = 0: Omega and the sums of the current field (the start); which = 1: of the trial field
__global__ __launch_bounds__(kRedBlock) void obs_omega_k(const double *__restrict__ B0, const double *__restrict__ B1,
                                                        double *__restrict__ O0, double *__restrict__ O1,
                                                        const double *__restrict__ wt, const double *__restrict__ Bobs,
                                                        const double *__restrict__ wm, double *__restrict__ part,
                                                        const double *__restrict__ state, int which, OptArgs p) {
  __shared__ double sh[kObsSums][kRedBlock];
  ndsm::omega_pass<ObsState, true>(sh, B0, B1, O0, O1, wt, Bobs, wm, part, state, which, p);
}

// one block: the fold and tree over the partials of obs_omega_k, then thread 0 forms L and decides
__global__ __launch_bounds__(kRedBlock) void obs_final_k(const double *__restrict__ part, int nb,
                                                        double *__restrict__ state, int which, double nu,
                                                        double dt_min) {
  __shared__ double sh[kObsSums][kRedBlock];
  if (state[ObsState::STOP] != 0.0) return;
  ndsm::block_final<kObsSums, kObsSums>(sh, part, nb);
  if (threadIdx.x != 0) return;
  const double lf = sh[0][0], ld = sh[1][0], lm = sh[2][0];
  if (ndsm::descent_decide<ObsState>(state, (lf + ld) + nu * lm, which != 0, dt_min)) {
    state[ObsState::TERM] = lf;
    state[ObsState::TERM + 1] = ld;
    state[ObsState::TERM + 2] = lm;
  }
}

// T = B + dt F~ inside, T = B + dt H on the freed nodes of the k = 0 plane, T = B on its rim and on the five other
// faces; B, Omega: the current buffers, T: the other B buffer
__global__ __launch_bounds__(256) void obs_force_k(double *__restrict__ B0, double *__restrict__ B1,
                                                   const double *__restrict__ O0, const double *__restrict__ O1,
                                                   const double *__restrict__ wt, const double *__restrict__ Bobs,
                                                   const double *__restrict__ wm, const double *__restrict__ state,
                                                   OptArgs p, double nu, int free) {
  ndsm::force_pass<ObsState, true>(B0, B1, O0, O1, wt, Bobs, wm, state, p, nu, free);
}

int obs_args(const int32_t *n3, const double *h_dq3, double nu, int free, OptArgs &p) {
  if (int rc = ndsm::opt_args(n3, h_dq3, p)) return rc;
  NDSM_CHECK_ARG((free == 0 || free == 1) && nu >= 0.0);
  return 0;
}

int obs_evaluate(double *B0, double *B1, double *O, const double *w, const double *Bobs, const double *wm,
                 double *work, const OptArgs &p, double nu, int which, double dt_min) {
  const size_t N3 = 3 * (size_t)p.n[0] * (size_t)p.n[1] * (size_t)p.n[2];
  const int nb = ndsm::red_blocks(p.nrows);
  double *state = work, *part = work + ObsState::LEN;
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(obs_omega_k, dim3(nb), dim3(kRedBlock), 0, s, B0, B1, O, O + N3, w, Bobs, wm, part, state, which,
                     p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(obs_final_k, dim3(1), dim3(kRedBlock), 0, s, part, nb, state, which, nu, dt_min);
  NDSM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" size_t ndsmk_optimize_obs_work_bytes(void) { return ndsm::descent_work_bytes<ObsState, kObsSums>(); }

// The start: the state (tries 0, dt0, buffer 0 current), then Omega and L of B0.  Asynchronous.
extern "C" int ndsmk_optimize_obs_begin(double *B0, double *B1, double *O, const double *w, const double *Bobs,
                                        const double *wm, double *work, const int32_t *n3, const double *h_dq3,
                                        double nu, double dt0, double dt_min) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B0 && B1 && O && Bobs && work);
  OptArgs p;
  if (int rc = obs_args(n3, h_dq3, nu, 0, p)) return rc;
  if (int rc = ndsm::descent_begin<ObsState>(work, dt0)) return rc;
  return obs_evaluate(B0, B1, O, w, Bobs, wm, work, p, nu, 0, dt_min);
}

// ntries tries, each the force-and-update pass, the Omega pass of the trial field and the decision.  Asynchronous:
// nothing is read back.
extern "C" int ndsmk_optimize_obs_tries(double *B0, double *B1, double *O, const double *w, const double *Bobs,
                                        const double *wm, double *work, const int32_t *n3, const double *h_dq3,
                                        double nu, int free, double dt_min, int ntries) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B0 && B1 && O && Bobs && work && ntries >= 0);
  OptArgs p;
  if (int rc = obs_args(n3, h_dq3, nu, free, p)) return rc;
  const size_t N3 = 3 * (size_t)n3[0] * (size_t)n3[1] * (size_t)n3[2];
  dim3 grid, block;
  ndsm::force_shape(p, grid, block);
  for (int it = 0; it < ntries; ++it) {
    hipLaunchKernelGGL(obs_force_k, grid, block, 0, ndsm::stream(), B0, B1, O, O + N3, w, Bobs, wm, work, p, nu, free);
    NDSM_LAUNCH_CHECK();
    if (int rc = obs_evaluate(B0, B1, O, w, Bobs, wm, work, p, nu, 1, dt_min)) return rc;
  }
  return 0;
}

// Blocking.  h_row9 (host) = [tries, L, L_f, L_d, L_m, dt, accepted, current buffer (0: B0, 1: B1), stop flag]
extern "C" int ndsmk_optimize_obs_row(const double *work, double *h_row9) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(work && h_row9);
  return ndsm::descent_row<ObsState>(work, h_row9);
}
