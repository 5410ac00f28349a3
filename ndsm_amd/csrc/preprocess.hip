// Magnetogram preprocessing on the device (DESIGN.md "Magnetogram preprocessing"; Wiegelmann, Inhester & Sakurai
// 2006): a vector magnetogram B (nx,ny,3) on the lower face is moved, within the measurement error, towards one whose
// net Maxwell force and torque vanish and which is smooth.  One try of the descent is three launches:
//
//   pre_update_k : reads B, Lambda (the 5-point Laplacian of B) of the CURRENT buffers, the observation and the sums
//                  S1 .. S6 of the current field from the state; writes the TRIAL field T = B - dt (E / hh) G at every
//                  node, G the exact gradient of L.  Streaming, one thread per node: 72 B/pt in, 24 out.
//   pre_sums_k   : reads the trial (at the start: the current, or the observed) field, writes its Lambda and the block
//                  partials of the eleven sums with opt_omega_k's row walk and descent.hpp's tree: 48 B/pt in, 24 out.
//   pre_final_k  : one block: descent.hpp's fold and tree over the partials, then ONE thread forms L1 .. L4 and L and
//                  runs descent.hpp's decision: L_T < L accepts (the buffer index flips, dt grows by 1.01), anything
//                  else - a NaN included - rejects (dt halves).  The sums of the accepted field stay in the state for
//                  the next update pass.  The pass over the observation (PRE_OBS) only stores its two norms.
//
// Which of the two B and the two Lambda buffers is "current" is a number in the device-resident state (descent.hpp's
// DescentState: five terms, eight sums in the row, two norms behind the control words), and so are dt,
// L, the sums and the counters: the host reads nothing back between two checks.  A dt below dt_min raises the state's
// stop flag; the launches already queued behind it return at once.  Every step is deterministic and the library is
// built without contraction: tests/preprocess_model.py restates the iteration in numpy bit for bit.
#include "descent.hpp"
#include "diffq.hpp"

namespace {

using ndsm::kRedBlock;
using ndsm::trap_w;

constexpr int kPreSums = 11;          // S1 .. S11

// the device-resident state: the history row [tries, L, L1, L2, L3h, L3z, L4, dt, accepted, S1 .. S6, S10, S11], the
// control words, then the norms E and M of the observation
using PreState = ndsm::DescentState<5, 8, 2>;
enum {
  ST_L1 = PreState::TERM, ST_L2, ST_L3H, ST_L3Z, ST_L4,
  ST_S1 = PreState::EXTRA, ST_S2, ST_S3, ST_S4, ST_S5, ST_S6, ST_S10, ST_S11,
  ST_E = PreState::TAIL, ST_M
};

// which field a sums pass and the decision behind it are about
enum { PRE_START = 0, PRE_TRIAL = 1, PRE_OBS = 2 };

struct PreArgs {
  int n[2];
  double dq[2];
  double mu[5];   // mu1, mu2, mu3h, mu3z, mu4
};

// node coordinate about the centre of the plane
__device__ __forceinline__ double centred(int q, int n, double h) { return ((double)q - 0.5 * (double)(n - 1)) * h; }

// the 5-point stencil on a component v of the plane at an interior node c
__device__ __forceinline__ double lap5(const double *__restrict__ v, size_t c, size_t sy, double rx, double ry) {
  const double v0 = v[c];
  return ((v[c - 1] + v[c + 1]) - 2.0 * v0) * rx + ((v[c - sy] + v[c + sy]) - 2.0 * v0) * ry;
}

// the same stencil on Lambda at ANY node, Lambda taken as 0 outside the plane (it is stored as 0 on the edge nodes)
__device__ __forceinline__ double lap5t(const double *__restrict__ v, size_t c, int i, int j, int nx, int ny, size_t sy,
                                        double rx, double ry) {
  const double v0 = v[c];
  const double xm = i > 0 ? v[c - 1] : 0.0, xp = i < nx - 1 ? v[c + 1] : 0.0;
  const double ym = j > 0 ? v[c - sy] : 0.0, yp = j < ny - 1 ? v[c + sy] : 0.0;
  return ((xm + xp) - 2.0 * v0) * rx + ((ym + yp) - 2.0 * v0) * ry;
}

// which = PRE_START: Lambda and the sums of the current field; PRE_TRIAL: of the trial field; PRE_OBS: the sums of the
// observation (its Lambda goes to the trial buffer's place, which the first try overwrites)
__global__ __launch_bounds__(kRedBlock) void pre_sums_k(const double *__restrict__ B0, const double *__restrict__ B1,
                                                       double *__restrict__ La0, double *__restrict__ La1,
                                                       const double *__restrict__ obs, double *__restrict__ part,
                                                       const double *__restrict__ state, int which, PreArgs p) {
  __shared__ double sh[kPreSums][kRedBlock];
  if (state[PreState::STOP] != 0.0) return;
  const int cur = (int)state[PreState::CUR];
  const int src = which == PRE_START ? cur : 1 - cur;
  const double *B = which == PRE_OBS ? obs : (src ? B1 : B0);
  double *La = src ? La1 : La0;
  const int t = threadIdx.x;
  const int nx = p.n[0], ny = p.n[1];
  const size_t sy = (size_t)nx, N = (size_t)nx * (size_t)ny;
  const double hx = p.dq[0], hy = p.dq[1];
  const double rx = 1.0 / (hx * hx), ry = 1.0 / (hy * hy);
  const double *Bx = B, *By = B + N, *Bz = B + 2 * N;
  const double *Ox = obs, *Oy = obs + N, *Oz = obs + 2 * N;
  double v[kPreSums];
  for (int q = 0; q < kPreSums; ++q) v[q] = 0.0;
  for (size_t r = blockIdx.x; r < (size_t)ny; r += gridDim.x) {
    const int j = (int)r;
    const double wy = trap_w(j, ny, hy);
    const double y = centred(j, ny, hy);
    for (int i = t; i < nx; i += kRedBlock) {
      const size_t c = (size_t)i + sy * (size_t)j;
      const double w = trap_w(i, nx, hx) * wy;
      const double x = centred(i, nx, hx);
      const double bx = Bx[c], by = By[c], bz = Bz[c];
      const double e = (bz * bz - bx * bx) - by * by;
      const double bb = (bx * bx + by * by) + bz * bz;
      const double dx = bx - Ox[c], dy = by - Oy[c], dz = bz - Oz[c];
      double lx = 0.0, ly = 0.0, lz = 0.0;
      if (i > 0 && i < nx - 1 && j > 0 && j < ny - 1) {
        lx = lap5(Bx, c, sy, rx, ry);
        ly = lap5(By, c, sy, rx, ry);
        lz = lap5(Bz, c, sy, rx, ry);
      }
      La[c] = lx;
      La[c + N] = ly;
      La[c + 2 * N] = lz;
      v[0] = v[0] + w * (bx * bz);
      v[1] = v[1] + w * (by * bz);
      v[2] = v[2] + w * e;
      v[3] = v[3] + w * (x * e);
      v[4] = v[4] + w * (y * e);
      v[5] = v[5] + w * ((y * bx) * bz - (x * by) * bz);
      v[6] = v[6] + w * (dx * dx + dy * dy);
      v[7] = v[7] + w * (dz * dz);
      v[8] = v[8] + ((lx * lx + ly * ly) + lz * lz);
      v[9] = v[9] + w * bb;
      v[10] = v[10] + w * (sqrt(x * x + y * y) * bb);
    }
  }
  ndsm::block_part<kPreSums, kPreSums>(sh, v, part);
}

// one block: the fold and tree over the partials of pre_sums_k, then thread 0 forms L and decides
__global__ __launch_bounds__(kRedBlock) void pre_final_k(const double *__restrict__ part, int nb,
                                                        double *__restrict__ state, int which, double dt_min,
                                                        PreArgs p) {
  __shared__ double sh[kPreSums][kRedBlock];
  if (state[PreState::STOP] != 0.0) return;
  ndsm::block_final<kPreSums, kPreSums>(sh, part, nb);
  if (threadIdx.x != 0) return;
  if (which == PRE_OBS) {   // the norms of the observation, fixed for the call
    state[ST_E] = sh[9][0];
    state[ST_M] = sh[10][0];
    return;
  }
  const double hh = p.dq[0] * p.dq[1];
  const double E = state[ST_E], M = state[ST_M];
  const double s1 = sh[0][0], s2 = sh[1][0], s3 = sh[2][0], s4 = sh[3][0], s5 = sh[4][0], s6 = sh[5][0];
  const double s9 = hh * sh[8][0];
  const double l1 = ((s1 * s1 + s2 * s2) + s3 * s3) / (E * E);
  const double l2 = ((s4 * s4 + s5 * s5) + s6 * s6) / (M * M);
  const double l3h = sh[6][0] / E, l3z = sh[7][0] / E;
  const double l4 = ((hh * hh) * s9) / E;
  const double l = (((p.mu[0] * l1 + p.mu[1] * l2) + p.mu[2] * l3h) + p.mu[3] * l3z) + p.mu[4] * l4;
  if (ndsm::descent_decide<PreState>(state, l, which == PRE_TRIAL, dt_min)) {
    state[ST_L1] = l1;
    state[ST_L2] = l2;
    state[ST_L3H] = l3h;
    state[ST_L3Z] = l3z;
    state[ST_L4] = l4;
    state[ST_S1] = s1;
    state[ST_S2] = s2;
    state[ST_S3] = s3;
    state[ST_S4] = s4;
    state[ST_S5] = s5;
    state[ST_S6] = s6;
    state[ST_S10] = sh[9][0];
    state[ST_S11] = sh[10][0];
  }
}

// T = B - dt (E / hh) G at every node; B, Lambda: the current buffers, T: the other B buffer
__global__ __launch_bounds__(256) void pre_update_k(double *__restrict__ B0, double *__restrict__ B1,
                                                    const double *__restrict__ La0, const double *__restrict__ La1,
                                                    const double *__restrict__ obs, const double *__restrict__ state,
                                                    PreArgs p) {
  if (state[PreState::STOP] != 0.0) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  const int nx = p.n[0], ny = p.n[1];
  if (i >= nx || j >= ny) return;
  const int cur = (int)state[PreState::CUR];
  const double *B = cur ? B1 : B0;
  const double *La = cur ? La1 : La0;
  double *T = cur ? B0 : B1;
  const size_t sy = (size_t)nx, N = (size_t)nx * (size_t)ny;
  const size_t c = (size_t)i + sy * (size_t)j;
  const double hx = p.dq[0], hy = p.dq[1];
  const double hh = hx * hy;
  const double rx = 1.0 / (hx * hx), ry = 1.0 / (hy * hy);
  const double E = state[ST_E], M = state[ST_M];
  const double s1 = state[ST_S1], s2 = state[ST_S2], s3 = state[ST_S3];
  const double s4 = state[ST_S4], s5 = state[ST_S5], s6 = state[ST_S6];
  const double step = state[PreState::DT] * (E / hh);
  const double a = (2.0 * p.mu[0]) / (E * E), b = (2.0 * p.mu[1]) / (M * M);
  const double c3h = (2.0 * p.mu[2]) / E, c3z = (2.0 * p.mu[3]) / E;
  const double c4 = ((2.0 * p.mu[4]) * ((hh * hh) * hh)) / E;
  const double w = trap_w(i, nx, hx) * trap_w(j, ny, hy);
  const double x = centred(i, nx, hx), y = centred(j, ny, hy);
  const double bx = B[c], by = B[c + N], bz = B[c + 2 * N];
  const double dx = bx - obs[c], dy = by - obs[c + N], dz = bz - obs[c + 2 * N];
  const double tx = lap5t(La, c, i, j, nx, ny, sy, rx, ry);
  const double ty = lap5t(La + N, c, i, j, nx, ny, sy, rx, ry);
  const double tz = lap5t(La + 2 * N, c, i, j, nx, ny, sy, rx, ry);
  const double f1x = s1 * bz - (2.0 * s3) * bx;
  const double f1y = s2 * bz - (2.0 * s3) * by;
  const double f1z = (s1 * bx + s2 * by) + (2.0 * s3) * bz;
  const double f2x = ((((-2.0) * s4) * x) * bx - ((2.0 * s5) * y) * bx) + (s6 * y) * bz;
  const double f2y = ((((-2.0) * s4) * x) * by - ((2.0 * s5) * y) * by) - (s6 * x) * bz;
  const double f2z = (((2.0 * s4) * x) * bz + ((2.0 * s5) * y) * bz) + s6 * (y * bx - x * by);
  const double gx = w * ((a * f1x + b * f2x) + c3h * dx) + c4 * tx;
  const double gy = w * ((a * f1y + b * f2y) + c3h * dy) + c4 * ty;
  const double gz = w * ((a * f1z + b * f2z) + c3z * dz) + c4 * tz;
  T[c] = bx - step * gx;
  T[c + N] = by - step * gy;
  T[c + 2 * N] = bz - step * gz;
}

int pre_args(const int32_t *n2, const double *h_dq2, const double *h_mu5, PreArgs &p) {
  NDSM_CHECK_ARG(n2 && h_dq2 && h_mu5);
  NDSM_CHECK_ARG(n2[0] >= 3 && n2[1] >= 3 && (n2[1] + 3) / 4 <= 65535);
  for (int d = 0; d < 2; ++d) {
    p.n[d] = n2[d];
    p.dq[d] = h_dq2[d];
  }
  for (int q = 0; q < 5; ++q) p.mu[q] = h_mu5[q];
  return 0;
}

int pre_evaluate(double *B0, double *B1, double *La, const double *obs, double *work, const PreArgs &p, int which,
                 double dt_min) {
  const size_t N3 = 3 * (size_t)p.n[0] * (size_t)p.n[1];
  const int nb = ndsm::red_blocks((size_t)p.n[1]);
  double *state = work, *part = work + PreState::LEN;
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(pre_sums_k, dim3(nb), dim3(kRedBlock), 0, s, B0, B1, La, La + N3, obs, part, state, which, p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(pre_final_k, dim3(1), dim3(kRedBlock), 0, s, part, nb, state, which, dt_min, p);
  NDSM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" size_t ndsmk_preprocess_work_bytes(void) { return ndsm::descent_work_bytes<PreState, kPreSums>(); }

// The start: the state (tries 0, dt0, buffer 0 current), E and M of the observation, then Lambda, the sums and L of
// B0.  Asynchronous.
extern "C" int ndsmk_preprocess_begin(double *B0, double *B1, double *La, const double *obs, double *work,
                                      const int32_t *n2, const double *h_dq2, const double *h_mu5, double dt0,
                                      double dt_min) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B0 && B1 && La && obs && work);
  PreArgs p;
  if (int rc = pre_args(n2, h_dq2, h_mu5, p)) return rc;
  if (int rc = ndsm::descent_begin<PreState>(work, dt0)) return rc;
  if (int rc = pre_evaluate(B0, B1, La, obs, work, p, PRE_OBS, dt_min)) return rc;
  return pre_evaluate(B0, B1, La, obs, work, p, PRE_START, dt_min);
}

// ntries tries, each the update pass, the sums pass of the trial field and the decision.  Asynchronous: nothing is
// read back.
extern "C" int ndsmk_preprocess_tries(double *B0, double *B1, double *La, const double *obs, double *work,
                                      const int32_t *n2, const double *h_dq2, const double *h_mu5, double dt_min,
                                      int ntries) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B0 && B1 && La && obs && work && ntries >= 0);
  PreArgs p;
  if (int rc = pre_args(n2, h_dq2, h_mu5, p)) return rc;
  const size_t N3 = 3 * (size_t)n2[0] * (size_t)n2[1];
  dim3 block(64, 4, 1);
  dim3 grid((n2[0] + 63) / 64, (n2[1] + 3) / 4, 1);
  for (int it = 0; it < ntries; ++it) {
    hipLaunchKernelGGL(pre_update_k, grid, block, 0, ndsm::stream(), B0, B1, La, La + N3, obs, work, p);
    NDSM_LAUNCH_CHECK();
    if (int rc = pre_evaluate(B0, B1, La, obs, work, p, PRE_TRIAL, dt_min)) return rc;
  }
  return 0;
}

// Blocking.  h_row21 (host) = the history row [tries, L, L1, L2, L3h, L3z, L4, dt, accepted, S1 .. S6, S10, S11], then
// [current buffer (0: B0, 1: B1), stop flag (dt < dt_min), E, M]
extern "C" int ndsmk_preprocess_row(const double *work, double *h_row21) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(work && h_row21);
  return ndsm::descent_row<PreState>(work, h_row21);
}
