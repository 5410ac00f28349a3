// The optimization method with a measurement term and a freed lower face (DESIGN.md "Measurement errors and a freed
// lower face"; Wiegelmann & Inhester 2010, Wiegelmann et al. 2012): optimize.hip's three launches per try with
//
//   obs_force_k : the k = 0 plane is a branch (k is blockIdx.z: uniform per block).  Its rim is copied; with free = 1
//                 its other nodes get T = B + dt H,  H = (F~ + c G) - c (nu (wm (B - Bobs))),  c = 2 / h_z:  F~ with
//                 ddq's rows as they are at the face node (centred in x and y, three-point one-sided in z: P and s at
//                 k = 1, 2 recomputed from Omega and B), G = w (-P_y, P_x, -s) the surface term of the variation.
//                 Every other node is optimize.hip's: T = B + dt F~ inside, T = B on the five other faces.
//   obs_omega_k : a third sum through the same row walk and tree: the threads of the rows with k = 0 add
//                 W2 ((wm_x dx dx + wm_y dy dy) + wm_z dz dz), d = B - Bobs, W2 = w_x w_y; the others add nothing.
//   obs_final_k : L = (L_f + L_d) + nu L_m, formed by the deciding thread; the decision is optimize.hip's.
//
// The state is one history row (7 doubles) plus the buffer index and the stop flag.  No atomics; every step is
// deterministic and the library is built without contraction: tests/optimize_obs_model.py restates the iteration in
// numpy bit for bit.
#include "common.hpp"
#include "diffq.hpp"
#include "optimize_ps.hpp"

namespace {

using ndsm::dcen;
using ndsm::ddq;
using ndsm::dlow;
using ndsm::PS;
using ndsm::ps_at;
using ndsm::trap_w;

constexpr int kObsBlock = 256;        // kOptBlock of optimize.hip
constexpr int kObsMaxBlocks = 2048;   // kOptMaxBlocks
constexpr int kObsSums = 3;           // L_f, L_d, L_m

enum {
  ST_TRIES = 0, ST_L = 1, ST_LF = 2, ST_LD = 3, ST_LM = 4, ST_DT = 5, ST_ACCEPTED = 6, ST_CUR = 7, ST_STOP = 8,
  ST_LEN = 9
};

struct ObsArgs {
  int n[3];
  double dq[3];
  size_t nrows;   // ny * nz
  double nu;
  int free;
};

// which = 0: Omega and the sums of the current field (the start); which = 1: of the trial field
__global__ __launch_bounds__(kObsBlock) void obs_omega_k(const double *__restrict__ B0, const double *__restrict__ B1,
                                                        double *__restrict__ O0, double *__restrict__ O1,
                                                        const double *__restrict__ wt, const double *__restrict__ Bobs,
                                                        const double *__restrict__ wm, double *__restrict__ part,
                                                        const double *__restrict__ state, int which, ObsArgs p) {
  __shared__ double sh[kObsSums][kObsBlock];
  if (state[ST_STOP] != 0.0) return;
  const int cur = (int)state[ST_CUR];
  const int src = which ? 1 - cur : cur;
  const double *B = src ? B1 : B0;
  double *O = src ? O1 : O0;
  const int t = threadIdx.x;
  const int nx = p.n[0], ny = p.n[1], nz = p.n[2];
  const size_t sy = (size_t)nx, sz = (size_t)nx * ny, N = sz * (size_t)nz;
  const double *Bx = B, *By = B + N, *Bz = B + 2 * N;
  double v[kObsSums];
  for (int q = 0; q < kObsSums; ++q) v[q] = 0.0;
  for (size_t r = blockIdx.x; r < p.nrows; r += gridDim.x) {
    const int j = (int)(r % (size_t)ny), k = (int)(r / (size_t)ny);
    const double wy = trap_w(j, ny, p.dq[1]);
    const double wyz = wy * trap_w(k, nz, p.dq[2]);
    for (int i = t; i < nx; i += kObsBlock) {
      const size_t c = (size_t)i + sy * (size_t)j + sz * (size_t)k;
      const double wx = trap_w(i, nx, p.dq[0]);
      double w = wx * wyz;
      if (wt) w = w * wt[c];
      const double bx = Bx[c], by = By[c], bz = Bz[c];
      const double bb = (bx * bx + by * by) + bz * bz;
      // curl_k's expressions (post.hip)
      const double jx = ddq(Bz, c, j, ny, sy, p.dq[1]) - ddq(By, c, k, nz, sz, p.dq[2]);
      const double jy = ddq(Bx, c, k, nz, sz, p.dq[2]) - ddq(Bz, c, i, nx, 1, p.dq[0]);
      const double jz = ddq(By, c, i, nx, 1, p.dq[0]) - ddq(Bx, c, j, ny, sy, p.dq[1]);
      const double dv = ddq(Bx, c, i, nx, 1, p.dq[0]) + ddq(By, c, j, ny, sy, p.dq[1]) + ddq(Bz, c, k, nz, sz, p.dq[2]);
      double ox = 0.0, oy = 0.0, oz = 0.0;
      if (bb > 0.0) {
        const double cx = jy * bz - jz * by, cy = jz * bx - jx * bz, cz = jx * by - jy * bx;
        ox = (cx - dv * bx) / bb;
        oy = (cy - dv * by) / bb;
        oz = (cz - dv * bz) / bb;
        v[0] = v[0] + w * (((cx * cx + cy * cy) + cz * cz) / bb);
        v[1] = v[1] + w * (dv * dv);
      }
      O[c] = ox;
      O[c + N] = oy;
      O[c + 2 * N] = oz;
      if (k == 0) {   // the measurement term: c is the node's index in the (nx,ny,3) planes too
        const double dx = bx - Bobs[c], dy = by - Bobs[c + sz], dz = bz - Bobs[c + 2 * sz];
        double m;
        if (wm)
          m = (wm[c] * (dx * dx) + wm[c + sz] * (dy * dy)) + wm[c + 2 * sz] * (dz * dz);
        else
          m = (dx * dx + dy * dy) + dz * dz;
        v[2] = v[2] + (wx * wy) * m;
      }
    }
  }
  for (int q = 0; q < kObsSums; ++q) sh[q][t] = v[q];
  __syncthreads();
  for (int o = kObsBlock / 2; o > 0; o >>= 1) {
    if (t < o)
      for (int q = 0; q < kObsSums; ++q) sh[q][t] = sh[q][t] + sh[q][t + o];
    __syncthreads();
  }
  if (t < kObsSums) part[(size_t)blockIdx.x * kObsSums + t] = sh[t][0];
}

// one block: the fold and tree over the partials of obs_omega_k, then thread 0 forms L and decides
__global__ __launch_bounds__(kObsBlock) void obs_final_k(const double *__restrict__ part, int nb,
                                                        double *__restrict__ state, int which, double nu,
                                                        double dt_min) {
  __shared__ double sh[kObsSums][kObsBlock];
  if (state[ST_STOP] != 0.0) return;
  const int t = threadIdx.x;
  double v[kObsSums];
  for (int q = 0; q < kObsSums; ++q) v[q] = 0.0;
  for (int b = t; b < nb; b += kObsBlock)
    for (int q = 0; q < kObsSums; ++q) v[q] = v[q] + part[(size_t)b * kObsSums + q];
  for (int q = 0; q < kObsSums; ++q) sh[q][t] = v[q];
  __syncthreads();
  for (int o = kObsBlock / 2; o > 0; o >>= 1) {
    if (t < o)
      for (int q = 0; q < kObsSums; ++q) sh[q][t] = sh[q][t] + sh[q][t + o];
    __syncthreads();
  }
  if (t != 0) return;
  const double lf = sh[0][0], ld = sh[1][0], lm = sh[2][0];
  const double l = (lf + ld) + nu * lm;
  double dt = state[ST_DT];
  if (which == 0) {
    state[ST_L] = l;
    state[ST_LF] = lf;
    state[ST_LD] = ld;
    state[ST_LM] = lm;
  } else {
    state[ST_TRIES] = state[ST_TRIES] + 1.0;
    if (l < state[ST_L]) {   // (false for a NaN on either side: a rejection)
      state[ST_L] = l;
      state[ST_LF] = lf;
      state[ST_LD] = ld;
      state[ST_LM] = lm;
      state[ST_CUR] = 1.0 - state[ST_CUR];
      state[ST_ACCEPTED] = state[ST_ACCEPTED] + 1.0;
      dt = dt * 1.01;
    } else {
      dt = dt * 0.5;
    }
    state[ST_DT] = dt;
  }
  if (dt < dt_min) state[ST_STOP] = 1.0;
}

// F~ of optimize.hip's opt_force_k at node c.  kLow = false: an interior node.  kLow = true: a node of the k = 0 plane
// off its rim - ddq takes its one-sided row in z by itself, P and s come from the planes k = 0, 1, 2.
template <bool kLow>
__device__ __forceinline__ void ftilde(const double *__restrict__ B, const double *__restrict__ O,
                                       const double *__restrict__ wt, size_t c, int i, int j, int k, const ObsArgs &p,
                                       const PS &here, double &fx, double &fy, double &fz) {
  const int nx = p.n[0], ny = p.n[1], nz = p.n[2];
  const size_t sy = (size_t)nx, sz = (size_t)nx * ny, N = sz * (size_t)nz;
  const double hx = p.dq[0], hy = p.dq[1], hz = p.dq[2];
  const double *Bx = B, *By = B + N, *Bz = B + 2 * N;
  const double bx = Bx[c], by = By[c], bz = Bz[c];
  const double jx = ddq(Bz, c, j, ny, sy, hy) - ddq(By, c, k, nz, sz, hz);
  const double jy = ddq(Bx, c, k, nz, sz, hz) - ddq(Bz, c, i, nx, 1, hx);
  const double jz = ddq(By, c, i, nx, 1, hx) - ddq(Bx, c, j, ny, sy, hy);
  const double dv = ddq(Bx, c, i, nx, 1, hx) + ddq(By, c, j, ny, sy, hy) + ddq(Bz, c, k, nz, sz, hz);
  const double ox = O[c], oy = O[c + N], oz = O[c + 2 * N];
  const PS xm = ps_at(B, O, c - 1, N), xp = ps_at(B, O, c + 1, N);
  const PS ym = ps_at(B, O, c - sy, N), yp = ps_at(B, O, c + sy, N);
  double dzpx, dzpy, gsz;
  if (kLow) {
    const PS z1 = ps_at(B, O, c + sz, N), z2 = ps_at(B, O, c + 2 * sz, N);
    dzpx = dlow(here.px, z1.px, z2.px, hz);
    dzpy = dlow(here.py, z1.py, z2.py, hz);
    gsz = dlow(here.s, z1.s, z2.s, hz);
  } else {
    const PS zm = ps_at(B, O, c - sz, N), zp = ps_at(B, O, c + sz, N);
    dzpx = dcen(zm.px, zp.px, hz);
    dzpy = dcen(zm.py, zp.py, hz);
    gsz = dcen(zm.s, zp.s, hz);
  }
  // curl_h P in curl_k's expressions, grad_h s
  const double cpx = dcen(ym.pz, yp.pz, hy) - dzpy;
  const double cpy = dzpx - dcen(xm.pz, xp.pz, hx);
  const double cpz = dcen(xm.py, xp.py, hx) - dcen(ym.px, yp.px, hy);
  const double gsx = dcen(xm.s, xp.s, hx), gsy = dcen(ym.s, yp.s, hy);
  // Omega x J, |Omega|^2
  const double qx = oy * jz - oz * jy, qy = oz * jx - ox * jz, qz = ox * jy - oy * jx;
  const double oo = (ox * ox + oy * oy) + oz * oz;
  fx = (((cpx - qx) - gsx) + ox * dv) + oo * bx;
  fy = (((cpy - qy) - gsy) + oy * dv) + oo * by;
  fz = (((cpz - qz) - gsz) + oz * dv) + oo * bz;
  if (wt) {
    const double w = wt[c];
    const double gwx = ddq(wt, c, i, nx, 1, hx), gwy = ddq(wt, c, j, ny, sy, hy), gwz = ddq(wt, c, k, nz, sz, hz);
    fx = (w * fx - (here.py * gwz - here.pz * gwy)) - here.s * gwx;
    fy = (w * fy - (here.pz * gwx - here.px * gwz)) - here.s * gwy;
    fz = (w * fz - (here.px * gwy - here.py * gwx)) - here.s * gwz;
  }
}

// T = B + dt F~ inside, T = B + dt H on the freed nodes of the k = 0 plane, T = B on its rim and on the five other
// faces; B, Omega: the current buffers, T: the other B buffer
__global__ __launch_bounds__(256) void obs_force_k(double *__restrict__ B0, double *__restrict__ B1,
                                                   const double *__restrict__ O0, const double *__restrict__ O1,
                                                   const double *__restrict__ wt, const double *__restrict__ Bobs,
                                                   const double *__restrict__ wm, const double *__restrict__ state,
                                                   ObsArgs p) {
  if (state[ST_STOP] != 0.0) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  const int k = blockIdx.z;
  const int nx = p.n[0], ny = p.n[1], nz = p.n[2];
  if (i >= nx || j >= ny) return;
  const int cur = (int)state[ST_CUR];
  const double dt = state[ST_DT];
  const double *B = cur ? B1 : B0;
  const double *O = cur ? O1 : O0;
  double *T = cur ? B0 : B1;
  const size_t sy = (size_t)nx, sz = (size_t)nx * ny, N = sz * (size_t)nz;
  const size_t c = (size_t)i + sy * (size_t)j + sz * (size_t)k;
  const double bx = B[c], by = B[c + N], bz = B[c + 2 * N];
  const bool rim = i == 0 || i == nx - 1 || j == 0 || j == ny - 1;
  if (rim || k == nz - 1 || (k == 0 && !p.free)) {
    T[c] = bx;
    T[c + N] = by;
    T[c + 2 * N] = bz;
    return;
  }
  const PS here = ps_at(B, O, c, N);
  double fx, fy, fz;
  if (k == 0) {   // (uniform per block)
    ftilde<true>(B, O, wt, c, i, j, k, p, here, fx, fy, fz);
    const double c2 = 2.0 / p.dq[2];
    double gx = -here.py, gy = here.px, gz = -here.s;
    if (wt) {
      const double w = wt[c];
      gx = w * gx;
      gy = w * gy;
      gz = w * gz;
    }
    double mx = bx - Bobs[c], my = by - Bobs[c + sz], mz = bz - Bobs[c + 2 * sz];
    if (wm) {
      mx = wm[c] * mx;
      my = wm[c + sz] * my;
      mz = wm[c + 2 * sz] * mz;
    }
    fx = (fx + c2 * gx) - c2 * (p.nu * mx);
    fy = (fy + c2 * gy) - c2 * (p.nu * my);
    fz = (fz + c2 * gz) - c2 * (p.nu * mz);
  } else {
    ftilde<false>(B, O, wt, c, i, j, k, p, here, fx, fy, fz);
  }
  T[c] = bx + dt * fx;
  T[c + N] = by + dt * fy;
  T[c + 2 * N] = bz + dt * fz;
}

__global__ void obs_state_k(double *__restrict__ state, double dt0) {
  if (threadIdx.x < ST_LEN) state[threadIdx.x] = threadIdx.x == ST_DT ? dt0 : 0.0;
}

int obs_args(const int32_t *n3, const double *h_dq3, double nu, int free, ObsArgs &p) {
  NDSM_CHECK_ARG(n3[0] >= 3 && n3[1] >= 3 && n3[2] >= 3 && n3[2] <= 65535 && (n3[1] + 3) / 4 <= 65535);
  NDSM_CHECK_ARG((free == 0 || free == 1) && nu >= 0.0);
  for (int d = 0; d < 3; ++d) {
    p.n[d] = n3[d];
    p.dq[d] = h_dq3[d];
  }
  p.nrows = (size_t)n3[1] * (size_t)n3[2];
  p.nu = nu;
  p.free = free;
  return 0;
}

int obs_evaluate(double *B0, double *B1, double *O, const double *w, const double *Bobs, const double *wm,
                 double *work, const ObsArgs &p, int which, double dt_min) {
  const size_t N3 = 3 * (size_t)p.n[0] * (size_t)p.n[1] * (size_t)p.n[2];
  const int nb = (int)(p.nrows < (size_t)kObsMaxBlocks ? p.nrows : (size_t)kObsMaxBlocks);
  double *state = work, *part = work + ST_LEN;
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(obs_omega_k, dim3(nb), dim3(kObsBlock), 0, s, B0, B1, O, O + N3, w, Bobs, wm, part, state, which,
                     p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(obs_final_k, dim3(1), dim3(kObsBlock), 0, s, part, nb, state, which, p.nu, dt_min);
  NDSM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" size_t ndsmk_optimize_obs_work_bytes(void) {
  return sizeof(double) * (ST_LEN + (size_t)kObsMaxBlocks * kObsSums);
}

// The start: the state (tries 0, dt0, buffer 0 current), then Omega and L of B0.  Asynchronous.
extern "C" int ndsmk_optimize_obs_begin(double *B0, double *B1, double *O, const double *w, const double *Bobs,
                                        const double *wm, double *work, const int32_t *n3, const double *h_dq3,
                                        double nu, double dt0, double dt_min) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B0 && B1 && O && Bobs && work);
  ObsArgs p;
  if (int rc = obs_args(n3, h_dq3, nu, 0, p)) return rc;
  hipLaunchKernelGGL(obs_state_k, dim3(1), dim3(64), 0, ndsm::stream(), work, dt0);
  NDSM_LAUNCH_CHECK();
  return obs_evaluate(B0, B1, O, w, Bobs, wm, work, p, 0, dt_min);
}

// ntries tries, each the force-and-update pass, the Omega pass of the trial field and the decision.  Asynchronous:
// nothing is read back.
extern "C" int ndsmk_optimize_obs_tries(double *B0, double *B1, double *O, const double *w, const double *Bobs,
                                        const double *wm, double *work, const int32_t *n3, const double *h_dq3,
                                        double nu, int free, double dt_min, int ntries) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B0 && B1 && O && Bobs && work && ntries >= 0);
  ObsArgs p;
  if (int rc = obs_args(n3, h_dq3, nu, free, p)) return rc;
  const size_t N3 = 3 * (size_t)n3[0] * (size_t)n3[1] * (size_t)n3[2];
  dim3 block(64, 4, 1);
  dim3 grid((n3[0] + 63) / 64, (n3[1] + 3) / 4, n3[2]);
  for (int it = 0; it < ntries; ++it) {
    hipLaunchKernelGGL(obs_force_k, grid, block, 0, ndsm::stream(), B0, B1, O, O + N3, w, Bobs, wm, work, p);
    NDSM_LAUNCH_CHECK();
    if (int rc = obs_evaluate(B0, B1, O, w, Bobs, wm, work, p, 1, dt_min)) return rc;
  }
  return 0;
}

// Blocking.  h_row9 (host) = [tries, L, L_f, L_d, L_m, dt, accepted, current buffer (0: B0, 1: B1), stop flag]
extern "C" int ndsmk_optimize_obs_row(const double *work, double *h_row9) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(work && h_row9);
  hipStream_t s = ndsm::stream();
  NDSM_HIP(hipMemcpyAsync(h_row9, work, ST_LEN * sizeof(double), hipMemcpyDeviceToHost, s));
  NDSM_HIP(hipStreamSynchronize(s));
  return 0;
}
