// The optimization-method force-free solver on the device (DESIGN.md "Optimization-method force-free field";
// Wheatland, Sturrock & Roumeliotis 2000; Wiegelmann 2004).  One try of the iteration is three launches:
//
//   opt_force_k : reads B, Omega and w of the CURRENT buffers, writes the TRIAL field T = B + dt F~ on the interior
//                 nodes and T = B on the six faces.  P = Omega x B and s = Omega.B at the six neighbours are recomputed
//                 from Omega and B (pointwise products: the bits a stored P, s would have).  Streaming, one thread per
//                 node: 56 B/pt in (B, Omega, w), 24 out.
//   opt_omega_k : reads the trial (or, at the start, the current) field, writes its Omega and the block partials of
//                 L_f = sum W w |J x B|^2 / |B|^2 and L_d = sum W w (div_h B)^2 with nlfff_part_k's row walk and
//                 256-wide tree (field.hip): 24 B/pt in (+ 8 of w), 24 out.
//   opt_final_k : one block: nlfff_final_k's fold and tree over the partials, then ONE thread decides: L_T < L accepts
//                 (the buffer index flips, dt grows by 1.01), anything else - a NaN included - rejects (dt halves).
//
// Which of the two B and the two Omega buffers is "current" is a number in the device-resident state, and so are dt,
// L and the counters: the kernels of the next try read them from there, and the host reads nothing back between two
// checks.  A dt below dt_min raises the state's stop flag; the launches already queued behind it return at once.
// Every step is deterministic and the library is built without contraction: tests/optimize_model.py restates the
// iteration in numpy bit for bit.
#include "common.hpp"
#include "diffq.hpp"
#include "optimize_ps.hpp"

namespace {

using ndsm::dcen;
using ndsm::ddq;
using ndsm::PS;
using ndsm::ps_at;
using ndsm::trap_w;

constexpr int kOptBlock = 256;        // kHelBlock of field.hip
constexpr int kOptMaxBlocks = 2048;   // kHelMaxBlocks
constexpr int kOptSums = 2;           // L_f, L_d

// the device-resident state, all doubles so that it is one history row plus two control words
enum { ST_TRIES = 0, ST_L = 1, ST_LF = 2, ST_LD = 3, ST_DT = 4, ST_ACCEPTED = 5, ST_CUR = 6, ST_STOP = 7, ST_LEN = 8 };

struct OptArgs {
  int n[3];
  double dq[3];
  size_t nrows;   // ny * nz
};

// which = 0: Omega and the sums of the current field (the start); which = 1: of the trial field
__global__ __launch_bounds__(kOptBlock) void opt_omega_k(const double *__restrict__ B0, const double *__restrict__ B1,
                                                        double *__restrict__ O0, double *__restrict__ O1,
                                                        const double *__restrict__ wt, double *__restrict__ part,
                                                        const double *__restrict__ state, int which, OptArgs p) {
  __shared__ double sh[kOptSums][kOptBlock];
  if (state[ST_STOP] != 0.0) return;
  const int cur = (int)state[ST_CUR];
  const int src = which ? 1 - cur : cur;
  const double *B = src ? B1 : B0;
  double *O = src ? O1 : O0;
  const int t = threadIdx.x;
  const int nx = p.n[0], ny = p.n[1], nz = p.n[2];
  const size_t sy = (size_t)nx, sz = (size_t)nx * ny, N = sz * (size_t)nz;
  const double *Bx = B, *By = B + N, *Bz = B + 2 * N;
  double v[kOptSums];
  for (int q = 0; q < kOptSums; ++q) v[q] = 0.0;
  for (size_t r = blockIdx.x; r < p.nrows; r += gridDim.x) {
    const int j = (int)(r % (size_t)ny), k = (int)(r / (size_t)ny);
    const double wyz = trap_w(j, ny, p.dq[1]) * trap_w(k, nz, p.dq[2]);
    for (int i = t; i < nx; i += kOptBlock) {
      const size_t c = (size_t)i + sy * (size_t)j + sz * (size_t)k;
      double w = trap_w(i, nx, p.dq[0]) * wyz;
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
    }
  }
  for (int q = 0; q < kOptSums; ++q) sh[q][t] = v[q];
  __syncthreads();
  for (int o = kOptBlock / 2; o > 0; o >>= 1) {
    if (t < o)
      for (int q = 0; q < kOptSums; ++q) sh[q][t] = sh[q][t] + sh[q][t + o];
    __syncthreads();
  }
  if (t < kOptSums) part[(size_t)blockIdx.x * kOptSums + t] = sh[t][0];
}

// one block: nlfff_final_k's fold and tree over the partials of opt_omega_k, then thread 0 decides
__global__ __launch_bounds__(kOptBlock) void opt_final_k(const double *__restrict__ part, int nb,
                                                        double *__restrict__ state, int which, double dt_min) {
  __shared__ double sh[kOptSums][kOptBlock];
  if (state[ST_STOP] != 0.0) return;
  const int t = threadIdx.x;
  double v[kOptSums];
  for (int q = 0; q < kOptSums; ++q) v[q] = 0.0;
  for (int b = t; b < nb; b += kOptBlock)
    for (int q = 0; q < kOptSums; ++q) v[q] = v[q] + part[(size_t)b * kOptSums + q];
  for (int q = 0; q < kOptSums; ++q) sh[q][t] = v[q];
  __syncthreads();
  for (int o = kOptBlock / 2; o > 0; o >>= 1) {
    if (t < o)
      for (int q = 0; q < kOptSums; ++q) sh[q][t] = sh[q][t] + sh[q][t + o];
    __syncthreads();
  }
  if (t != 0) return;
  const double lf = sh[0][0], ld = sh[1][0];
  const double l = lf + ld;
  double dt = state[ST_DT];
  if (which == 0) {
    state[ST_L] = l;
    state[ST_LF] = lf;
    state[ST_LD] = ld;
  } else {
    state[ST_TRIES] = state[ST_TRIES] + 1.0;
    if (l < state[ST_L]) {   // (false for a NaN on either side: a rejection)
      state[ST_L] = l;
      state[ST_LF] = lf;
      state[ST_LD] = ld;
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

// T = B + dt F~ inside, T = B on the faces; B, Omega: the current buffers, T: the other B buffer
__global__ __launch_bounds__(256) void opt_force_k(double *__restrict__ B0, double *__restrict__ B1,
                                                   const double *__restrict__ O0, const double *__restrict__ O1,
                                                   const double *__restrict__ wt, const double *__restrict__ state,
                                                   OptArgs p) {
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
  if (i == 0 || i == nx - 1 || j == 0 || j == ny - 1 || k == 0 || k == nz - 1) {
    T[c] = bx;
    T[c + N] = by;
    T[c + 2 * N] = bz;
    return;
  }
  const double hx = p.dq[0], hy = p.dq[1], hz = p.dq[2];
  const double *Bx = B, *By = B + N, *Bz = B + 2 * N;
  // J and D as in opt_omega_k (an interior node: ddq's centred rows)
  const double jx = ddq(Bz, c, j, ny, sy, hy) - ddq(By, c, k, nz, sz, hz);
  const double jy = ddq(Bx, c, k, nz, sz, hz) - ddq(Bz, c, i, nx, 1, hx);
  const double jz = ddq(By, c, i, nx, 1, hx) - ddq(Bx, c, j, ny, sy, hy);
  const double dv = ddq(Bx, c, i, nx, 1, hx) + ddq(By, c, j, ny, sy, hy) + ddq(Bz, c, k, nz, sz, hz);
  const double ox = O[c], oy = O[c + N], oz = O[c + 2 * N];
  const PS xm = ps_at(B, O, c - 1, N), xp = ps_at(B, O, c + 1, N);
  const PS ym = ps_at(B, O, c - sy, N), yp = ps_at(B, O, c + sy, N);
  const PS zm = ps_at(B, O, c - sz, N), zp = ps_at(B, O, c + sz, N);
  // curl_h P in curl_k's expressions, grad_h s
  const double cpx = dcen(ym.pz, yp.pz, hy) - dcen(zm.py, zp.py, hz);
  const double cpy = dcen(zm.px, zp.px, hz) - dcen(xm.pz, xp.pz, hx);
  const double cpz = dcen(xm.py, xp.py, hx) - dcen(ym.px, yp.px, hy);
  const double gsx = dcen(xm.s, xp.s, hx), gsy = dcen(ym.s, yp.s, hy), gsz = dcen(zm.s, zp.s, hz);
  // Omega x J, |Omega|^2
  const double qx = oy * jz - oz * jy, qy = oz * jx - ox * jz, qz = ox * jy - oy * jx;
  const double oo = (ox * ox + oy * oy) + oz * oz;
  double fx = (((cpx - qx) - gsx) + ox * dv) + oo * bx;
  double fy = (((cpy - qy) - gsy) + oy * dv) + oo * by;
  double fz = (((cpz - qz) - gsz) + oz * dv) + oo * bz;
  if (wt) {
    const double w = wt[c];
    const double gwx = ddq(wt, c, i, nx, 1, hx), gwy = ddq(wt, c, j, ny, sy, hy), gwz = ddq(wt, c, k, nz, sz, hz);
    const double px = oy * bz - oz * by, py = oz * bx - ox * bz, pz = ox * by - oy * bx;
    const double s = (ox * bx + oy * by) + oz * bz;
    fx = (w * fx - (py * gwz - pz * gwy)) - s * gwx;
    fy = (w * fy - (pz * gwx - px * gwz)) - s * gwy;
    fz = (w * fz - (px * gwy - py * gwx)) - s * gwz;
  }
  T[c] = bx + dt * fx;
  T[c + N] = by + dt * fy;
  T[c + 2 * N] = bz + dt * fz;
}

__global__ void opt_state_k(double *__restrict__ state, double dt0) {
  if (threadIdx.x < ST_LEN) state[threadIdx.x] = threadIdx.x == ST_DT ? dt0 : 0.0;
}

int opt_args(const int32_t *n3, const double *h_dq3, OptArgs &p) {
  NDSM_CHECK_ARG(n3[0] >= 3 && n3[1] >= 3 && n3[2] >= 3 && n3[2] <= 65535 && (n3[1] + 3) / 4 <= 65535);
  for (int d = 0; d < 3; ++d) {
    p.n[d] = n3[d];
    p.dq[d] = h_dq3[d];
  }
  p.nrows = (size_t)n3[1] * (size_t)n3[2];
  return 0;
}

int opt_evaluate(double *B0, double *B1, double *O, const double *w, double *work, const OptArgs &p, int which,
                 double dt_min) {
  const size_t N3 = 3 * (size_t)p.n[0] * (size_t)p.n[1] * (size_t)p.n[2];
  const int nb = (int)(p.nrows < (size_t)kOptMaxBlocks ? p.nrows : (size_t)kOptMaxBlocks);
  double *state = work, *part = work + ST_LEN;
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(opt_omega_k, dim3(nb), dim3(kOptBlock), 0, s, B0, B1, O, O + N3, w, part, state, which, p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(opt_final_k, dim3(1), dim3(kOptBlock), 0, s, part, nb, state, which, dt_min);
  NDSM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" size_t ndsmk_optimize_work_bytes(void) {
  return sizeof(double) * (ST_LEN + (size_t)kOptMaxBlocks * kOptSums);
}

// The start: the state (tries 0, dt0, buffer 0 current), then Omega and L of B0.  Asynchronous.
extern "C" int ndsmk_optimize_begin(double *B0, double *B1, double *O, const double *w, double *work,
                                    const int32_t *n3, const double *h_dq3, double dt0, double dt_min) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B0 && B1 && O && work);
  OptArgs p;
  if (int rc = opt_args(n3, h_dq3, p)) return rc;
  hipLaunchKernelGGL(opt_state_k, dim3(1), dim3(64), 0, ndsm::stream(), work, dt0);
  NDSM_LAUNCH_CHECK();
  return opt_evaluate(B0, B1, O, w, work, p, 0, dt_min);
}

// ntries tries, each the force-and-update pass, the Omega pass of the trial field and the decision.  Asynchronous:
// nothing is read back.
extern "C" int ndsmk_optimize_tries(double *B0, double *B1, double *O, const double *w, double *work,
                                    const int32_t *n3, const double *h_dq3, double dt_min, int ntries) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B0 && B1 && O && work && ntries >= 0);
  OptArgs p;
  if (int rc = opt_args(n3, h_dq3, p)) return rc;
  const size_t N3 = 3 * (size_t)n3[0] * (size_t)n3[1] * (size_t)n3[2];
  dim3 block(64, 4, 1);
  dim3 grid((n3[0] + 63) / 64, (n3[1] + 3) / 4, n3[2]);
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
  hipStream_t s = ndsm::stream();
  NDSM_HIP(hipMemcpyAsync(h_row8, work, ST_LEN * sizeof(double), hipMemcpyDeviceToHost, s));
  NDSM_HIP(hipStreamSynchronize(s));
  return 0;
}
