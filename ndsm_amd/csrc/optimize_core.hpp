// The two passes of a try of the optimization method, shared by optimize.hip (kObs = false) and optimize_obs.hip
// (kObs = true: a measurement term in L and a freed lower face).  kObs is a compile-time flag: the plain solver's
// kernels carry none of the other's registers or branches.  The reduction, the state and the decision are descent.hpp's.
//
//   omega_pass : reads the trial (or, at the start, the current) field, writes its Omega and the block partials of
//                L_f = sum W w |J x B|^2 / |B|^2 and L_d = sum W w (div_h B)^2; kObs: the threads of the rows with
//                k = 0 add a third sum, W2 ((wm_x dx dx + wm_y dy dy) + wm_z dz dz), d = B - Bobs, W2 = w_x w_y.
//   force_pass : reads B, Omega and w of the CURRENT buffers, writes the TRIAL field T = B + dt F~ on the interior nodes
//                and T = B on the faces.  P = Omega x B and s = Omega.B at the neighbours are recomputed from Omega and
//                B (pointwise products: the bits a stored P, s would have).  kObs with free = 1: the nodes of the k = 0
//                plane off its rim get T = B + dt H,  H = (F~ + c G) - c (nu (wm (B - Bobs))),  c = 2 / h_z:  F~ with
//                ddq's rows as they are at the face node (centred in x and y, three-point one-sided in z: P and s at
//                k = 1, 2), G = w (-P_y, P_x, -s) the surface term of the variation.
#pragma once

#include "descent.hpp"
#include "diffq.hpp"

namespace ndsm {

struct OptArgs {
  int n[3];
  double dq[3];
  size_t nrows;   // ny * nz
};

inline int opt_args(const int32_t *n3, const double *h_dq3, OptArgs &p) {
  NDSM_CHECK_ARG(n3[0] >= 3 && n3[1] >= 3 && n3[2] >= 3 && n3[2] <= 65535 && (n3[1] + 3) / 4 <= 65535);
  for (int d = 0; d < 3; ++d) {
    p.n[d] = n3[d];
    p.dq[d] = h_dq3[d];
  }
  p.nrows = (size_t)n3[1] * (size_t)n3[2];
  return 0;
}

// ddq's centred row on two values that are not in an array
__device__ __forceinline__ double dcen(double vm, double vp, double h) {
  const double half = 0.5;
  double d = 0.0;
  d = d + vm * (-1 * half / h);
  d = d + vp * (+1 * half / h);
  return d;
}

// ddq's one-sided row of the lower end plane on three values that are not in an array
__device__ __forceinline__ double dlow(double v0, double v1, double v2, double h) {
  const double half = 0.5;
  double d = 0.0;
  d = d + v0 * (-3 * half / h);
  d = d + v1 * (+4 * half / h);
  d = d + v2 * (-1 * half / h);
  return d;
}

struct PS {
  double px, py, pz, s;
};

// P = Omega x B and s = Omega.B of one node's values
__device__ __forceinline__ PS ps_of(double bx, double by, double bz, double ox, double oy, double oz) {
  PS r;
  r.px = oy * bz - oz * by;
  r.py = oz * bx - ox * bz;
  r.pz = ox * by - oy * bx;
  r.s = (ox * bx + oy * by) + oz * bz;
  return r;
}

// the same at node c
__device__ __forceinline__ PS ps_at(const double *__restrict__ B, const double *__restrict__ O, size_t c, size_t N) {
  return ps_of(B[c], B[c + N], B[c + 2 * N], O[c], O[c + N], O[c + 2 * N]);
}

// S: the solver's DescentState.  which = 0: Omega and the sums of the current field (the start); which = 1: of the
// trial field.  sh: 2 rows, kObs 3.  Bobs, wm: read with kObs only.
template <class S, bool kObs>
__device__ __forceinline__ void omega_pass(double (*sh)[kRedBlock], const double *__restrict__ B0,
                                           const double *__restrict__ B1, double *__restrict__ O0,
                                           double *__restrict__ O1, const double *__restrict__ wt,
                                           const double *__restrict__ Bobs, const double *__restrict__ wm,
                                           double *__restrict__ part, const double *__restrict__ state, int which,
                                           const OptArgs &p) {
  constexpr int kSums = kObs ? 3 : 2;   // L_f, L_d, (L_m)
  if (state[S::STOP] != 0.0) return;
  const int cur = (int)state[S::CUR];
  const int src = which ? 1 - cur : cur;
  const double *B = src ? B1 : B0;
  double *O = src ? O1 : O0;
  const int t = threadIdx.x;
  const int nx = p.n[0], ny = p.n[1], nz = p.n[2];
  const size_t sy = (size_t)nx, sz = (size_t)nx * ny, N = sz * (size_t)nz;
  const double *Bx = B, *By = B + N, *Bz = B + 2 * N;
  double v[kSums];
  for (int q = 0; q < kSums; ++q) v[q] = 0.0;
  for (size_t r = blockIdx.x; r < p.nrows; r += gridDim.x) {
    const int j = (int)(r % (size_t)ny), k = (int)(r / (size_t)ny);
    const double wy = trap_w(j, ny, p.dq[1]);
    const double wyz = wy * trap_w(k, nz, p.dq[2]);
    for (int i = t; i < nx; i += kRedBlock) {
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
      if (kObs && k == 0) {   // the measurement term: c is the node's index in the (nx,ny,3) planes too
        const double dx = bx - Bobs[c], dy = by - Bobs[c + sz], dz = bz - Bobs[c + 2 * sz];
        double m;
        if (wm)
          m = (wm[c] * (dx * dx) + wm[c + sz] * (dy * dy)) + wm[c + 2 * sz] * (dz * dz);
        else
          m = (dx * dx + dy * dy) + dz * dz;
        v[kSums - 1] = v[kSums - 1] + (wx * wy) * m;
      }
    }
  }
  block_part<kSums, kSums>(sh, v, part);
}

// F~ at node c.  kLow = false: an interior node.  kLow = true: a node of the k = 0 plane off its rim - ddq takes its
// one-sided row in z by itself, P and s come from the planes k = 0, 1, 2.  The node's own P, s are formed only where
// they are used (they would stay live across the whole body otherwise: DESIGN.md "Shared descent machinery").
template <bool kLow>
__device__ __forceinline__ void ftilde(const double *__restrict__ B, const double *__restrict__ O,
                                       const double *__restrict__ wt, size_t c, int i, int j, int k, const OptArgs &p,
                                       double bx, double by, double bz, double &fx, double &fy, double &fz) {
  const int nx = p.n[0], ny = p.n[1], nz = p.n[2];
  const size_t sy = (size_t)nx, sz = (size_t)nx * ny, N = sz * (size_t)nz;
  const double hx = p.dq[0], hy = p.dq[1], hz = p.dq[2];
  const double *Bx = B, *By = B + N, *Bz = B + 2 * N;
  // J and D as in omega_pass
  const double jx = ddq(Bz, c, j, ny, sy, hy) - ddq(By, c, k, nz, sz, hz);
  const double jy = ddq(Bx, c, k, nz, sz, hz) - ddq(Bz, c, i, nx, 1, hx);
  const double jz = ddq(By, c, i, nx, 1, hx) - ddq(Bx, c, j, ny, sy, hy);
  const double dv = ddq(Bx, c, i, nx, 1, hx) + ddq(By, c, j, ny, sy, hy) + ddq(Bz, c, k, nz, sz, hz);
  const double ox = O[c], oy = O[c + N], oz = O[c + 2 * N];
  const PS xm = ps_at(B, O, c - 1, N), xp = ps_at(B, O, c + 1, N);
  const PS ym = ps_at(B, O, c - sy, N), yp = ps_at(B, O, c + sy, N);
  double dzpx, dzpy, gsz;
  if (kLow) {
    const PS here = ps_of(bx, by, bz, ox, oy, oz);
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
    const PS here = ps_of(bx, by, bz, ox, oy, oz);
    fx = (w * fx - (here.py * gwz - here.pz * gwy)) - here.s * gwx;
    fy = (w * fy - (here.pz * gwx - here.px * gwz)) - here.s * gwy;
    fz = (w * fz - (here.px * gwy - here.py * gwx)) - here.s * gwz;
  }
}

// B, Omega: the current buffers, T: the other B buffer.  k is blockIdx.z, so the k = 0 branch is uniform per block.
// Bobs, wm, nu, free: read with kObs only.
template <class S, bool kObs>
__device__ __forceinline__ void force_pass(double *__restrict__ B0, double *__restrict__ B1,
                                           const double *__restrict__ O0, const double *__restrict__ O1,
                                           const double *__restrict__ wt, const double *__restrict__ Bobs,
                                           const double *__restrict__ wm, const double *__restrict__ state,
                                           const OptArgs &p, double nu, int free) {
  if (state[S::STOP] != 0.0) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  const int k = blockIdx.z;
  const int nx = p.n[0], ny = p.n[1], nz = p.n[2];
  if (i >= nx || j >= ny) return;
  const int cur = (int)state[S::CUR];
  const double dt = state[S::DT];
  const double *B = cur ? B1 : B0;
  const double *O = cur ? O1 : O0;
  double *T = cur ? B0 : B1;
  const size_t sy = (size_t)nx, sz = (size_t)nx * ny, N = sz * (size_t)nz;
  const size_t c = (size_t)i + sy * (size_t)j + sz * (size_t)k;
  const double bx = B[c], by = B[c + N], bz = B[c + 2 * N];
  const bool rim = i == 0 || i == nx - 1 || j == 0 || j == ny - 1;
  if (rim || k == nz - 1 || (k == 0 && !(kObs && free))) {
    T[c] = bx;
    T[c + N] = by;
    T[c + 2 * N] = bz;
    return;
  }
  double fx, fy, fz;
  if (kObs && k == 0) {
    ftilde<true>(B, O, wt, c, i, j, k, p, bx, by, bz, fx, fy, fz);
    const PS here = ps_at(B, O, c, N);
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
    fx = (fx + c2 * gx) - c2 * (nu * mx);
    fy = (fy + c2 * gy) - c2 * (nu * my);
    fz = (fz + c2 * gz) - c2 * (nu * mz);
  } else {
    ftilde<false>(B, O, wt, c, i, j, k, p, bx, by, bz, fx, fy, fz);
  }
  T[c] = bx + dt * fx;
  T[c + N] = by + dt * fy;
  T[c + 2 * N] = bz + dt * fz;
}

// the launch shape of a force pass: one thread per node
inline void force_shape(const OptArgs &p, dim3 &grid, dim3 &block) {
  block = dim3(64, 4, 1);
  grid = dim3((p.n[0] + 63) / 64, (p.n[1] + 3) / 4, p.n[2]);
}

}  // namespace ndsm
