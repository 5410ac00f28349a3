// Photospheric flows from two vector magnetograms, and the fluxes of relative helicity and magnetic energy through the
// lower face (DESIGN.md "Flow inversion and boundary fluxes").  The semantics - the staged quantities, the nine columns,
// the order of every sum, the scaled LDL^T and the status rules - are written out in include/ndsm_hip.h
// (ndsm_hip_flow_fit, ndsm_hip_flow_flux) and restated in numpy by tests/flow_model.py bit for bit (-ffp-contract=off,
// IEEE division and sqrt).  Here:
//
//   prep   flow_prep_k<0>  pointwise: Bm = 0.5 (B0 + B1) and T = (B1z - B0z) / dt into the planes 0..3 of the scratch
//          flow_prep_k<1>  pointwise: Zx, Zy and D, diffq.hpp's ddq of the planes just written, into the planes 4..6 -
//                          two launches of one kernel, so that ddq itself reads Bm from memory
//   fit    flow_fit_k      one lane per target pixel, a 16 x 16 tile of targets per workgroup of 256.  The seven planes
//                          of the tile and its halo of r pixels go through LDS ((16 + 2r)^2 56 B: 126 KiB at r = 16);
//                          a lane walks its window b ascending, a ascending, skips the pixels outside the magnetogram
//                          and keeps the 45 + 9 sums in registers.  The 9 x 9 scaled LDL^T, the two triangular solves
//                          and the unscaling are fully unrolled: every index is static, nothing goes to scratch memory.
//   flux   flux_part_k     block b walks the rows b, b + gridDim.x, ..., its lanes the pixels of a row: the four
//                          densities, and the six weighted sums through descent.hpp's block_part
//          flux_final_k    one block: block_final's fold and tree (the reduction behind ndsm_hip_vecpot_helicity)
// No atomics anywhere: the same input gives the same bits.
#include "descent.hpp"
#include "diffq.hpp"

#include <cmath>

namespace {

using ndsm::ddq;
using ndsm::i64;
using ndsm::trap_w;

constexpr int kTile = 16;               // targets per side of a workgroup's tile
constexpr int kFitBlock = kTile * kTile;
constexpr int kPlanes = 7;              // Bx, By, Bz, T, Zx, Zy, D
constexpr int kMaxR = 16;

struct FlowArgs {
  int nsx, nsy, r;
  size_t npix;
  double hx, hy, dt, rcond;
};

// STAGE 0: scr planes 0..3 <- Bm, T.  STAGE 1: scr planes 4..6 <- Zx, Zy, D of the planes 0..2
template <int STAGE>
__global__ __launch_bounds__(256) void flow_prep_k(const double *__restrict__ B0, const double *__restrict__ B1,
                                                   double *__restrict__ scr, FlowArgs p) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= p.npix) return;
  if (STAGE == 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) scr[(size_t)d * p.npix + c] = 0.5 * (B0[(size_t)d * p.npix + c] + B1[(size_t)d * p.npix + c]);
    scr[3 * p.npix + c] = (B1[2 * p.npix + c] - B0[2 * p.npix + c]) / p.dt;
  } else {
    const size_t j = c / (size_t)p.nsx;
    const int i = (int)(c - j * (size_t)p.nsx);
    const double *bx = scr, *by = scr + p.npix, *bz = scr + 2 * p.npix;
    scr[4 * p.npix + c] = ddq(bz, c, i, p.nsx, 1, p.hx);
    scr[5 * p.npix + c] = ddq(bz, c, (int)j, p.nsy, (size_t)p.nsx, p.hy);
    scr[6 * p.npix + c] = ddq(bx, c, i, p.nsx, 1, p.hx) + ddq(by, c, (int)j, p.nsy, (size_t)p.nsx, p.hy);
  }
}

// entry (k, l), k <= l, of the upper triangle of a symmetric 9 x 9 matrix, row after row
__host__ __device__ constexpr int tri(int k, int l) { return k * 9 - (k * (k - 1)) / 2 + (l - k); }
// entry (k, j), j < k, of a strictly lower triangle, row after row
__host__ __device__ constexpr int low(int k, int j) { return (k * (k - 1)) / 2 + j; }

__device__ __forceinline__ bool finite7(const double *v) {
  bool ok = true;
#pragma unroll
  for (int q = 0; q < kPlanes; ++q) ok = ok && (fabs(v[q]) <= 1.7976931348623157e308);
  return ok;
}

__global__ __launch_bounds__(kFitBlock) void flow_fit_k(const double *__restrict__ scr, FlowArgs p, double *__restrict__ V,
                                                        double *__restrict__ coef, int32_t *__restrict__ status) {
  extern __shared__ double lds[];
  const int r = p.r, W = kTile + 2 * r, WH = W * W;
  const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x >> 4;
  const int i0 = (int)blockIdx.x * kTile - r, j0 = (int)blockIdx.y * kTile - r;
  for (int n = threadIdx.x; n < WH; n += kFitBlock) {
    const int ly = n / W, lx = n - ly * W;
    const int gx = i0 + lx, gy = j0 + ly;
    if (gx >= 0 && gx < p.nsx && gy >= 0 && gy < p.nsy) {
      const size_t c = (size_t)gy * (size_t)p.nsx + (size_t)gx;
#pragma unroll
      for (int q = 0; q < kPlanes; ++q) lds[q * WH + n] = scr[(size_t)q * p.npix + c];
    }
  }
  __syncthreads();
  const int i = i0 + r + tx, j = j0 + r + ty;
  if (i >= p.nsx || j >= p.nsy) return;           // (no barrier below)

  double G[45], g[9];
#pragma unroll
  for (int q = 0; q < 45; ++q) G[q] = 0.0;
#pragma unroll
  for (int q = 0; q < 9; ++q) g[q] = 0.0;
  bool clean = true;
  const int b0 = j - r < 0 ? -j : -r, b1 = j + r > p.nsy - 1 ? p.nsy - 1 - j : r;
  const int a0 = i - r < 0 ? -i : -r, a1 = i + r > p.nsx - 1 ? p.nsx - 1 - i : r;
  for (int b = b0; b <= b1; ++b) {
    const double yp = (double)b * p.hy;
    const double *row = lds + (ty + r + b) * W + (tx + r);
    for (int a = a0; a <= a1; ++a) {
      const double xp = (double)a * p.hx;
      double v[kPlanes];
#pragma unroll
      for (int q = 0; q < kPlanes; ++q) v[q] = row[q * WH + a];
      clean = clean && finite7(v);
      const double Bx = v[0], By = v[1], Bz = v[2], T = v[3], Zx = v[4], Zy = v[5], D = v[6];
      double s[9];
      s[0] = Zx;
      s[1] = Zx * xp + Bz;
      s[2] = Zx * yp;
      s[3] = Zy;
      s[4] = Zy * xp;
      s[5] = Zy * yp + Bz;
      s[6] = -D;
      s[7] = -(D * xp) - Bx;
      s[8] = -(D * yp) - By;
      const double nT = -T;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
#pragma unroll
        for (int l = k; l < 9; ++l) G[tri(k, l)] = G[tri(k, l)] + s[k] * s[l];
        g[k] = g[k] + nT * s[k];
      }
    }
  }

  // scaling: d_k = 1 / sqrt(G_kk), Gs_kl = (G_kl d_k) d_l, gs_k = g_k d_k
  bool solved = true;
  double d[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    solved = solved && (G[tri(k, k)] > 0.0);
    d[k] = 1.0 / sqrt(G[tri(k, k)]);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int l = k; l < 9; ++l) G[tri(k, l)] = (G[tri(k, l)] * d[k]) * d[l];
    g[k] = g[k] * d[k];
  }
  // LDL^T by rows, no pivoting: w_kj = Gs_jk - sum_{m<j} w_km L_jm, L_kj = w_kj / D_j, D_k = Gs_kk - sum_{j<k} w_kj L_kj
  double L[36], Dg[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    double w[9];
#pragma unroll
    for (int jj = 0; jj < k; ++jj) {
      double acc = 0.0;
#pragma unroll
      for (int m = 0; m < jj; ++m) acc = acc + w[m] * L[low(jj, m)];
      w[jj] = G[tri(jj, k)] - acc;
      L[low(k, jj)] = w[jj] / Dg[jj];
    }
    double acc = 0.0;
#pragma unroll
    for (int jj = 0; jj < k; ++jj) acc = acc + w[jj] * L[low(k, jj)];
    Dg[k] = G[tri(k, k)] - acc;
    solved = solved && (Dg[k] > p.rcond);
  }
  // L y = gs, z = y / D, L^T ps = z, p = ps d
  double y[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    double acc = 0.0;
#pragma unroll
    for (int jj = 0; jj < k; ++jj) acc = acc + L[low(k, jj)] * y[jj];
    y[k] = g[k] - acc;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) y[k] = y[k] / Dg[k];
#pragma unroll
  for (int k = 8; k >= 0; --k) {
    double acc = 0.0;
#pragma unroll
    for (int jj = k + 1; jj < 9; ++jj) acc = acc + L[low(jj, k)] * y[jj];
    y[k] = y[k] - acc;
  }
  const int st = !clean ? 2 : (solved ? 0 : 1);
  const size_t c = (size_t)j * (size_t)p.nsx + (size_t)i;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double pk = st == 0 ? y[k] * d[k] : (st == 1 ? 0.0 : __builtin_nan(""));
    coef[(size_t)k * p.npix + c] = pk;
    if (k % 3 == 0) V[(size_t)(k / 3) * p.npix + c] = pk;
  }
  status[c] = st;
}

constexpr int kFluxBlock = ndsm::kRedBlock;
constexpr int kFluxVals = 6;            // sums of w h_em, w h_sh, w s_em, w s_sh, w |Bz|, w Bz

__global__ __launch_bounds__(kFluxBlock) void flux_part_k(const double *__restrict__ B, const double *__restrict__ V,
                                                          const double *__restrict__ Ap, double *__restrict__ dens,
                                                          double *__restrict__ part, FlowArgs p) {
  __shared__ double sh[kFluxVals][kFluxBlock];
  double v[kFluxVals];
  for (int q = 0; q < kFluxVals; ++q) v[q] = 0.0;
  for (int j = blockIdx.x; j < p.nsy; j += gridDim.x) {
    const double wy = trap_w(j, p.nsy, p.hy);
    for (int i = threadIdx.x; i < p.nsx; i += kFluxBlock) {
      const size_t c = (size_t)j * (size_t)p.nsx + (size_t)i;
      const double w = trap_w(i, p.nsx, p.hx) * wy;
      const double bx = B[c], by = B[p.npix + c], bz = B[2 * p.npix + c];
      const double vx = V[c], vy = V[p.npix + c], vz = V[2 * p.npix + c];
      const double ax = Ap[c], ay = Ap[p.npix + c];
      const double hem = 2.0 * ((ax * bx + ay * by) * vz);
      const double hsh = -2.0 * ((ax * vx + ay * vy) * bz);
      const double sem = (bx * bx + by * by) * vz;
      const double ssh = -((bx * vx + by * vy) * bz);
      dens[c] = hem;
      dens[p.npix + c] = hsh;
      dens[2 * p.npix + c] = sem;
      dens[3 * p.npix + c] = ssh;
      v[0] = v[0] + w * hem;
      v[1] = v[1] + w * hsh;
      v[2] = v[2] + w * sem;
      v[3] = v[3] + w * ssh;
      v[4] = v[4] + w * fabs(bz);
      v[5] = v[5] + w * bz;
    }
  }
  ndsm::block_part<kFluxVals, kFluxVals>(sh, v, part);
}

__global__ __launch_bounds__(kFluxBlock) void flux_final_k(const double *__restrict__ part, int nb,
                                                           double *__restrict__ out) {
  __shared__ double sh[kFluxVals][kFluxBlock];
  ndsm::block_final<kFluxVals, kFluxVals>(sh, part, nb);
  if (threadIdx.x < kFluxVals) out[threadIdx.x] = sh[threadIdx.x][0];
}

// scratch of the calls, kept between calls and grown on demand (no result depends on its size): the seven planes of
// the fit; the block partials and the pinned sums of the fluxes
struct FlowScratch {
  void *a = nullptr;
  size_t cap = 0;
  double *d_part = nullptr;    // [kRedMaxBlocks * kFluxVals + kFluxVals]
  double *h_pin = nullptr;     // [kFluxVals] pinned
  bool registered = false;
};
FlowScratch g_flow;

void flow_release() {
  if (g_flow.a) (void)hipFree(g_flow.a);
  if (g_flow.d_part) (void)hipFree(g_flow.d_part);
  if (g_flow.h_pin) (void)hipHostFree(g_flow.h_pin);
  g_flow = FlowScratch();
}

void flow_register() {
  if (g_flow.registered) return;
  ndsm::at_reset(flow_release);
  g_flow.registered = true;
}

int flow_grow(size_t bytes) {
  flow_register();
  if (bytes <= g_flow.cap) return 0;
  if (g_flow.a) {
    const int rc = ndsmk_free(g_flow.a);      // (drains the streams first)
    g_flow.a = nullptr;
    g_flow.cap = 0;
    if (rc != 0) return rc;
  }
  const int rc = ndsmk_alloc(&g_flow.a, bytes);
  if (rc != 0) return rc;
  g_flow.cap = bytes;
  return 0;
}

int flux_scratch() {
  flow_register();
  if (!g_flow.d_part)
    NDSM_HIP(hipMalloc((void **)&g_flow.d_part, sizeof(double) * (ndsm::kRedMaxBlocks * kFluxVals + kFluxVals)));
  if (!g_flow.h_pin) NDSM_HIP(hipHostMalloc((void **)&g_flow.h_pin, sizeof(double) * kFluxVals, hipHostMallocDefault));
  return 0;
}

// the mesh of a call: at least nmin nodes per axis and both spacings > 0 (false for a NaN as well)
bool mesh_ok(const int32_t *nsrc2, const double *h_xs, const double *h_ys, int nmin) {
  if (nsrc2[0] < nmin || nsrc2[1] < nmin) return false;
  return h_xs[1] - h_xs[0] > 0.0 && h_ys[1] - h_ys[0] > 0.0;
}

}  // namespace

// 0, or 9001 when the device cannot hold a call's arrays: caller_bytes of the caller's side (staged host arrays) plus,
// for the fit, the seven planes, against the device's TOTAL memory - ndsmk_green_fits' screen, all in doubles
extern "C" int ndsmk_flow_fits(const int32_t *nsrc2, int fit, double caller_bytes) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(nsrc2);
  size_t fr = 0, tot = 0;
  const int rc = ndsmk_mem_info(&fr, &tot);
  if (rc != 0) return rc;
  if (caller_bytes + (fit ? 8.0 * kPlanes * (double)nsrc2[0] * (double)nsrc2[1] : 0.0) > (double)tot)
    return ndsmk_note_error(NDSMK_ENODEV, "flow: the arrays and the scratch need more device memory than the device has");
  return 0;
}

// The flow fit (semantics: include/ndsm_hip.h, ndsm_hip_flow_fit).  B0, B1, V (nsx,nsy,3), coef (nsx,nsy,9) and status
// (nsx,nsy; int32) are DEVICE arrays, h_xs and h_ys on the HOST.  Returns when the outputs are complete.
extern "C" int ndsmk_flow_fit(const int32_t *nsrc2, const double *h_xs, const double *h_ys, const double *B0,
                              const double *B1, double dt, int r, double rcond, double *V, double *coef,
                              int32_t *status) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(nsrc2 && h_xs && h_ys && B0 && B1 && V && coef && status);
  if (!mesh_ok(nsrc2, h_xs, h_ys, 3) || !std::isfinite(dt) || dt == 0.0 || r < 1 || r > kMaxR || !(rcond >= 0.0) ||
      !(rcond < 1.0))
    return ndsmk_note_error(NDSMK_EVALUE, "flow_fit: at least 3 nodes per axis, spacings > 0, a finite dt != 0, "
                                          "1 <= r <= 16 and 0 <= rcond < 1");
  FlowArgs p;
  p.nsx = nsrc2[0];
  p.nsy = nsrc2[1];
  p.r = r;
  p.npix = (size_t)p.nsx * (size_t)p.nsy;
  p.hx = h_xs[1] - h_xs[0];
  p.hy = h_ys[1] - h_ys[0];
  p.dt = dt;
  p.rcond = rcond;
  const size_t nb = (p.npix + 255) / 256;
  const unsigned gx = (unsigned)((p.nsx + kTile - 1) / kTile), gy = (unsigned)((p.nsy + kTile - 1) / kTile);
  NDSM_CHECK_ARG(nb <= (size_t)0x7fffffff && gy <= 65535u);
  int rc = flow_grow(sizeof(double) * kPlanes * p.npix);
  if (rc != 0) return rc;
  double *scr = (double *)g_flow.a;
  const size_t lds_bytes = sizeof(double) * kPlanes * (size_t)(kTile + 2 * r) * (size_t)(kTile + 2 * r);
  static int attr_epoch = 0;
  if (ndsm::first_in_epoch(attr_epoch))
    NDSM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(flow_fit_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(sizeof(double) * kPlanes * (kTile + 2 * kMaxR) * (kTile + 2 * kMaxR))));
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(flow_prep_k<0>, dim3((unsigned)nb), dim3(256), 0, s, B0, B1, scr, p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(flow_prep_k<1>, dim3((unsigned)nb), dim3(256), 0, s, B0, B1, scr, p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(flow_fit_k, dim3(gx, gy), dim3(kFitBlock), lds_bytes, s, scr, p, V, coef, status);
  NDSM_LAUNCH_CHECK();
  NDSM_HIP(hipStreamSynchronize(s));
  return 0;
}

// The boundary fluxes (semantics: include/ndsm_hip.h, ndsm_hip_flow_flux).  B, V (nsx,nsy,3), Ap (nsx,nsy,2) and dens
// (nsx,nsy,4) are DEVICE arrays; h_xs, h_ys and h_out8 on the HOST.  Blocking: one read of the six sums.
extern "C" int ndsmk_flow_flux(const int32_t *nsrc2, const double *h_xs, const double *h_ys, const double *B,
                               const double *V, const double *Ap, double *dens, double *h_out8) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(nsrc2 && h_xs && h_ys && B && V && Ap && dens && h_out8);
  if (!mesh_ok(nsrc2, h_xs, h_ys, 2))
    return ndsmk_note_error(NDSMK_EVALUE, "flow_flux: at least 2 nodes per axis and spacings > 0");
  if (int rc = flux_scratch()) return rc;
  FlowArgs p = {};
  p.nsx = nsrc2[0];
  p.nsy = nsrc2[1];
  p.npix = (size_t)p.nsx * (size_t)p.nsy;
  p.hx = h_xs[1] - h_xs[0];
  p.hy = h_ys[1] - h_ys[0];
  const int nb = ndsm::red_blocks((size_t)p.nsy);
  double *out = g_flow.d_part + (size_t)ndsm::kRedMaxBlocks * kFluxVals;
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(flux_part_k, dim3(nb), dim3(kFluxBlock), 0, s, B, V, Ap, dens, g_flow.d_part, p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(flux_final_k, dim3(1), dim3(kFluxBlock), 0, s, g_flow.d_part, nb, out);
  NDSM_LAUNCH_CHECK();
  NDSM_HIP(hipMemcpyAsync(g_flow.h_pin, out, kFluxVals * sizeof(double), hipMemcpyDeviceToHost, s));
  NDSM_HIP(hipStreamSynchronize(s));
  const double *v = g_flow.h_pin;
  h_out8[0] = v[0];
  h_out8[1] = v[1];
  h_out8[2] = v[0] + v[1];
  h_out8[3] = v[2];
  h_out8[4] = v[3];
  h_out8[5] = v[2] + v[3];
  h_out8[6] = v[4];
  h_out8[7] = v[5];
  return 0;
}
