// The current-carrying field on the device: what the vector potential of a field with curl B != 0 adds to
// the potential pipeline (DESIGN.md "Vector potential of a current-carrying field"):
//
//   curl_rhs : rhs_c = -(curl B)_c, the right-hand side of the 3-D problem laplace(A_c) = -J_c, written
//              straight into the level-1 rhs of component c's solver.  The differences and expressions of
//              post.hip's curl_k (derivq, ndsm_vector_potential.f90:852-870), negated: the same bits as
//              -curl_k(B).  Streaming: two components of B in, one array out (24 B/pt).
//   current_rhs : rhs_c = -J_c for a current J the caller prescribes (alpha == nullptr), or rhs_c = -(alpha F_c) for
//              the Grad-Rubin pass, J = alpha B formed on the way: one rounding and a sign.  8 or 16 B/pt in, 8 out.
//   nlfff metrics : one pass over B^{k+1}, B^k and the alpha map's status -> the history row of a Grad-Rubin pass (the
//              change, the energy, the current-weighted sine, the lines that reach the lower face), with the
//              helicity reduction's deterministic row walk and tree.
//   helicity : one pass over A, A_p, B, B_p and B_rec (the field solve's curl A + balance) with trapezoid
//              weights -> relative helicity (Finn-Antonsen), the mutual term, both energies, the
//              reconstruction error and the two divergences (15 arrays, 120 B/pt).  Deterministic: every
//              block sums a fixed set of grid rows in a fixed order, one block then sums the block
//              partials in a fixed order; the grid size depends on the shape alone.
#include "descent.hpp"
#include "diffq.hpp"

namespace {

struct CurlArgs {
  int n[3];
  double dq[3];
};

using ndsm::ddq;
using ndsm::trap_w;

template <int C>
__global__ __launch_bounds__(256) void curl_rhs_k(const double *__restrict__ B, double *__restrict__ rhs, CurlArgs p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  const int k = blockIdx.z;
  if (i >= p.n[0] || j >= p.n[1]) return;
  const size_t sy = (size_t)p.n[0], sz = (size_t)p.n[0] * p.n[1];
  const size_t N = sz * (size_t)p.n[2];
  const size_t c = (size_t)i + sy * (size_t)j + sz * (size_t)k;
  const double *Bx = B, *By = B + N, *Bz = B + 2 * N;
  if (C == 0) {
    const double byz = ddq(By, c, k, p.n[2], sz, p.dq[2]);
    const double bzy = ddq(Bz, c, j, p.n[1], sy, p.dq[1]);
    rhs[c] = -(bzy - byz);
  } else if (C == 1) {
    const double bxz = ddq(Bx, c, k, p.n[2], sz, p.dq[2]);
    const double bzx = ddq(Bz, c, i, p.n[0], 1, p.dq[0]);
    rhs[c] = -(bxz - bzx);
  } else {
    const double bxy = ddq(Bx, c, j, p.n[1], sy, p.dq[1]);
    const double byx = ddq(By, c, i, p.n[0], 1, p.dq[0]);
    rhs[c] = -(byx - bxy);
  }
}

// rhs = -(a F) with a = alpha[c] (or 1: rhs = -F), one component
__global__ __launch_bounds__(256) void current_rhs_k(const double *__restrict__ F, const double *__restrict__ alpha,
                                                     double *__restrict__ rhs, size_t n) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  rhs[c] = alpha ? -(alpha[c] * F[c]) : -F[c];
}

constexpr int kHelBlock = ndsm::kRedBlock;           // descent.hpp's reduction: block_part, block_final
constexpr int kHelMaxBlocks = ndsm::kRedMaxBlocks;
constexpr int kHelVals = 9;           // 6 sums, 3 maxima
constexpr int kHelSums = 6;

struct HelArgs {
  int n[3];
  double dq[3];
  size_t nrows;   // ny * nz
};

// block partials: v[0..5] = sums of w (A+Ap).(B-Bp), w (A-Ap).(B-Bp), w |B|^2, w |Bp|^2, w |Br-B|^2, w;
// v[6..8] = maxima of |Br-B| (over points and components), |div_h B|, |div_h A|.  Block b walks rows b,
// b + gridDim.x, ...; its threads the points of a row.
__global__ __launch_bounds__(kHelBlock) void helicity_part_k(const double *__restrict__ A, const double *__restrict__ Ap,
                                                            const double *__restrict__ B, const double *__restrict__ Bp,
                                                            const double *__restrict__ Br, double *__restrict__ part,
                                                            HelArgs p) {
  __shared__ double sh[kHelVals][kHelBlock];
  const int t = threadIdx.x;
  const int nx = p.n[0], ny = p.n[1], nz = p.n[2];
  const size_t sy = (size_t)nx, sz = (size_t)nx * ny, N = sz * (size_t)nz;
  double v[kHelVals];
  for (int q = 0; q < kHelVals; ++q) v[q] = 0.0;
  for (size_t r = blockIdx.x; r < p.nrows; r += gridDim.x) {
    const int j = (int)(r % (size_t)ny), k = (int)(r / (size_t)ny);
    const double wyz = trap_w(j, ny, p.dq[1]) * trap_w(k, nz, p.dq[2]);
    for (int i = t; i < nx; i += kHelBlock) {
      const size_t c = (size_t)i + sy * (size_t)j + sz * (size_t)k;
      const double w = trap_w(i, nx, p.dq[0]) * wyz;
      double hr = 0.0, hj = 0.0, bb = 0.0, pp = 0.0, ee = 0.0, em = 0.0;
      for (int d = 0; d < 3; ++d) {
        const size_t o = c + (size_t)d * N;
        const double a = A[o], ap = Ap[o], b = B[o], bp = Bp[o], br = Br[o];
        const double db = b - bp, e = br - b;
        hr = hr + (a + ap) * db;
        hj = hj + (a - ap) * db;
        bb = bb + b * b;
        pp = pp + bp * bp;
        ee = ee + e * e;
        em = fmax(em, fabs(e));
      }
      v[0] = v[0] + w * hr;
      v[1] = v[1] + w * hj;
      v[2] = v[2] + w * bb;
      v[3] = v[3] + w * pp;
      v[4] = v[4] + w * ee;
      v[5] = v[5] + w;
      v[6] = fmax(v[6], em);
      const double divb = ddq(B, c, i, nx, 1, p.dq[0]) + ddq(B + N, c, j, ny, sy, p.dq[1]) +
                          ddq(B + 2 * N, c, k, nz, sz, p.dq[2]);
      const double diva = ddq(A, c, i, nx, 1, p.dq[0]) + ddq(A + N, c, j, ny, sy, p.dq[1]) +
                          ddq(A + 2 * N, c, k, nz, sz, p.dq[2]);
      v[7] = fmax(v[7], fabs(divb));
      v[8] = fmax(v[8], fabs(diva));
    }
  }
  ndsm::block_part<kHelVals, kHelSums>(sh, v, part);
}

// one block: descent.hpp's fold (thread t: the partials of blocks t, t + 256, ... in that order) and halving tree
__global__ __launch_bounds__(kHelBlock) void helicity_final_k(const double *__restrict__ part, int nb,
                                                             double *__restrict__ out) {
  __shared__ double sh[kHelVals][kHelBlock];
  ndsm::block_final<kHelVals, kHelSums>(sh, part, nb);
  if (threadIdx.x < kHelVals) out[threadIdx.x] = sh[threadIdx.x][0];
}

constexpr int kNlVals = 5;            // 4 sums, 1 maximum
constexpr int kNlSums = 4;

// block partials of a Grad-Rubin pass: v[0..3] = sums of w |B|^2, w |J x B| / |B|, w |J|, [status == ZLO];
// v[4] = the maximum of |B_c - Bold_c| over points and components.  J = curl_h B (derivq's differences); points where
// |B| is not > 0 add to neither of the two current sums.  Rows and threads as helicity_part_k.
__global__ __launch_bounds__(kHelBlock) void nlfff_part_k(const double *__restrict__ B, const double *__restrict__ Bold,
                                                         const int32_t *__restrict__ status, double *__restrict__ part,
                                                         HelArgs p) {
  __shared__ double sh[kNlVals][kHelBlock];
  const int t = threadIdx.x;
  const int nx = p.n[0], ny = p.n[1], nz = p.n[2];
  const size_t sy = (size_t)nx, sz = (size_t)nx * ny, N = sz * (size_t)nz;
  const double *Bx = B, *By = B + N, *Bz = B + 2 * N;
  double v[kNlVals];
  for (int q = 0; q < kNlVals; ++q) v[q] = 0.0;
  for (size_t r = blockIdx.x; r < p.nrows; r += gridDim.x) {
    const int j = (int)(r % (size_t)ny), k = (int)(r / (size_t)ny);
    const double wyz = trap_w(j, ny, p.dq[1]) * trap_w(k, nz, p.dq[2]);
    for (int i = t; i < nx; i += kHelBlock) {
      const size_t c = (size_t)i + sy * (size_t)j + sz * (size_t)k;
      const double w = trap_w(i, nx, p.dq[0]) * wyz;
      const double bx = Bx[c], by = By[c], bz = Bz[c];
      const double bb = (bx * bx + by * by) + bz * bz;
      v[0] = v[0] + w * bb;
      // curl_k's expressions (post.hip)
      const double jx = ddq(Bz, c, j, ny, sy, p.dq[1]) - ddq(By, c, k, nz, sz, p.dq[2]);
      const double jy = ddq(Bx, c, k, nz, sz, p.dq[2]) - ddq(Bz, c, i, nx, 1, p.dq[0]);
      const double jz = ddq(By, c, i, nx, 1, p.dq[0]) - ddq(Bx, c, j, ny, sy, p.dq[1]);
      const double bm = sqrt(bb);
      if (bm > 0.0) {
        const double cx = jy * bz - jz * by, cy = jz * bx - jx * bz, cz = jx * by - jy * bx;
        v[1] = v[1] + w * (sqrt((cx * cx + cy * cy) + cz * cz) / bm);
        v[2] = v[2] + w * sqrt((jx * jx + jy * jy) + jz * jz);
      }
      if (status[c] == NDSMK_TRACE_ZLO) v[3] = v[3] + 1.0;
      double em = fabs(bx - Bold[c]);
      em = fmax(em, fabs(by - Bold[c + N]));
      em = fmax(em, fabs(bz - Bold[c + 2 * N]));
      v[4] = fmax(v[4], em);
    }
  }
  ndsm::block_part<kNlVals, kNlSums>(sh, v, part);
}

// one block: helicity_final_k's fold and tree over the partials of nlfff_part_k
__global__ __launch_bounds__(kHelBlock) void nlfff_final_k(const double *__restrict__ part, int nb,
                                                          double *__restrict__ out) {
  __shared__ double sh[kNlVals][kHelBlock];
  ndsm::block_final<kNlVals, kNlSums>(sh, part, nb);
  if (threadIdx.x < kNlVals) out[threadIdx.x] = sh[threadIdx.x][0];
}

struct HelScratch {
  double *d_part = nullptr;   // [kHelMaxBlocks * kHelVals + kHelVals]: block partials, then the result
  double *h_pin = nullptr;    // [kHelVals] pinned
};
HelScratch g_hel;

void hel_release() {
  if (g_hel.d_part) (void)hipFree(g_hel.d_part);
  if (g_hel.h_pin) (void)hipHostFree(g_hel.h_pin);
  g_hel = HelScratch();
}

// the scratch of the two reductions, allocated at the first (nlfff_part_k's kNlVals <= kHelVals values fit)
int hel_scratch() {
  if (g_hel.d_part) return 0;
  ndsm::at_reset(hel_release);
  NDSM_HIP(hipMalloc((void **)&g_hel.d_part, sizeof(double) * (kHelMaxBlocks * kHelVals + kHelVals)));
  NDSM_HIP(hipHostMalloc((void **)&g_hel.h_pin, sizeof(double) * kHelVals, hipHostMallocDefault));
  return 0;
}

}  // namespace

// rhs = -(curl B)_c on the whole field: B (nx,ny,nz,3), rhs (nx,ny,nz), both DEVICE arrays; c = 0, 1, 2
extern "C" int ndsmk_curl_rhs(const double *B, double *rhs, const int32_t *n3, const double *h_dq3, int c) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B && rhs && n3[0] >= 3 && n3[1] >= 3 && n3[2] >= 3 && n3[2] <= 65535 && c >= 0 && c < 3);
  CurlArgs p;
  for (int d = 0; d < 3; ++d) {
    p.n[d] = n3[d];
    p.dq[d] = h_dq3[d];
  }
  dim3 block(64, 4, 1);
  dim3 grid((n3[0] + 63) / 64, (n3[1] + 3) / 4, n3[2]);
  if (c == 0)
    hipLaunchKernelGGL(curl_rhs_k<0>, grid, block, 0, ndsm::stream(), B, rhs, p);
  else if (c == 1)
    hipLaunchKernelGGL(curl_rhs_k<1>, grid, block, 0, ndsm::stream(), B, rhs, p);
  else
    hipLaunchKernelGGL(curl_rhs_k<2>, grid, block, 0, ndsm::stream(), B, rhs, p);
  NDSM_LAUNCH_CHECK();
  return 0;
}

// rhs = -(F_c) of a prescribed current F = J (alpha == nullptr), or rhs = -(alpha F_c) with F = B (the Grad-Rubin pass):
// F (nx,ny,nz,3), alpha (nx,ny,nz), rhs (nx,ny,nz), all DEVICE arrays; c = 0, 1, 2
extern "C" int ndsmk_current_rhs(const double *F, const double *alpha, double *rhs, const int32_t *n3, int c) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(F && rhs && n3[0] >= 1 && n3[1] >= 1 && n3[2] >= 1 && c >= 0 && c < 3);
  const size_t n = (size_t)n3[0] * (size_t)n3[1] * (size_t)n3[2];
  const size_t nb = (n + 255) / 256;
  NDSM_CHECK_ARG(nb <= (size_t)0x7fffffff);
  hipLaunchKernelGGL(current_rhs_k, dim3((unsigned)nb), dim3(256), 0, ndsm::stream(), F + (size_t)c * n, alpha, rhs, n);
  NDSM_LAUNCH_CHECK();
  return 0;
}

// Blocking.  A, Ap, B, Bp, Br: DEVICE arrays (nx,ny,nz,3).  h_out8 (host):
//   [0] H_R = sum w (A+Ap).(B-Bp)   [1] H_J = sum w (A-Ap).(B-Bp)   [2] E = 1/2 sum w |B|^2
//   [3] E_p = 1/2 sum w |Bp|^2      [4] max |Br_c-B_c|              [5] sqrt(sum w |Br-B|^2 / sum w)
//   [6] max |div_h B|               [7] max |div_h A|
// w = w_x w_y w_z, w_d = h_d inside and h_d / 2 on both end planes; div_h with derivq's differences.
extern "C" int ndsmk_helicity_reduce(const double *A, const double *Ap, const double *B, const double *Bp,
                                     const double *Br, const int32_t *n3, const double *h_dq3, double *h_out8) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(A && Ap && B && Bp && Br && h_out8 && n3[0] >= 3 && n3[1] >= 3 && n3[2] >= 3);
  if (int rc = hel_scratch()) return rc;
  HelArgs p;
  for (int d = 0; d < 3; ++d) {
    p.n[d] = n3[d];
    p.dq[d] = h_dq3[d];
  }
  p.nrows = (size_t)n3[1] * (size_t)n3[2];
  const int nb = ndsm::red_blocks(p.nrows);
  double *out = g_hel.d_part + (size_t)kHelMaxBlocks * kHelVals;
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(helicity_part_k, dim3(nb), dim3(kHelBlock), 0, s, A, Ap, B, Bp, Br, g_hel.d_part, p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(helicity_final_k, dim3(1), dim3(kHelBlock), 0, s, g_hel.d_part, nb, out);
  NDSM_LAUNCH_CHECK();
  NDSM_HIP(hipMemcpyAsync(g_hel.h_pin, out, kHelVals * sizeof(double), hipMemcpyDeviceToHost, s));
  NDSM_HIP(hipStreamSynchronize(s));
  const double *v = g_hel.h_pin;
  h_out8[0] = v[0];
  h_out8[1] = v[1];
  h_out8[2] = 0.5 * v[2];
  h_out8[3] = 0.5 * v[3];
  h_out8[4] = v[6];
  h_out8[5] = sqrt(v[4] / v[5]);
  h_out8[6] = v[7];
  h_out8[7] = v[8];
  return 0;
}

// Blocking.  The history row of a Grad-Rubin pass: B (the new field), Bold (the field before), DEVICE arrays
// (nx,ny,nz,3); status the alpha map's (nx,ny,nz; int32, DEVICE).  h_out4 (host):
//   [0] max |B_c - Bold_c|   [1] 1/2 sum w |B|^2   [2] sum w |J x B| / |B| over sum w |J|, J = curl_h B (0 when the
//   denominator is 0)        [3] the number of nodes whose status is NDSMK_TRACE_ZLO
// Weights and differences as ndsmk_helicity_reduce; the same scratch and the same deterministic order.
extern "C" int ndsmk_nlfff_metrics(const double *B, const double *Bold, const int32_t *status, const int32_t *n3,
                                   const double *h_dq3, double *h_out4) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B && Bold && status && h_out4 && n3[0] >= 3 && n3[1] >= 3 && n3[2] >= 3);
  if (int rc = hel_scratch()) return rc;
  HelArgs p;
  for (int d = 0; d < 3; ++d) {
    p.n[d] = n3[d];
    p.dq[d] = h_dq3[d];
  }
  p.nrows = (size_t)n3[1] * (size_t)n3[2];
  const int nb = ndsm::red_blocks(p.nrows);
  double *out = g_hel.d_part + (size_t)kHelMaxBlocks * kHelVals;
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(nlfff_part_k, dim3(nb), dim3(kHelBlock), 0, s, B, Bold, status, g_hel.d_part, p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(nlfff_final_k, dim3(1), dim3(kHelBlock), 0, s, g_hel.d_part, nb, out);
  NDSM_LAUNCH_CHECK();
  NDSM_HIP(hipMemcpyAsync(g_hel.h_pin, out, kNlVals * sizeof(double), hipMemcpyDeviceToHost, s));
  NDSM_HIP(hipStreamSynchronize(s));
  const double *v = g_hel.h_pin;
  h_out4[0] = v[4];
  h_out4[1] = 0.5 * v[0];
  h_out4[2] = v[2] > 0.0 ? v[1] / v[2] : 0.0;
  h_out4[3] = v[3];
  return 0;
}
