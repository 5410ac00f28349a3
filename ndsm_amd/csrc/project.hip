// Solenoidal projection of a field on the device (DESIGN.md "Solenoidal projection"): B' = B - G_h phi with
// laplace_7(phi) = div_h B - c, all six faces Neumann.  The Poisson solve is the ordinary 3-D multigrid; these
// are the streaming passes around it:
//
//   div_rhs  : d = div_h B (derivq's differences, ddq0) straight into the level-1 rhs of the projection solver,
//              with block partials of sum w d, sum w, max |d|; one block folds them and forms
//              c = sum w d / sum w on the device; a streaming pass makes rhs = d - c.  No host read-back.
//              B in, rhs out, then rhs in and out: 24 + 16 B/pt.
//   grad_sub : B_q -= (G_h phi)_q at the points inside along axis q (the centred rows of ddq); the normal
//              component on the two end planes of its axis is not written at all.  Block partials of
//              sum w |G_h phi|^2.  phi and B in, B out: 8 + 24 + 24 B/pt (the end planes are not written).
//   div_max  : max |div_h B'| (and sum w div_h B') with the expressions of div_rhs, then the one read-back.
//              24 B/pt.
// Every reduction is deterministic: block b sums grid rows b, b + gridDim.x, ... in that order (the grid size
// depends on the shape alone), one block folds the block partials in a fixed order and a fixed halving tree.
#include "descent.hpp"
#include "diffq.hpp"

namespace {

using ndsm::ddq;
using ndsm::ddq0;
using ndsm::trap_w;

constexpr int kPrjBlock = ndsm::kRedBlock;           // descent.hpp's reduction: block_part, block_final
constexpr int kPrjMaxBlocks = ndsm::kRedMaxBlocks;
constexpr int kPrjVals = 3;           // per block: sum w d, sum w, max |d|  (grad_sub: sum w |G phi|^2)
constexpr int kPrjRes = 8;            // device results: [0..3] div_rhs (+ c), [4] grad_sub, [5..7] div_max

struct PrjArgs {
  int n[3];
  double dq[3];
  size_t nrows;   // ny * nz
};

PrjArgs prj_args(const int32_t *n3, const double *h_dq3) {
  PrjArgs p;
  for (int d = 0; d < 3; ++d) {
    p.n[d] = n3[d];
    p.dq[d] = h_dq3[d];
  }
  p.nrows = (size_t)n3[1] * (size_t)n3[2];
  return p;
}

int prj_blocks(const PrjArgs &p) { return ndsm::red_blocks(p.nrows); }

// d = div_h B with ddq0 on every axis, in the order x, y, z
__device__ __forceinline__ double div_h(const double *__restrict__ B, size_t c, int i, int j, int k, size_t N,
                                        size_t sy, size_t sz, const PrjArgs &p) {
  return ddq0(B, c, i, p.n[0], 1, p.dq[0]) + ddq0(B + N, c, j, p.n[1], sy, p.dq[1]) +
         ddq0(B + 2 * N, c, k, p.n[2], sz, p.dq[2]);
}

// block partials of div_h B: sum w d, sum w, max |d|; RHS: d is also written to rhs
template <bool RHS>
__global__ __launch_bounds__(kPrjBlock) void div_part_k(const double *__restrict__ B, double *__restrict__ rhs,
                                                        double *__restrict__ part, PrjArgs p) {
  __shared__ double sh[kPrjVals][kPrjBlock];
  const int t = threadIdx.x;
  const int nx = p.n[0], ny = p.n[1], nz = p.n[2];
  const size_t sy = (size_t)nx, sz = (size_t)nx * ny, N = sz * (size_t)nz;
  double v[kPrjVals] = {0.0, 0.0, 0.0};
  for (size_t r = blockIdx.x; r < p.nrows; r += gridDim.x) {
    const int j = (int)(r % (size_t)ny), k = (int)(r / (size_t)ny);
    const double wyz = trap_w(j, ny, p.dq[1]) * trap_w(k, nz, p.dq[2]);
    for (int i = t; i < nx; i += kPrjBlock) {
      const size_t c = (size_t)i + sy * (size_t)j + sz * (size_t)k;
      const double w = trap_w(i, nx, p.dq[0]) * wyz;
      const double d = div_h(B, c, i, j, k, N, sy, sz, p);
      if (RHS) rhs[c] = d;
      v[0] = v[0] + w * d;
      v[1] = v[1] + w;
      v[2] = fmax(v[2], fabs(d));
    }
  }
  ndsm::block_part<kPrjVals, 2>(sh, v, part);
}

// B_q -= (G_h phi)_q where index q is inside its axis; block partials of sum w |G_h phi|^2 in slot 0
__global__ __launch_bounds__(kPrjBlock) void grad_sub_k(double *__restrict__ B, const double *__restrict__ phi,
                                                        double *__restrict__ part, PrjArgs p) {
  __shared__ double sh[1][kPrjBlock];
  const int t = threadIdx.x;
  const int nx = p.n[0], ny = p.n[1], nz = p.n[2];
  const size_t sy = (size_t)nx, sz = (size_t)nx * ny, N = sz * (size_t)nz;
  double v[1] = {0.0};
  for (size_t r = blockIdx.x; r < p.nrows; r += gridDim.x) {
    const int j = (int)(r % (size_t)ny), k = (int)(r / (size_t)ny);
    const double wyz = trap_w(j, ny, p.dq[1]) * trap_w(k, nz, p.dq[2]);
    const bool yin = j > 0 && j < ny - 1, zin = k > 0 && k < nz - 1;
    for (int i = t; i < nx; i += kPrjBlock) {
      const size_t c = (size_t)i + sy * (size_t)j + sz * (size_t)k;
      const double w = trap_w(i, nx, p.dq[0]) * wyz;
      double e = 0.0;
      if (i > 0 && i < nx - 1) {
        const double g = ddq(phi, c, i, nx, 1, p.dq[0]);
        B[c] = B[c] - g;
        e = e + g * g;
      }
      if (yin) {
        const double g = ddq(phi, c, j, ny, sy, p.dq[1]);
        B[c + N] = B[c + N] - g;
        e = e + g * g;
      }
      if (zin) {
        const double g = ddq(phi, c, k, nz, sz, p.dq[2]);
        B[c + 2 * N] = B[c + 2 * N] - g;
        e = e + g * g;
      }
      v[0] = v[0] + w * e;
    }
  }
  ndsm::block_part<1, 1>(sh, v, part, kPrjVals);
}

// one block: descent.hpp's fold (thread t: the partials of blocks t, t + 256, ... in that order) and halving tree; the
// NV results go to out[0..NV-1], and (MEAN) out[NV] = out[0] / out[1]
template <int NV, int NS, bool MEAN>
__global__ __launch_bounds__(kPrjBlock) void prj_fold_k(const double *__restrict__ part, int nb,
                                                        double *__restrict__ out) {
  __shared__ double sh[NV][kPrjBlock];
  const int t = threadIdx.x;
  ndsm::block_final<NV, NS>(sh, part, nb, kPrjVals);
  if (t < NV) out[t] = sh[t][0];
  if (MEAN && t == 0) out[NV] = sh[0][0] / sh[1][0];
}

// rhs -= c, c read from the device (the fold's result)
__global__ __launch_bounds__(kPrjBlock) void sub_mean_k(double *__restrict__ rhs, size_t n,
                                                        const double *__restrict__ cm) {
  const double c = *cm;
  for (size_t q = (size_t)blockIdx.x * kPrjBlock + threadIdx.x; q < n; q += (size_t)gridDim.x * kPrjBlock)
    rhs[q] = rhs[q] - c;
}

struct PrjScratch {
  double *d_part = nullptr;   // [kPrjMaxBlocks * kPrjVals + kPrjRes]: block partials, then the results
  double *h_pin = nullptr;    // [kPrjRes] pinned
};
PrjScratch g_prj;

void prj_release() {
  if (g_prj.d_part) (void)hipFree(g_prj.d_part);
  if (g_prj.h_pin) (void)hipHostFree(g_prj.h_pin);
  g_prj = PrjScratch();
}

int prj_scratch() {
  if (!g_prj.d_part) {
    ndsm::at_reset(prj_release);
    NDSM_HIP(hipMalloc((void **)&g_prj.d_part, sizeof(double) * (kPrjMaxBlocks * kPrjVals + kPrjRes)));
    NDSM_HIP(hipHostMalloc((void **)&g_prj.h_pin, sizeof(double) * kPrjRes, hipHostMallocDefault));
  }
  return 0;
}

double *prj_res() { return g_prj.d_part + (size_t)kPrjMaxBlocks * kPrjVals; }

}  // namespace

// rhs = div_h B - c, c = sum w div_h B / sum w (left on the device for ndsmk_project_div_max).  B (nx,ny,nz,3),
// rhs (nx,ny,nz): DEVICE arrays.  Asynchronous.
extern "C" int ndsmk_project_div_rhs(const double *B, double *rhs, const int32_t *n3, const double *h_dq3) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B && rhs && n3[0] >= 3 && n3[1] >= 3 && n3[2] >= 3);
  const int rc = prj_scratch();
  if (rc != 0) return rc;
  const PrjArgs p = prj_args(n3, h_dq3);
  const int nb = prj_blocks(p);
  const size_t N = p.nrows * (size_t)n3[0];
  const size_t nsub = (N + kPrjBlock - 1) / kPrjBlock;
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(div_part_k<true>, dim3(nb), dim3(kPrjBlock), 0, s, B, rhs, g_prj.d_part, p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL((prj_fold_k<3, 2, true>), dim3(1), dim3(kPrjBlock), 0, s, g_prj.d_part, nb, prj_res());
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(sub_mean_k, dim3((unsigned)(nsub < 8192 ? nsub : 8192)), dim3(kPrjBlock), 0, s, rhs, N,
                     prj_res() + 3);
  NDSM_LAUNCH_CHECK();
  return 0;
}

// B -= G_h phi (normal component on the end planes of its axis untouched), sum w |G_h phi|^2 left on the device.
// B (nx,ny,nz,3), phi (nx,ny,nz): DEVICE arrays.  Asynchronous.
extern "C" int ndsmk_project_grad_sub(double *B, const double *phi, const int32_t *n3, const double *h_dq3) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B && phi && n3[0] >= 3 && n3[1] >= 3 && n3[2] >= 3);
  const int rc = prj_scratch();
  if (rc != 0) return rc;
  const PrjArgs p = prj_args(n3, h_dq3);
  const int nb = prj_blocks(p);
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(grad_sub_k, dim3(nb), dim3(kPrjBlock), 0, s, B, phi, g_prj.d_part, p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL((prj_fold_k<1, 1, false>), dim3(1), dim3(kPrjBlock), 0, s, g_prj.d_part, nb, prj_res() + 4);
  NDSM_LAUNCH_CHECK();
  return 0;
}

// Blocking.  max |div_h B| of the projected field, then the results of the three passes to the host:
//   h_out4[0] c = sum w div_h B / sum w   [1] max |div_h B| before   [2] max |div_h B'|   [3] 1/2 sum w |G_h phi|^2
extern "C" int ndsmk_project_div_max(const double *B, const int32_t *n3, const double *h_dq3, double *h_out4) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B && h_out4 && n3[0] >= 3 && n3[1] >= 3 && n3[2] >= 3);
  const int rc = prj_scratch();
  if (rc != 0) return rc;
  const PrjArgs p = prj_args(n3, h_dq3);
  const int nb = prj_blocks(p);
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(div_part_k<false>, dim3(nb), dim3(kPrjBlock), 0, s, B, nullptr, g_prj.d_part, p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL((prj_fold_k<3, 2, false>), dim3(1), dim3(kPrjBlock), 0, s, g_prj.d_part, nb, prj_res() + 5);
  NDSM_LAUNCH_CHECK();
  NDSM_HIP(hipMemcpyAsync(g_prj.h_pin, prj_res(), kPrjRes * sizeof(double), hipMemcpyDeviceToHost, s));
  NDSM_HIP(hipStreamSynchronize(s));
  const double *v = g_prj.h_pin;
  h_out4[0] = v[3];
  h_out4[1] = v[2];
  h_out4[2] = v[7];
  h_out4[3] = 0.5 * v[4];
  return 0;
}
