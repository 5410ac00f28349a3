// Red-black Gauss-Seidel smoother for the 7-point (3-D) / 5-point (2-D) Poisson
// stencil with mirrored-ghost Neumann faces and fixed Dirichlet faces.
//
// Reference semantics: ndsm_optimized.f90:40-191 (3-D), ndsm_poisson.f90:451-619
// (2-D, incl. the all-Neumann mean shift).  Operand order is kept and the file
// is compiled with -ffp-contract=off, so a sweep is bit-identical to the
// reference built by its own Makefile (no FMA contraction on x86-64).
//
// Bandwidth model: 24 B per lattice update = u read + rhs read +
// u write, once per full red+black sweep.
//   rbgs3_color   : two launches per sweep, half-line utilisation -> baseline
//                   and fallback for tiny / oddly shaped levels
//   rbgs3_fused   : one launch per sweep (see smooth_fused.hip)
//   rbgs3_block_k : two sweeps per launch on the cache-resident levels in between (see smooth_block.hip)
#include "common.hpp"
#include "relax_plan.hpp"

#include <cstdlib>

namespace ndsm {
void fused_metric_accumulate(bool on);
const int *fused_cfg();
const int64_t *block_cfg();
bool block_smoother_on();
int64_t fused_coarse_plane(const ndsmk_grid &g, const ndsmk_xfer *px);
int launch_rbgs3_fused(const plan::Pass &p, const ndsmk_grid &g, const double *u, double *uout, const double *rhs,
                       double *rout, const double *prev, const ndsmk_xfer *px, const double *uc);
int launch_rbgs3_block(const ndsmk_grid &g, const double *u, double *uout, const double *rhs, int sweeps, int bz);
int fetch_fused_metric(double *h_out2);
int launch_mean_shift(double *u, int64_t n);

// the development knobs as the planner takes them (the environment is read where each knob lives)
plan::Knobs relax_knobs() {
  plan::Knobs kn;
  for (int i = 0; i < 5; ++i) kn.fused[i] = fused_cfg()[i];
  kn.block[0] = block_cfg()[0];
  kn.block[1] = block_cfg()[1];
  kn.block_on = block_smoother_on();
  return kn;
}
}

namespace {

__device__ __forceinline__ size_t lin3(int i, int j, int k, int nx, int ny) {
  return (size_t)i + (size_t)nx * ((size_t)j + (size_t)ny * (size_t)k);
}

// One colour of one sweep.  Thread (tx, j, k) updates i = i0(j,k) + 2 tx, so a
// wave touches every second double of a row.
__global__ __launch_bounds__(256) void rbgs3_color(double *__restrict__ u, const double *__restrict__ rhs,
                                                  ndsmk_grid g, int par) {
  const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
  const int j = g.lb[1] + blockIdx.y * blockDim.y + threadIdx.y;
  const int k = g.lb[2] + blockIdx.z;
  if (j > g.ub[1]) return;
  const int kg = k + g.k0;  // global plane index keeps the colouring global under z-slabs
  const int i0 = g.lb[0] + ((((g.lb[0] + j + kg) & 1) != par) ? 1 : 0);
  const int i = i0 + 2 * (blockIdx.x * blockDim.x + threadIdx.x);
  if (i > g.ub[0]) return;
  int xl = i - 1, xh = i + 1, yl = j - 1, yh = j + 1, zl = k - 1, zh = k + 1;
  if (xl < 0) xl = 1;
  if (xh > nx - 1) xh = nx - 2;
  if (yl < 0) yl = 1;
  if (yh > ny - 1) yh = ny - 2;
  // physical z faces only: a slab's interior edges read the ghost planes k-1 / k+1
  if (kg - 1 < 0) zl = k + 1;
  if (kg + 1 > g.nzg - 1) zh = k - 1;
  (void)nz;
  const double unew = (u[lin3(xh, j, k, nx, ny)] + u[lin3(xl, j, k, nx, ny)]) * g.w[0] +
                      (u[lin3(i, yh, k, nx, ny)] + u[lin3(i, yl, k, nx, ny)]) * g.w[1] +
                      (u[lin3(i, j, zh, nx, ny)] + u[lin3(i, j, zl, nx, ny)]) * g.w[2] -
                      (rhs ? rhs[lin3(i, j, k, nx, ny)] : 0.0);  // rhs == nullptr: identically zero
  u[lin3(i, j, k, nx, ny)] = g.w1 * unew;
}

// Small 3-D levels (<= 16^3 points): all `nsweeps` sweeps in ONE launch of ONE
// workgroup.  The level is L2-resident and a colour pass is shorter than a kernel
// boundary, so two launches per sweep are pure launch latency; inside a single
// workgroup __syncthreads() orders the colour passes (global writes of a block are
// visible to the block after the barrier).  Same update expression as rbgs3_color.
__global__ __launch_bounds__(1024) void rbgs3_small(double *__restrict__ u_g, const double *__restrict__ rhs_g,
                                                    ndsmk_grid g, int nsweeps) {
  // the whole level (<= 4096 points) and its right-hand side sit in LDS for the duration
  __shared__ double u[4096], rhs[4096];
  const int nx = g.n[0], ny = g.n[1];
  const int n = nx * ny * g.n[2];
  for (int p = threadIdx.x; p < n; p += blockDim.x) {
    u[p] = u_g[p];
    rhs[p] = rhs_g ? rhs_g[p] : 0.0;
  }
  __syncthreads();
  const int mx = g.ub[0] - g.lb[0] + 1, my = g.ub[1] - g.lb[1] + 1, mz = g.ub[2] - g.lb[2] + 1;
  const int half = (mx + 1) / 2;
  const int total = half * my * mz;
  for (int sw = 0; sw < nsweeps; ++sw) {
    for (int pass = 0; pass < 2; ++pass) {
      const int par = (g.first_par + pass) & 1;
      for (int p = threadIdx.x; p < total; p += blockDim.x) {
        const int t = p % half, j = g.lb[1] + (p / half) % my, k = g.lb[2] + p / (half * my);
        const int i0 = g.lb[0] + ((((g.lb[0] + j + k) & 1) != par) ? 1 : 0);
        const int i = i0 + 2 * t;
        if (i > g.ub[0]) continue;
        int xl = i - 1, xh = i + 1, yl = j - 1, yh = j + 1, zl = k - 1, zh = k + 1;
        if (xl < 0) xl = 1;
        if (xh > nx - 1) xh = nx - 2;
        if (yl < 0) yl = 1;
        if (yh > ny - 1) yh = ny - 2;
        if (zl < 0) zl = 1;
        if (zh > g.n[2] - 1) zh = g.n[2] - 2;
        const double unew = (u[lin3(xh, j, k, nx, ny)] + u[lin3(xl, j, k, nx, ny)]) * g.w[0] +
                            (u[lin3(i, yh, k, nx, ny)] + u[lin3(i, yl, k, nx, ny)]) * g.w[1] +
                            (u[lin3(i, j, zh, nx, ny)] + u[lin3(i, j, zl, nx, ny)]) * g.w[2] -
                            rhs[lin3(i, j, k, nx, ny)];
        u[lin3(i, j, k, nx, ny)] = g.w1 * unew;
      }
      __syncthreads();
    }
  }
  for (int p = threadIdx.x; p < n; p += blockDim.x) u_g[p] = u[p];
}

// Small 2-D level (<= 4096 points): every sweep of a relax call - both colour passes and, on
// all-Neumann problems, the mean shift after each sweep (ndsm_poisson.f90:534-547) - in ONE
// single-workgroup launch.  The six face solves of the vector potential are pure dispatch
// latency on their coarse levels (5 of the 8 levels of a 512^2 face); this takes ~30 launches
// per level and V-cycle down to 3.  Same update expressions as rbgs2_color; the mean is a fixed
// tree over the workgroup (the reference's own sum is an unordered OpenMP reduction).
__global__ __launch_bounds__(1024) void rbgs2_small(double *__restrict__ u_g, const double *__restrict__ rhs_g,
                                                    ndsmk_grid g, int nsweeps) {
  __shared__ double u[4096], rhs[4096];  // the whole level in LDS
  __shared__ double red[16];
  const int nx = g.n[0], ny = g.n[1];
  const int n = nx * ny;
  for (int p = threadIdx.x; p < n; p += blockDim.x) {
    u[p] = u_g[p];
    rhs[p] = rhs_g ? rhs_g[p] : 0.0;
  }
  __syncthreads();
  const int mx = g.ub[0] - g.lb[0] + 1, my = g.ub[1] - g.lb[1] + 1;
  const int half = (mx + 1) / 2;
  const int total = half * my;
  for (int sw = 0; sw < nsweeps; ++sw) {
    for (int pass = 0; pass < 2; ++pass) {
      const int par = (g.first_par + pass) & 1;
      for (int p = threadIdx.x; p < total; p += blockDim.x) {
        const int t = p % half, j = g.lb[1] + p / half;
        const int i0 = g.lb[0] + ((((g.lb[0] + j) & 1) != par) ? 1 : 0);
        const int i = i0 + 2 * t;
        if (i > g.ub[0]) continue;
        const int xl = (i == 0) ? 1 : (i == nx - 1 ? nx - 2 : i - 1);
        const int xh = (i == 0) ? 1 : (i == nx - 1 ? nx - 2 : i + 1);
        const int yl = (j == 0) ? 1 : (j == ny - 1 ? ny - 2 : j - 1);
        const int yh = (j == 0) ? 1 : (j == ny - 1 ? ny - 2 : j + 1);
        double un = 0.0;  // ndsm_poisson.f90:603-617
        un = un + u[xl + nx * j] * g.w[0] + u[xh + nx * j] * g.w[0];
        un = un + u[i + nx * yl] * g.w[1] + u[i + nx * yh] * g.w[1];
        u[i + nx * j] = (un - rhs[i + nx * j]) * g.w1;
      }
      __syncthreads();
    }
    if (g.all_neumann) {
      double sm = 0.0;
      for (int p = threadIdx.x; p < n; p += blockDim.x) sm = sm + u[p];
      for (int o = 32; o > 0; o >>= 1) sm = sm + __shfl_down(sm, o, 64);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sm;
      __syncthreads();
      double tot = 0.0;
      for (int q = 0; q < 16; ++q) tot = tot + red[q];
      const double mean = tot / (double)n;
      for (int p = threadIdx.x; p < n; p += blockDim.x) u[p] = u[p] - mean;
      __syncthreads();
    }
  }
  for (int p = threadIdx.x; p < n; p += blockDim.x) u_g[p] = u[p];
}

// Mid-size 2-D level (4096 < points <= kMed2D, e.g. the 128^2 level of a 2-D face solve): the same
// single-workgroup scheme with only u in LDS (up to 152 KB, dynamic) and the right-hand side read
// from global memory (L2-resident: one 8-byte read per update).  A level of 16384 points otherwise
// costs ~5 launches per sweep (two colours, two-stage mean, subtraction), i.e. ~50 dispatch
// latencies per level visit; this is one.
using ndsm::plan::kMed2D;
__global__ __launch_bounds__(1024) void rbgs2_medium(double *__restrict__ u_g, const double *__restrict__ rhs_g,
                                                     ndsmk_grid g, int nsweeps) {
  extern __shared__ __attribute__((aligned(16))) double u[];  // the whole level
  __shared__ double red[16];
  constexpr int KQ = 8;   // points per thread and colour held in registers (128^2: exactly these; more: the loop below)
  const int nx = g.n[0], ny = g.n[1];
  const int n = nx * ny;
  for (int p = threadIdx.x; p < n; p += blockDim.x) u[p] = u_g[p];
  const int mx = g.ub[0] - g.lb[0] + 1, my = g.ub[1] - g.lb[1] + 1;
  const int half = (mx + 1) / 2;
  const int total = half * my;
  // one point of the colour pass `par`: ndsm_poisson.f90:603-617, mirror faces folded into the neighbour index
  auto update = [&](int i, int j, double r) {
    const int xl = (i == 0) ? 1 : (i == nx - 1 ? nx - 2 : i - 1);
    const int xh = (i == 0) ? 1 : (i == nx - 1 ? nx - 2 : i + 1);
    const int yl = (j == 0) ? 1 : (j == ny - 1 ? ny - 2 : j - 1);
    const int yh = (j == 0) ? 1 : (j == ny - 1 ? ny - 2 : j + 1);
    double un = 0.0;
    un = un + u[xl + nx * j] * g.w[0] + u[xh + nx * j] * g.w[0];
    un = un + u[i + nx * yl] * g.w[1] + u[i + nx * yh] * g.w[1];
    u[i + nx * j] = (un - r) * g.w1;
  };
  auto point_of = [&](int p, int par, int &i, int &j) {
    const int t = p % half;
    j = g.lb[1] + p / half;
    i = g.lb[0] + ((((g.lb[0] + j) & 1) != par) ? 1 : 0) + 2 * t;
    return p < total && i <= g.ub[0];
  };
  // A thread's first KQ points of either colour are fixed for the whole call: their coordinates (-1: none) and
  // right-hand side sit in registers - one integer division per point HERE instead of one per point and colour
  // pass, and no global load inside the sweeps (each was a dependent ~1 us L2 round trip in front of a pass that
  // has ~0.5 us of work).  Same expression per point: same bits.
  int pij[2][KQ];
  double rr[2][KQ];
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      int i, j;
      const bool have = point_of((int)threadIdx.x + 1024 * q, (g.first_par + pass) & 1, i, j);
      pij[pass][q] = have ? (i | (j << 16)) : -1;
      rr[pass][q] = (have && rhs_g) ? rhs_g[i + nx * j] : 0.0;
    }
  }
  __syncthreads();
  for (int sw = 0; sw < nsweeps; ++sw) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
        const int c = pij[pass][q];
        if (c >= 0) update(c & 0xffff, c >> 16, rr[pass][q]);
        if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // (four points' neighbour reads in flight at a time: registers)
      }
      for (int p = (int)threadIdx.x + 1024 * KQ; p < total; p += 1024) {   // (levels of more than 16384 points)
        int i, j;
        if (point_of(p, (g.first_par + pass) & 1, i, j)) update(i, j, rhs_g ? rhs_g[i + nx * j] : 0.0);
      }
      __syncthreads();
    }
    if (g.all_neumann) {
      double sm = 0.0;
#pragma unroll 8
      for (int p = threadIdx.x; p < n; p += 1024) sm = sm + u[p];   // (unrolled: the reads overlap, the additions keep their order)
      for (int o = 32; o > 0; o >>= 1) sm = sm + __shfl_down(sm, o, 64);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sm;
      __syncthreads();
      double tot = 0.0;
      for (int q = 0; q < 16; ++q) tot = tot + red[q];
      const double mean = tot / (double)n;
#pragma unroll 8
      for (int p = threadIdx.x; p < n; p += 1024) u[p] = u[p] - mean;
      __syncthreads();
    }
  }
  for (int p = threadIdx.x; p < n; p += blockDim.x) u_g[p] = u[p];
}

__global__ __launch_bounds__(256) void rbgs2_color(double *__restrict__ u, const double *__restrict__ rhs,
                                                  ndsmk_grid g, int par) {
  const int nx = g.n[0], ny = g.n[1];
  const int j = g.lb[1] + blockIdx.y * blockDim.y + threadIdx.y;
  if (j > g.ub[1]) return;
  const int i0 = g.lb[0] + ((((g.lb[0] + j) & 1) != par) ? 1 : 0);
  const int i = i0 + 2 * (blockIdx.x * blockDim.x + threadIdx.x);
  if (i > g.ub[0]) return;
  // stencil_stride (ndsm_poisson.f90:633-658): both neighbours collapse onto
  // the inner one at a boundary
  const int xl = (i == 0) ? 1 : (i == nx - 1 ? nx - 2 : i - 1);
  const int xh = (i == 0) ? 1 : (i == nx - 1 ? nx - 2 : i + 1);
  const int yl = (j == 0) ? 1 : (j == ny - 1 ? ny - 2 : j - 1);
  const int yh = (j == 0) ? 1 : (j == ny - 1 ? ny - 2 : j + 1);
  double un = 0.0;  // ndsm_poisson.f90:603-617
  un = un + u[(size_t)xl + (size_t)nx * j] * g.w[0] + u[(size_t)xh + (size_t)nx * j] * g.w[0];
  un = un + u[(size_t)i + (size_t)nx * yl] * g.w[1] + u[(size_t)i + (size_t)nx * yh] * g.w[1];
  u[(size_t)i + (size_t)nx * j] = (un - (rhs ? rhs[(size_t)i + (size_t)nx * j] : 0.0)) * g.w1;
}

}  // namespace


// the two colour passes of one sweep, in place
static int launch_color(const ndsmk_grid &g, double *u, const double *rhs) {
  const int half = (g.ub[0] - g.lb[0] + 2) / 2, my = g.ub[1] - g.lb[1] + 1;
  const dim3 block(64, 4, 1);
  const dim3 grid((half + 63) / 64, (my + 3) / 4, g.ndim == 3 ? g.ub[2] - g.lb[2] + 1 : 1);
  for (int pass = 0; pass < 2; ++pass) {
    if (g.ndim == 3)
      hipLaunchKernelGGL(rbgs3_color, grid, block, 0, ndsm::stream(), u, rhs, g, (g.first_par + pass) & 1);
    else
      hipLaunchKernelGGL(rbgs2_color, grid, block, 0, ndsm::stream(), u, rhs, g, (g.first_par + pass) & 1);
    NDSM_LAUNCH_CHECK();
  }
  return 0;
}

// The sweeps of one relax call, as plan::relax_plan (relax_plan.hpp; DESIGN.md "Which launch a relax call makes")
// lays them out.  bufs[0] holds u on entry; the out-of-place fused and block passes write to whichever of
// bufs[0..2] is neither the current one nor `keep` (bufs[2] may be null: plain ping-pong); *where tells which
// buffer holds the result.  keep: a buffer that must survive (the iterate the V-cycle started from, which the
// convergence metric is taken against); prev: evaluate that metric in the launch of the last sweep (*met_done).
// rout: residual on the last sweep (*res_done).  px / uc: u += P uc comes first (coarse_to_fine).
// src_zero: bufs[0] is zero but was never written (the first guess of a coarse level): the first launch takes the
// zeros from a descriptor of zero records where the plan says it can, otherwise they are written here first.
static int relax_impl(const ndsmk_grid *gp, double *const bufs[3], const double *keep, const double *rhs, int nsweeps,
                      int variant, int *where, double *rout, int *res_done, const double *prev, int *met_done,
                      const ndsmk_xfer *px = nullptr, const double *uc = nullptr, bool src_zero = false) {
  NDSM_REQUIRE_READY();
  const ndsmk_grid g = *gp;
  ndsm::plan::Request rq;
  rq.src_zero = src_zero;
  rq.nsweeps = nsweeps;
  rq.variant = variant;
  rq.rhs = rhs != nullptr;
  rq.want_res = rout != nullptr;
  rq.want_met = prev != nullptr;
  rq.corr = px != nullptr;
  if (px) rq.coarse_plane = ndsm::fused_coarse_plane(g, px);
  for (int c = 0; c < 3; ++c) {
    rq.have[c] = bufs[c] != nullptr;
    if (keep && bufs[c] == keep) rq.keep = c;
  }
  const ndsm::plan::Plan pl = ndsm::plan::relax_plan(g, rq, ndsm::relax_knobs());
  if (pl.err) return ndsm::fail(pl.err, pl.what, __FILE__, __LINE__);
  if (res_done) *res_done = pl.res_done;
  if (met_done) *met_done = pl.met_done;
  if (where) *where = pl.result;
  const int64_t npts = (int64_t)g.n[0] * g.n[1] * g.n[2];
  hipStream_t s = ndsm::stream();
  if (pl.materialise) NDSM_HIP(hipMemsetAsync(bufs[0], 0, sizeof(double) * (size_t)npts, s));
  if (pl.prolong_only) return ndsmk_prolong_add(px, uc, bufs[0]);
  for (const ndsm::plan::Pass &p : pl.pass) {
    double *u = bufs[p.src], *uout = bufs[p.dst];
    int rc = p.prolong_first ? ndsmk_prolong_add(px, uc, u) : 0;
    if (rc) return rc;
    switch (p.kind) {
      case ndsm::plan::SMALL3D:
        hipLaunchKernelGGL(rbgs3_small, dim3(1), dim3(1024), 0, s, u, rhs, g, p.sweeps);
        break;
      case ndsm::plan::SMALL2D:
        hipLaunchKernelGGL(rbgs2_small, dim3(1), dim3(1024), 0, s, u, rhs, g, p.sweeps);
        break;
      case ndsm::plan::MEDIUM2D: {
        static int attr_epoch = 0;
        if (ndsm::first_in_epoch(attr_epoch))
          NDSM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(rbgs2_medium), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kMed2D * (int)sizeof(double)));
        hipLaunchKernelGGL(rbgs2_medium, dim3(1), dim3(1024), (size_t)npts * sizeof(double), s, u, rhs, g, p.sweeps);
        break;
      }
      case ndsm::plan::FUSED: rc = ndsm::launch_rbgs3_fused(p, g, u, uout, rhs, rout, prev, px, uc); break;
      case ndsm::plan::BLOCK: rc = ndsm::launch_rbgs3_block(g, u, uout, rhs, p.sweeps, p.bz); break;
      default: rc = launch_color(g, u, rhs); break;
    }
    if (rc) return rc;
    NDSM_LAUNCH_CHECK();
    if (p.mean_shift) {
      rc = ndsm::launch_mean_shift(uout, npts);
      if (rc) return rc;
    }
  }
  if (pl.result != 0 && !where)   // caller cannot swap: bring the result home
    NDSM_HIP(hipMemcpyAsync(bufs[0], bufs[pl.result], sizeof(double) * (size_t)npts, hipMemcpyDeviceToDevice, s));
  return 0;
}

extern "C" int ndsmk_relax(const ndsmk_grid *gp, double *u, double *ualt, const double *rhs, int nsweeps,
                           int variant, int *result_in_alt) {
  double *const bufs[3] = {u, ualt, nullptr};
  return relax_impl(gp, bufs, nullptr, rhs, nsweeps, variant, result_in_alt, nullptr, nullptr, nullptr, nullptr);
}

// nsweeps sweeps followed by r = rhs - L u: where the fused kernel covers the level
// the residual is produced by the launch of the last sweep, otherwise by residual.hip.
// variant 2 (tests): the fused sweep+residual launch or an error.
extern "C" int ndsmk_relax_residual(const ndsmk_grid *gp, double *u, double *ualt, const double *rhs, double *r,
                                    int nsweeps, int variant, int *result_in_alt) {
  NDSM_CHECK_ARG(r != nullptr && result_in_alt != nullptr && (variant == 0 || variant == 2));
  int res_done = 0;
  double *const bufs[3] = {u, ualt, nullptr};
  int rc = relax_impl(gp, bufs, nullptr, rhs, nsweeps, variant, result_in_alt, r, &res_done, nullptr, nullptr);
  if (rc) return rc;
  if (!res_done) {
    if (variant == 2)
      return ndsm::fail(NDSMK_EARG, "fused sweep + residual does not cover this level", __FILE__, __LINE__);
    rc = ndsmk_residual(gp, *result_in_alt ? ualt : u, rhs, r);
  }
  return rc;
}

// The zero first guess of a coarse level (ndsm_kernels.h): on by default
static bool zero_guess_env() {
  static const bool on = std::getenv("NDSM_HIP_NO_ZERO_GUESS") == nullptr;
  return on;
}
static int g_zero_guess_off = 0;   // ndsmk_debug_zero_guess(0) switches it off at run time (tests: A/B in one process)

extern "C" int ndsmk_zero_guess_on(void) { return zero_guess_env() && !g_zero_guess_off ? 1 : 0; }

extern "C" int ndsmk_debug_zero_guess(int on) {
  g_zero_guess_off = on ? 0 : 1;
  return 0;
}

extern "C" int ndsmk_relax_zero_src(const ndsmk_grid *gp, double *u, double *ualt, const double *rhs, double *r,
                                    int nsweeps, int variant, int *result_in_alt) {
  NDSM_CHECK_ARG(result_in_alt != nullptr && (!r || variant == 0 || variant == 2));
  int res_done = 0;
  double *const bufs[3] = {u, ualt, nullptr};
  int rc = relax_impl(gp, bufs, nullptr, rhs, nsweeps, variant, result_in_alt, r, &res_done, nullptr, nullptr, nullptr,
                      nullptr, true);
  if (rc || !r) return rc;
  if (!res_done) {
    if (variant == 2)
      return ndsm::fail(NDSMK_EARG, "fused sweep + residual does not cover this level", __FILE__, __LINE__);
    rc = ndsmk_residual(gp, *result_in_alt ? ualt : u, rhs, r);
  }
  return rc;
}

extern "C" int ndsmk_relax_zero_src_ok(const ndsmk_grid *gp, int has_rhs, int nsweeps, int variant, int with_res) {
  if (!ndsmk_zero_guess_on()) return 0;
  ndsm::plan::Request rq;
  rq.src_zero = true;
  rq.nsweeps = nsweeps;
  rq.variant = variant;
  rq.rhs = has_rhs != 0;
  rq.want_res = with_res != 0;
  rq.have[1] = true;
  const ndsm::plan::Plan pl = ndsm::plan::relax_plan(*gp, rq, ndsm::relax_knobs());
  return !pl.err && !pl.materialise && !pl.pass.empty() && pl.pass[0].src_zero ? 1 : 0;
}

// The V-cycle driver's level-1 form of the two calls above: three buffers (u on entry, two
// spares), `keep` is never written (the iterate the cycle started from), *where = 0/1/2 says
// which buffer holds the result.  r != NULL: residual of the result (fused into the last sweep's
// launch where possible).  prev != NULL: the launch of the last sweep also evaluates
// max / sum |u_new - prev| (*met_done = 1; read it with ndsmk_fetch_fused_metric), if it can.
// px != NULL: u += P uc (the coarse-grid correction) comes before the sweeps.
extern "C" int ndsmk_relax3(const ndsmk_grid *gp, double *u, double *a, double *b, const double *keep,
                            const double *rhs, int nsweeps, double *r, const double *prev, int *where,
                            int *met_done, const ndsmk_xfer *px, const double *uc) {
  NDSM_CHECK_ARG(where != nullptr && met_done != nullptr && u && a);
  int res_done = 0;
  double *const bufs[3] = {u, a, b};
  int rc = relax_impl(gp, bufs, keep, rhs, nsweeps, 0, where, r, &res_done, prev, met_done, px, uc);
  if (rc) return rc;
  if (r && !res_done) rc = ndsmk_residual(gp, bufs[*where], rhs, r);
  return rc;
}

extern "C" int ndsmk_fetch_fused_metric(double *h_out2) {
  NDSM_REQUIRE_READY();
  return ndsm::fetch_fused_metric(h_out2);
}

// The one fused pass of a window [z0, z1) of g's owned planes, u -> uout: planned and launched
static int fused_window(const ndsmk_grid *gp, const double *u, double *uout, const double *rhs, int nsweeps, int z0,
                        int z1, double *rout, const double *prev, const ndsmk_xfer *px, const double *uc) {
  ndsmk_grid g = *gp;
  g.zown0 = z0;
  g.zown1 = z1;
  ndsm::plan::Request rq;
  rq.window = true;
  rq.nsweeps = nsweeps;
  rq.rhs = rhs != nullptr;
  rq.want_res = rout != nullptr;
  rq.want_met = prev != nullptr;
  rq.corr = px != nullptr;
  if (px) rq.coarse_plane = ndsm::fused_coarse_plane(g, px);
  rq.have[1] = uout != nullptr;
  const ndsm::plan::Plan pl = ndsm::plan::relax_plan(g, rq, ndsm::relax_knobs());
  if (pl.err) return ndsm::fail(pl.err, pl.what, __FILE__, __LINE__);
  return ndsm::launch_rbgs3_fused(pl.pass[0], g, u, uout, rhs, rout, prev, px, uc);
}

// One out-of-place fused pass (nsweeps = 1 or 2) over the owned planes [z0, z1) of a z-slab only:
// the pieces of a pass whose halo exchange overlaps its interior (ndsmh_world).  u is read
// (z0 - 2 nsweeps .. z1 + 2 nsweeps must be valid planes), uout written on [z0, z1).
// px != NULL: u + P uc is formed while the planes are loaded (the launch that starts the
// post-smoothing; uc holds coarse planes [px->c_k0, px->c_k0 + px->c_cnt), which must cover the
// brackets of the window's planes AND of the ghost planes the launch reads).  Returns NDSMK_EARG
// if that launch does not exist for this level (general rhs, one sweep): the caller then
// interpolates with the stand-alone kernel first.
// prev != NULL: the launch also evaluates max / sum of |u_new - prev| over the planes it stores
// (update_u's metric; read back with ndsmk_fetch_fused_metric).  accumulate != 0: added to what the
// previous such launch left on the device - the windows of one pass, the slabs of one process.
extern "C" int ndsmk_fused_window(const ndsmk_grid *gp, const double *u, double *uout, const double *rhs, int nsweeps,
                                  int z0, int z1, const ndsmk_xfer *px, const double *uc, const double *prev,
                                  int accumulate) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(gp->ndim == 3 && (nsweeps == 1 || nsweeps == 2) && z0 >= gp->zown0 && z1 <= gp->zown1 && z0 < z1);
  NDSM_CHECK_ARG((!px || uc) && !(px && prev));
  ndsm::fused_metric_accumulate(accumulate != 0);
  const int rc = fused_window(gp, u, uout, rhs, nsweeps, z0, z1, nullptr, prev, px, uc);
  ndsm::fused_metric_accumulate(false);
  return rc;
}

// The sweep + residual pass on a window of owned planes [z0, z1): ONE sweep u -> uout and r = rhs - L uout on the
// window (u must be valid on z0 - 3 .. z1 + 2).  For the pieces of the last pre-smoothing pass whose halo
// exchange overlaps its interior (ndsmh_world).
extern "C" int ndsmk_fused_window_res(const ndsmk_grid *gp, const double *u, double *uout, const double *rhs, double *rout,
                                      int z0, int z1) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(gp->ndim == 3 && rout && z0 >= gp->zown0 && z1 <= gp->zown1 && z0 < z1);
  return fused_window(gp, u, uout, rhs, 1, z0, z1, rout, nullptr, nullptr, nullptr);
}

// would the window pass of nsweeps sweeps over g's owned planes be a launch of that mode?
static int window_mode_ok(const ndsmk_grid *gp, bool rhs, int nsweeps, int mode) {
  ndsm::plan::Request rq;
  rq.window = true;
  rq.nsweeps = nsweeps;
  rq.rhs = rhs;
  rq.want_met = mode == ndsm::plan::MET;
  rq.corr = mode == ndsm::plan::CORR;
  rq.have[1] = true;
  const ndsm::plan::Plan pl = ndsm::plan::relax_plan(*gp, rq, ndsm::relax_knobs());
  return !pl.err && pl.pass[0].mode == mode ? 1 : 0;
}

// can ndsmk_fused_window(..., prev) evaluate the metric? (fp64 level off the all-Neumann path)
extern "C" int ndsmk_fused_metric_ok(const ndsmk_grid *gp) { return window_mode_ok(gp, true, 1, ndsm::plan::MET); }

// can ndsmk_fused_window(..., px, uc) interpolate while it loads? (one sweep, or two without a right-hand side; fp64)
extern "C" int ndsmk_fused_prolong_ok(const ndsmk_grid *gp, const double *rhs, int nsweeps) {
  return window_mode_ok(gp, rhs != nullptr, nsweeps, ndsm::plan::CORR);
}

// tests / tools: the plan of a relax call (what = 0) or the z chunking of a fused launch (what = 1), on the host - no
// device, no ndsmk_init.  include/ndsm_hip.h (ndsm_hip_debug_relax_plan) has the layouts of the four arrays.
extern "C" int ndsmk_debug_relax_plan(int what, const int32_t *grid, const int64_t *req, const int64_t *knobs, int cap,
                                      int32_t *out) {
  namespace pn = ndsm::plan;
  if (what == 1) {
    NDSM_CHECK_ARG(req && out && cap >= 2 && req[0] >= 1 && req[0] < (1 << 30) && req[1] >= 1 && req[1] < (1 << 30) &&
                   req[2] >= 1 && req[3] >= 1 && req[3] < (1 << 20));
    const pn::Chunks ch = pn::z_chunks((int)req[0], (int)req[1], req[2], (int)req[3], req[4] != 0, (int)req[5]);
    out[0] = ch.nzc;
    out[1] = ch.zc;
    return 0;
  }
  // what = 2: what = 0 with the zero-source field - req[12], a seventh head value and a tenth value per pass
  const bool zs = what == 2;
  const int nh = zs ? 7 : 6, nr = zs ? 10 : 9;
  NDSM_CHECK_ARG((what == 0 || zs) && grid && req && knobs && out && cap >= nh && req[0] < (1 << 16));
  ndsmk_grid g = {};
  g.ndim = grid[0];
  for (int d = 0; d < 3; ++d) g.n[d] = grid[1 + d], g.lb[d] = grid[4 + d], g.ub[d] = grid[7 + d];
  g.all_neumann = grid[10], g.k0 = grid[11], g.nzg = grid[12], g.zown0 = grid[13], g.zown1 = grid[14];
  pn::Request rq;
  rq.nsweeps = (int)req[0], rq.variant = (int)req[1], rq.window = req[2] != 0, rq.fp32 = req[3] != 0;
  rq.rhs = req[4] != 0, rq.want_res = req[5] != 0, rq.want_met = req[6] != 0, rq.corr = req[7] != 0;
  rq.coarse_plane = req[8], rq.have[1] = req[9] != 0, rq.have[2] = req[10] != 0, rq.keep = (int)req[11];
  if (zs) rq.src_zero = req[12] != 0;
  pn::Knobs kn;
  for (int i = 0; i < 5; ++i) kn.fused[i] = (int)knobs[i];
  kn.block[0] = knobs[5], kn.block[1] = knobs[6], kn.block_on = knobs[7] == 0;
  const pn::Plan pl = pn::relax_plan(g, rq, kn);
  const int32_t head[7] = {pl.err,      (int32_t)pl.pass.size(), pl.result,     pl.res_done,
                           pl.met_done, pl.prolong_only,         pl.materialise};
  for (int i = 0; i < nh; ++i) out[i] = head[i];
  NDSM_CHECK_ARG((size_t)cap >= nh + nr * pl.pass.size());
  for (const pn::Pass &p : pl.pass) {
    const int32_t row[10] = {p.kind, p.sweeps, p.mode, p.inst, p.bz, p.src, p.dst, p.prolong_first, p.mean_shift, p.src_zero};
    for (int i = 0; i < nr; ++i) out[nh + nr * (&p - pl.pass.data()) + i] = row[i];
  }
  return 0;
}
