// Block-resident red-black Gauss-Seidel smoother for the 3-D levels above the single-workgroup
// kernels (<= 4096 points) and far below the z-streaming fused kernel (>= 2 M points): plan::relax_plan
// (relax_plan.hpp) sends levels of up to 512 K points here, the measured cut-over against the colour passes.
//
// There a colour pass (rbgs3_color) is shorter than the gap between two dependent launches, so a
// sweep costs two dispatch latencies whatever the level holds.  Here ONE launch performs S = 1 or 2
// full sweeps (2 S colour half-steps), out of place (u -> uout):
//   * a workgroup owns a block of BX x BY x BZ points and loads it with a ring of R = 2 S points
//     into static LDS (S = 2, 16 x 8 x 8: 24 x 16 x 16 doubles = 48 KB; 1024 threads, up to two workgroups per CU);
//     the ring is re-read from L2 by the neighbouring blocks - the level is cache resident, so the
//     redundant reads are cheap and the saved launches are not;
//   * half-step h updates colour (first_par + h) & 1 on the loaded region shrunk by h + 1 rings
//     (and inside lb..ub); one workgroup barrier per half-step; after the last one exactly the owned
//     block is valid.  Towards a domain face there is no ring and nothing shrinks: the mirrored
//     neighbour lies inside the block;
//   * every owned point is stored, updated or not: the partner array holds stale values, and the
//     Dirichlet data must arrive there too.
// The colouring and the update expression are rbgs3_color's (smooth.hip), operand for operand, and
// the file is compiled without contraction like the other smoothers: same bits.
// The right-hand side is read from L2 once per launch and point into registers (a thread updates
// the same points in every half-step of a colour); the LDS goes to u.
#include <cstdlib>
#include <cstring>

#include "common.hpp"

namespace {

constexpr int kNT = 1024;       // threads per workgroup: the launch is bound by dependent latency, not by registers or LDS
constexpr int kFar = 15;        // "no ring on this side": deeper than any half-step shrinks

template <int S, int BX, int BY, int BZ>
__global__ __launch_bounds__(kNT) void rbgs3_block_k(const double *__restrict__ u, double *__restrict__ uout,
                                                     const double *__restrict__ rhs, ndsmk_grid g) {
  constexpr int R = 2 * S;
  constexpr int LX = BX + 2 * R, LY = BY + 2 * R, LZ = BZ + 2 * R;
  constexpr int NL = LX * LY * LZ;                    // points of the loaded region
  constexpr int HX = LX / 2;                          // x-adjacent pairs in a row of the loaded region
  constexpr int NSLOT = HX * LY * LZ;
  constexpr int NIT = (NSLOT + kNT - 1) / kNT;        // pairs per thread: one point of either colour each
  constexpr int NLD = (NL + kNT - 1) / kNT;
  static_assert(LX % 2 == 0 && NL * 8 < 65536, "tile does not fit");
  __shared__ double t[NL];
  const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
  const int tid = threadIdx.x;
  // global coordinates of local point (0, 0, 0) - negative where the ring would cross a low face
  const int ox = (int)blockIdx.x * BX - R, oy = (int)blockIdx.y * BY - R, oz = (int)blockIdx.z * BZ - R;
  auto at = [&](int i, int j, int k) { return (size_t)i + (size_t)nx * ((size_t)j + (size_t)ny * (size_t)k); };

  // the loaded region: requested first, written to LDS after the index work below (which does not depend on it)
  double v[NLD];
#pragma unroll
  for (int q = 0; q < NLD; ++q) {
    const int p = tid + kNT * q;
    const int i = ox + p % LX, j = oy + (p / LX) % LY, k = oz + p / (LX * LY);
    v[q] = (p < NL && i >= 0 && i < nx && j >= 0 && j < ny && k >= 0 && k < nz) ? u[at(i, j, k)] : 0.0;
  }

  // rings between point c and the edge of the loaded region [o, o + L) along one axis; a face is no edge
  auto depth = [](int c, int o, int L, int n) {
    const int lo = o <= 0 ? kFar : c - o;
    const int hi = o + L - 1 >= n - 1 ? kFar : o + L - 1 - c;
    return lo < hi ? lo : hi;
  };
  // A thread's points are fixed for the launch: of each of its pairs (2 t, 2 t + 1) in a row (j, k) one point has
  // the colour of the even half-steps (c = 0: first_par) and one that of the odd ones.  Per c and pair:
  //   code = local index | depth << 16 | mirror flags << 20   (-1: no point, or never updated)
  //   rr   = its right-hand side
  // The colour of a point is rbgs3_color's: i = lb0 + (((lb0 + j + k) & 1) != par) + 2 t, i.e. (i + j + k) & 1 == par.
  int code[2][NIT];
  double rr[2][NIT];
#pragma unroll
  for (int q = 0; q < NIT; ++q) {
    const int p = tid + kNT * q;
    const int jl = (p / HX) % LY, kl = p / (HX * LY);
    const int j = oy + jl, k = oz + kl;
    const bool row = p < NSLOT && j >= g.lb[1] && j <= g.ub[1] && k >= g.lb[2] && k <= g.ub[2];
    const int dy = depth(j, oy, LY, ny), dz = depth(k, oz, LZ, nz);
    const int dyz = dy < dz ? dy : dz;
    // mirrored ghosts: xl < 0 -> 1, xh > nx - 1 -> nx - 2, likewise in y and z
    const int fyz = (j == 0 ? 4 : 0) | (j == ny - 1 ? 8 : 0) | (k == 0 ? 16 : 0) | (k == nz - 1 ? 32 : 0);
    const int first = (g.first_par + j + k + ox) & 1;   // which element of the pair has colour first_par
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int il = 2 * (p % HX) + (first ^ c);
      const int i = ox + il;
      const int dx = depth(i, ox, LX, nx);
      const int d = dx < dyz ? dx : dyz;
      // inside the update bounds, and inside the region of this colour's first half-step at least
      const bool ok = row && i >= g.lb[0] && i <= g.ub[0] && d >= c + 1;
      const int fl = fyz | (i == 0 ? 1 : 0) | (i == nx - 1 ? 2 : 0);
      code[c][q] = ok ? ((il + LX * (jl + LY * kl)) | (d << 16) | (fl << 20)) : -1;
      rr[c][q] = (ok && rhs) ? rhs[at(i, j, k)] : 0.0;   // rhs == nullptr: identically zero
    }
  }
#pragma unroll
  for (int q = 0; q < NLD; ++q) {
    const int p = tid + kNT * q;
    if (p < NL) t[p] = v[q];
  }
  __syncthreads();

#pragma unroll
  for (int h = 0; h < 2 * S; ++h) {
#pragma unroll
    for (int q = 0; q < NIT; ++q) {
      const int cd = code[h & 1][q];
      if (cd >= 0 && ((cd >> 16) & 15) >= h + 1) {
        const int p = cd & 0xffff;
        const int xl = (cd & (1 << 20)) ? p + 1 : p - 1, xh = (cd & (2 << 20)) ? p - 1 : p + 1;
        const int yl = (cd & (4 << 20)) ? p + LX : p - LX, yh = (cd & (8 << 20)) ? p - LX : p + LX;
        const int zl = (cd & (16 << 20)) ? p + LX * LY : p - LX * LY, zh = (cd & (32 << 20)) ? p - LX * LY : p + LX * LY;
        const double unew = (t[xh] + t[xl]) * g.w[0] + (t[yh] + t[yl]) * g.w[1] + (t[zh] + t[zl]) * g.w[2] - rr[h & 1][q];
        t[p] = g.w1 * unew;
      }
    }
    __syncthreads();
  }

  const int bx0 = ox + R, by0 = oy + R, bz0 = oz + R;
  for (int p = tid; p < BX * BY * BZ; p += kNT) {
    const int il = p % BX, jl = (p / BX) % BY, kl = p / (BX * BY);
    const int i = bx0 + il, j = by0 + jl, k = bz0 + kl;
    if (i < nx && j < ny && k < nz) uout[at(i, j, k)] = t[(il + R) + LX * ((jl + R) + LY * (kl + R))];
  }
}

template <int S, int BZ>
int launch_block(const ndsmk_grid &g, const double *u, double *uout, const double *rhs) {
  constexpr int BX = 16, BY = 8;
  const dim3 grid((g.n[0] + BX - 1) / BX, (g.n[1] + BY - 1) / BY, (g.n[2] + BZ - 1) / BZ);
  hipLaunchKernelGGL((rbgs3_block_k<S, BX, BY, BZ>), grid, dim3(kNT), 0, ndsm::stream(), u, uout, rhs, g);
  NDSM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

namespace ndsm {

// Development knob: NDSM_BLOCK_CFG=<bz>,<points> - <bz> 4 or 8 fixes the block height (0: by level size),
// <points> lets the block launch take levels below that many points BEFORE the fused launcher is asked
// (scripts/time_small_levels.py measures the cut-over that way).  Default 0,0.
const int64_t *block_cfg() {
  static int64_t cfg[2] = {-1, 0};
  if (cfg[0] < 0) {
    cfg[0] = 0;
    const char *e = std::getenv("NDSM_BLOCK_CFG");
    for (int i = 0; e && i < 2; ++i) {
      cfg[i] = std::atoll(e);
      e = std::strchr(e, ',');
      if (e) ++e;
    }
  }
  return cfg;
}

// NDSM_HIP_NO_BLOCK=1 (read once per process): relax keeps the colour passes on these levels - A/B runs
bool block_smoother_on() {
  static const bool on = std::getenv("NDSM_HIP_NO_BLOCK") == nullptr;
  return on;
}

// One block pass of a relax plan (relax_plan.hpp decides where it applies): `sweeps` = 1 or 2 sweeps u -> uout on a
// whole 3-D fp64 level in blocks of height bz
int launch_rbgs3_block(const ndsmk_grid &g, const double *u, double *uout, const double *rhs, int sweeps, int bz) {
  switch (10 * sweeps + bz) {
    case 24: return launch_block<2, 4>(g, u, uout, rhs);
    case 28: return launch_block<2, 8>(g, u, uout, rhs);
    case 14: return launch_block<1, 4>(g, u, uout, rhs);
    case 18: return launch_block<1, 8>(g, u, uout, rhs);
  }
  return fail(NDSMK_EARG, "block smoother: no such instantiation", __FILE__, __LINE__);
}

}  // namespace ndsm
