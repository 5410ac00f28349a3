// Magnetic dips and bald patches of a field on the device (DESIGN.md "Dips and bald patches"): the mesh edges on which
// B_z changes sign with (B.grad)B_z > 0 at the crossing.  The semantics - the nodal gradient, the crossing rule, the
// interpolation, the record and every operand order - are written out in include/ndsm_hip.h (ndsm_hip_vecpot_dips) and
// restated in numpy by tests/dips_model.py bit for bit (-ffp-contract=off).  Here:
//
//   vote    dip_vote_k   one lane per node, its up to three edges (+x, +y, +z): B_z at the node and at the three
//                        neighbours - each value comes from HBM once, the neighbours' reads hit the caches -, and only
//                        on a crossing B_x, B_y and the 14 more B_z of the two nodal gradients.  One ballot word per
//                        wave and family, and per workgroup the numbers of dips, crossings and bald patches
//   order   dip_sum_k    the totals of the crossings and of the bald patches (sums alone: nothing is placed by them)
//           scan64_k     exclusive sums of the workgroups' dips and their total; one blocking read of the three totals
//   fill    dip_fill_k   the lanes with a set bit repeat dip_edge - the same expressions, so the same bits - and write
//                        their records at rank = the number of set bits before theirs in edge order, while
//                        rank < max_dips
// Nothing is appended atomically and nothing is sorted: edge = 3 node + d ascends with the lane and, within a lane,
// with the family, so the rank is a count of bits.  plane_only launches over the nodes of k = 0 and the families x, y.
#include "diffq.hpp"
#include "scan64.hpp"

namespace {

using namespace ndsm;

constexpr int kDipBlock = 1024;                    // 16 waves, 48 mask words per workgroup
constexpr int kDipWaves = kDipBlock / kWave;

typedef unsigned long long u64;

struct DipArgs {
  size_t N, sy, sz;      // nodes of the mesh, strides of y and z
  size_t M;              // nodes looked at: N, or nx ny with plane_only
  int n[3];
  int nfam;              // families looked at: 3, or 2 with plane_only
  double lo[3], h[3];
};

// what a crossing's record holds besides its name
struct DipRec {
  double posd;           // the position along the edge's own axis
  double b[3], g[3], curv;
};

struct DipOut {
  long long *edge;
  double *pos, *bpt, *grad, *curv;
  int32_t *flag;
};

// node t -> (i, j, k) (32-bit divisions where they suffice)
__device__ __forceinline__ void dip_node(const DipArgs &p, size_t t, int q[3]) {
  if (p.N <= (size_t)0xffffffffu) {
    const unsigned r = (unsigned)t / (unsigned)p.n[0];
    q[0] = (int)((unsigned)t - r * (unsigned)p.n[0]);
    const unsigned k = r / (unsigned)p.n[1];
    q[1] = (int)(r - k * (unsigned)p.n[1]);
    q[2] = (int)k;
  } else {
    const size_t r = t / (size_t)p.n[0];
    q[0] = (int)(t - r * (size_t)p.n[0]);
    const size_t k = r / (size_t)p.n[1];
    q[1] = (int)(r - k * (size_t)p.n[1]);
    q[2] = (int)k;
  }
}

__device__ __forceinline__ size_t dip_stride(const DipArgs &p, int d) { return d == 0 ? (size_t)1 : (d == 1 ? p.sy : p.sz); }

// The edge of family d at node c = (q[0], q[1], q[2]), a = B_z there.  cross: it is there and B_z changes sign on it;
// returns whether it is a dip, with r filled on every crossing.
template <int d>
__device__ __forceinline__ bool dip_edge(const double *__restrict__ B, const DipArgs &p, size_t c, const int q[3],
                                         double a, bool &cross, DipRec &r) {
  cross = false;
  if (q[d] + 1 >= p.n[d]) return false;
  const double *__restrict__ bz = B + 2 * p.N;
  const size_t c2 = c + dip_stride(p, d);
  const double b = bz[c2];
  cross = (a > 0.0) != (b > 0.0);
  if (!cross) return false;
  const double t = a / (a - b);
  int q2[3] = {q[0], q[1], q[2]};
  q2[d] += 1;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const double g0 = ddq(bz, c, q[m], p.n[m], dip_stride(p, m), p.h[m]);
    const double g1 = ddq(bz, c2, q2[m], p.n[m], dip_stride(p, m), p.h[m]);
    r.g[m] = g0 + t * (g1 - g0);
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const double v0 = B[m * p.N + c], v1 = B[m * p.N + c2];
    r.b[m] = v0 + t * (v1 - v0);
  }
  r.b[2] = a + t * (b - a);
  r.posd = p.lo[d] + ((double)q[d] + t) * p.h[d];
  r.curv = r.b[0] * r.g[0] + r.b[1] * r.g[1];
  return r.curv > 0.0;
}

// words: 3 per wave (families x, y, z); cnt: three runs of ng + 1 int64 - the dips, the crossings and the bald
// patches of every workgroup, each run with one more slot for its total
__global__ __launch_bounds__(kDipBlock) void dip_vote_k(const double *__restrict__ B, DipArgs p, u64 *__restrict__ words,
                                                        i64 *__restrict__ cnt, size_t ng) {
  __shared__ unsigned wc[kDipWaves][3];
  const size_t t = (size_t)blockIdx.x * kDipBlock + threadIdx.x;
  bool dip[3] = {false, false, false}, cross[3] = {false, false, false};
  bool low = false;
  if (t < p.M) {
    int q[3];
    dip_node(p, t, q);
    low = q[2] == 0;
    const double a = B[2 * p.N + t];
    DipRec r;
    dip[0] = dip_edge<0>(B, p, t, q, a, cross[0], r);
    dip[1] = dip_edge<1>(B, p, t, q, a, cross[1], r);
    if (p.nfam == 3) dip[2] = dip_edge<2>(B, p, t, q, a, cross[2], r);
  }
  unsigned nd = 0, nc = 0, nb = 0;
  u64 w[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    w[d] = __ballot(dip[d]);
    nd += (unsigned)__popcll(w[d]);
    nc += (unsigned)__popcll(__ballot(cross[d]));
    if (d < 2) nb += (unsigned)__popcll(__ballot(dip[d] && low));
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    const size_t wv = t >> 6;
    words[3 * wv] = w[0];
    words[3 * wv + 1] = w[1];
    words[3 * wv + 2] = w[2];
    wc[threadIdx.x >> 6][0] = nd;
    wc[threadIdx.x >> 6][1] = nc;
    wc[threadIdx.x >> 6][2] = nb;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned s = 0;
#pragma unroll
    for (int i = 0; i < kDipWaves; ++i) s += wc[i][threadIdx.x];
    cnt[threadIdx.x * (ng + 1) + blockIdx.x] = (i64)s;
  }
}

// the crossings' and the bald patches' runs of cnt need no offsets, only their totals: slot ng of each run <- the sum
// of its ng counts.  One workgroup, strided reads, a tree in LDS.
__global__ __launch_bounds__(kScanBlock) void dip_sum_k(i64 *__restrict__ cnt, size_t ng) {
  __shared__ i64 part[2][kScanBlock];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const i64 *__restrict__ a = cnt + (size_t)(c + 1) * (ng + 1);
    i64 s = 0;
    for (size_t q = threadIdx.x; q < ng; q += kScanBlock) s += a[q];
    part[c][threadIdx.x] = s;
  }
  __syncthreads();
  for (int d = kScanBlock / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) {
      part[0][threadIdx.x] += part[0][threadIdx.x + d];
      part[1][threadIdx.x] += part[1][threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x < 2) cnt[(size_t)(threadIdx.x + 1) * (ng + 1) + ng] = part[threadIdx.x][0];
}

template <int d>
__device__ __forceinline__ void dip_emit(const double *__restrict__ B, const DipArgs &p, size_t c, const int q[3], double a,
                                         size_t rank, const DipOut &o) {
  bool cross;
  DipRec r;
  (void)dip_edge<d>(B, p, c, q, a, cross, r);
  o.edge[rank] = (long long)(3 * c + d);
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    o.pos[3 * rank + m] = m == d ? r.posd : p.lo[m] + (double)q[m] * p.h[m];
    o.bpt[3 * rank + m] = r.b[m];
    o.grad[3 * rank + m] = r.g[m];
  }
  o.curv[rank] = r.curv;
  o.flag[rank] = (q[2] == 0 && d != 2) ? 1 : 0;
}

// offs: the exclusive sums of the workgroups' dips
__global__ __launch_bounds__(kDipBlock) void dip_fill_k(const double *__restrict__ B, DipArgs p,
                                                        const u64 *__restrict__ words, const i64 *__restrict__ offs,
                                                        size_t limit, DipOut o) {
  size_t rank = (size_t)offs[blockIdx.x];
  if (rank >= limit) return;
  const size_t t = (size_t)blockIdx.x * kDipBlock + threadIdx.x;
  const size_t wv = t >> 6;
  const int lane = (int)(threadIdx.x & (kWave - 1));
  const u64 w0 = words[3 * wv], w1 = words[3 * wv + 1], w2 = words[3 * wv + 2];
  const unsigned mine = (unsigned)((w0 >> lane) & 1ull) | ((unsigned)((w1 >> lane) & 1ull) << 1) |
                        ((unsigned)((w2 >> lane) & 1ull) << 2);
  if (mine == 0u) return;               // (no bit is set past the last node)
  for (size_t ww = (size_t)blockIdx.x * kDipWaves; ww < wv; ++ww)
    rank += (size_t)(__popcll(words[3 * ww]) + __popcll(words[3 * ww + 1]) + __popcll(words[3 * ww + 2]));
  const u64 below = (1ull << lane) - 1ull;
  rank += (size_t)(__popcll(w0 & below) + __popcll(w1 & below) + __popcll(w2 & below));
  int q[3];
  dip_node(p, t, q);
  const double a = B[2 * p.N + t];
  if (mine & 1u) {
    if (rank >= limit) return;
    dip_emit<0>(B, p, t, q, a, rank, o);
    ++rank;
  }
  if (mine & 2u) {
    if (rank >= limit) return;
    dip_emit<1>(B, p, t, q, a, rank, o);
    ++rank;
  }
  if (mine & 4u) {
    if (rank >= limit) return;
    dip_emit<2>(B, p, t, q, a, rank, o);
  }
}

// scratch of the call, kept between calls and grown on demand (no result depends on its size): the mask words and the
// three runs of counts; three pinned totals
struct DipScratch {
  void *a = nullptr;
  size_t cap = 0;
  long long *h_pin = nullptr;
  bool registered = false;     // dip_release is queued for the next reset
};
DipScratch g_dip;

void dip_release() {
  if (g_dip.a) (void)hipFree(g_dip.a);
  if (g_dip.h_pin) (void)hipHostFree(g_dip.h_pin);
  g_dip = DipScratch();
}

int dip_grow(size_t bytes) {
  if (!g_dip.registered) {
    ndsm::at_reset(dip_release);
    g_dip.registered = true;
  }
  if (!g_dip.h_pin) NDSM_HIP(hipHostMalloc((void **)&g_dip.h_pin, 3 * sizeof(long long), hipHostMallocDefault));
  if (bytes <= g_dip.cap) return 0;
  if (g_dip.a) {
    const int rc = ndsmk_free(g_dip.a);      // (drains the streams first)
    g_dip.a = nullptr;
    g_dip.cap = 0;
    if (rc != 0) return rc;
  }
  const int rc = ndsmk_alloc(&g_dip.a, bytes);
  if (rc != 0) return rc;
  g_dip.cap = bytes;
  return 0;
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

// Dips of B (nx,ny,nz,3), a DEVICE array.  lo3, h_dq3: the mesh's first point and spacing per axis.  h_counts3 (HOST):
// crossings, dips, bald patches.  The first min(dips, max_dips) records in ascending edge order go into the DEVICE arrays
// edge (int64), pos, bpt, grad (3 each), curv, flag (int32) (not looked at with max_dips == 0).  Blocks for the three
// counts; the records are written asynchronously.
extern "C" int ndsmk_dips(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, int plane_only,
                          int64_t max_dips, int64_t *h_counts3, int64_t *edge, double *pos, double *bpt, double *grad,
                          double *curv, int32_t *flag) {
  NDSM_REQUIRE_READY();
  if (h_counts3) h_counts3[0] = h_counts3[1] = h_counts3[2] = 0;
  if (max_dips < 0) return fail(NDSMK_EVALUE, "dips: max_dips >= 0", __FILE__, __LINE__);
  if (plane_only != 0 && plane_only != 1) return fail(NDSMK_EVALUE, "dips: plane_only is 0 or 1", __FILE__, __LINE__);
  NDSM_CHECK_ARG(B && h_counts3 && n3 && lo3 && h_dq3 && (max_dips == 0 || (edge && pos && bpt && grad && curv && flag)));
  if (n3[0] < 3 || n3[1] < 3 || n3[2] < 3)
    return fail(NDSMK_EVALUE, "dips: at least 3 nodes on every axis", __FILE__, __LINE__);
  NDSM_CHECK_ARG(h_dq3[0] > 0.0 && h_dq3[1] > 0.0 && h_dq3[2] > 0.0);
  DipArgs p;
  for (int d = 0; d < 3; ++d) {
    p.n[d] = n3[d];
    p.lo[d] = lo3[d];
    p.h[d] = h_dq3[d];
  }
  p.sy = (size_t)n3[0];
  p.sz = p.sy * (size_t)n3[1];
  p.N = p.sz * (size_t)n3[2];
  p.M = plane_only ? p.sz : p.N;
  p.nfam = plane_only ? 2 : 3;
  const size_t ng = (p.M + kDipBlock - 1) / kDipBlock;
  NDSM_CHECK_ARG(ng <= (size_t)0x7fffffff);

  const size_t b_words = up256(ng * kDipWaves * 3 * sizeof(u64)), b_cnt = up256(3 * (ng + 1) * sizeof(i64));
  int rc = dip_grow(b_words + b_cnt);
  if (rc != 0) return rc;
  u64 *words = (u64 *)g_dip.a;
  i64 *cnt = (i64 *)((uint8_t *)g_dip.a + b_words);
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(dip_vote_k, dim3((unsigned)ng), dim3(kDipBlock), 0, s, B, p, words, cnt, ng);
  NDSM_LAUNCH_CHECK();
  // the crossings' and the bald patches' totals are queued first; the dips' scan brings all three home
  hipLaunchKernelGGL(dip_sum_k, dim3(1), dim3(kScanBlock), 0, s, cnt, ng);
  NDSM_LAUNCH_CHECK();
  for (int c = 1; c < 3; ++c)
    NDSM_HIP(hipMemcpyAsync(g_dip.h_pin + c, cnt + c * (ng + 1) + ng, sizeof(long long), hipMemcpyDeviceToHost, s));
  rc = scan64_total((int64_t *)cnt, ng, (int64_t *)g_dip.h_pin, s);
  if (rc != 0) return rc;
  const long long ndips = g_dip.h_pin[0];
  h_counts3[0] = g_dip.h_pin[1];
  h_counts3[1] = ndips;
  h_counts3[2] = g_dip.h_pin[2];
  const size_t limit = (unsigned long long)max_dips < (unsigned long long)ndips ? (size_t)max_dips : (size_t)ndips;
  if (limit == 0) return 0;
  const DipOut o = {(long long *)edge, pos, bpt, grad, curv, flag};
  hipLaunchKernelGGL(dip_fill_k, dim3((unsigned)ng), dim3(kDipBlock), 0, s, B, p, words, cnt, limit, o);
  NDSM_LAUNCH_CHECK();
  return 0;
}
