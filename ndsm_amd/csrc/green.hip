// Green's-function sums of the half space above a magnetogram (DESIGN.md "Open-box potential field"; semantics:
// include/ndsm_hip.h, ndsm_hip_green_points): all-pairs sums of targets times magnetogram pixels.
//
//   pairs_k<Term> : the classic all-pairs form.  A block of 256 threads owns 256 targets, one per thread, with X, Y and
//             the term - what is per target, and the sums - in registers.  blockIdx.y is the slice of the pixels (the
//             order of the sum is a function of npix alone: NS = min(64, ceil(npix / 4096)) slices of
//             len = ceil(npix / NS) pixels).  The slice goes through LDS in tiles of 256 pixels: thread l stages pixel
//             p = tile + l as xs[p mod nsx], ys[p div nsx] and q = bz[p] c, and every lane then reads the same address
//             (a broadcast, no bank conflict) pixel after pixel, so the terms are added left to right.  The Term::nc
//             slice sums go to scratch (NS, nc, chunk).
//   fold_k  : one thread per target adds the slice sums in ascending order, starting from slice 0's, applies the rules
//             of the plane (w < 0: NaN; w == 0: Bz is the bilinear interpolation of bz; neither for ApTerm's two sums)
//             and writes the target's components where its generator says.
//
// The pair terms, each one add(dx, dy, q) in the header's operand order:
//   GreenTerm : the potential field, three sums; a pair costs one sqrt and one division.
//   LfffTerm  : the constant-alpha field (ndsm_hip_lfff_points), Chiu & Hilton's half-space solution, three sums.
//             sin(alpha w) and cos(alpha w) are per target; a pair costs one sqrt, four divisions and one sincos.
//   ApTerm    : the potential field's vector potential ON the plane (ndsm_hip_green_ap_points): targets (X, Y), two
//             sums, no square root - one division.
//
// Three target generators serve the two field terms: a point list (3,npts), the face nodes of a box mesh and all nodes
// of a box mesh; two more serve ApTerm: a point list (2,npts) and the source's own nodes.  Targets are processed in
// chunks of at most 262144, which keeps the scratch at 384 MiB or less; a target's sums depend on nothing but the
// target and the source, so the chunking and the generator leave no trace in the bits.
//
// Plain C++ under -ffp-contract=off with IEEE division and sqrt: the operand order of the header is the bits, and
// tests/green_model.py restates it.
#include "common.hpp"

#include <cmath>
#include <cstdio>

namespace {

using ndsm::i64;

constexpr int kBlock = 256;             // targets per block and pixels per LDS tile
constexpr i64 kChunk = 262144;          // targets per launch: 64 slices x 3 x 8 B x 262144 = 384 MiB of scratch
constexpr i64 kSliceMin = 4096;         // pixels per slice before the 64-slice cap
constexpr int kSliceCap = 64;

enum { GEN_POINTS = 0, GEN_FACES = 1, GEN_VOLUME = 2, GEN_POINTS2 = 3, GEN_PLANE = 4 };

struct Source {
  const double *xs, *ys, *bz;           // DEVICE
  int nsx, nsy;
  i64 npix, len;
  int nslices;
  double zs, c;
};

struct Targets {
  int gen;
  int nc;                               // components per target: 3, or 2 for the plane's vector potential
  i64 count;                            // all targets of the call
  const double *pts;                    // GEN_POINTS: (3,npts), GEN_POINTS2: (2,npts), DEVICE
  const double *x, *y, *z;              // the box mesh (GEN_PLANE: the source's xs and ys), DEVICE
  int nx, ny, nz;
};

// the node (i, j, k) of face target t: the k = 0 plane, the k = nz - 1 plane, then plane after plane the ring of the
// rows j = 0 and j = ny - 1 and the columns i = 0 and i = nx - 1 between them
__device__ __forceinline__ void face_node(const Targets &g, i64 t, int &i, int &j, int &k) {
  const i64 plane = (i64)g.nx * g.ny;
  if (t < 2 * plane) {
    k = t < plane ? 0 : g.nz - 1;
    const i64 r = t < plane ? t : t - plane;
    j = (int)(r / g.nx);
    i = (int)(r - (i64)j * g.nx);
    return;
  }
  const i64 ring = 2 * (i64)g.nx + 2 * (i64)(g.ny - 2);
  const i64 u = t - 2 * plane;
  const i64 kk = u / ring;
  i64 r = u - kk * ring;
  k = 1 + (int)kk;
  if (r < g.nx) {
    j = 0;
    i = (int)r;
  } else if (r < 2 * (i64)g.nx) {
    j = g.ny - 1;
    i = (int)(r - g.nx);
  } else {
    r -= 2 * (i64)g.nx;
    j = 1 + (int)(r / 2);
    i = (r & 1) ? g.nx - 1 : 0;
  }
}

// coordinates of target t and where its component c goes: out[at + c * stride]
__device__ __forceinline__ void target_of(const Targets &g, i64 t, double &X, double &Y, double &Z, size_t &at,
                                          size_t &stride) {
  if (g.gen == GEN_POINTS) {
    X = g.pts[3 * t];
    Y = g.pts[3 * t + 1];
    Z = g.pts[3 * t + 2];
    at = (size_t)(3 * t);
    stride = 1;
    return;
  }
  if (g.gen == GEN_POINTS2) {
    X = g.pts[2 * t];
    Y = g.pts[2 * t + 1];
    Z = 0.0;
    at = (size_t)(2 * t);
    stride = 1;
    return;
  }
  if (g.gen == GEN_PLANE) {
    const i64 jp = t / g.nx;
    X = g.x[t - jp * g.nx];
    Y = g.y[jp];
    Z = 0.0;
    at = (size_t)t;
    stride = (size_t)g.nx * (size_t)g.ny;
    return;
  }
  int i, j, k;
  const i64 plane = (i64)g.nx * g.ny;
  if (g.gen == GEN_FACES) {
    face_node(g, t, i, j, k);
  } else {
    k = (int)(t / plane);
    const i64 r = t - (i64)k * plane;
    j = (int)(r / g.nx);
    i = (int)(r - (i64)j * g.nx);
  }
  X = g.x[i];
  Y = g.y[j];
  Z = g.z[k];
  at = (size_t)i + (size_t)g.nx * (size_t)j + (size_t)plane * (size_t)k;
  stride = (size_t)plane * (size_t)g.nz;
}

// The pair terms.  Term(w, alpha) sets up what is per target (w = Z - zs), add(dx, dy, q) adds one pixel's term to the
// sums a[0 .. nc - 1]: q = bz c of the pixel, (dx, dy) from the pixel to the target.
struct GreenTerm {
  static constexpr int nc = 3;
  double w, ww, a[nc];
  __device__ __forceinline__ GreenTerm(double w_, double) : w(w_), ww(w_ * w_), a{0.0, 0.0, 0.0} {}
  __device__ __forceinline__ void add(double dx, double dy, double q) {
    const double r2 = (dx * dx + dy * dy) + ww;
    if (r2 > 0.0) {
      const double t = q / (r2 * sqrt(r2));
      a[0] = a[0] + dx * t;
      a[1] = a[1] + dy * t;
      a[2] = a[2] + w * t;
    }
  }
};

struct LfffTerm {
  static constexpr int nc = 3;
  double w, ww, alpha, sz, cz, a[nc];
  __device__ __forceinline__ LfffTerm(double w_, double alpha_)
      : w(w_), ww(w_ * w_), alpha(alpha_), sz(sin(alpha_ * w_)), cz(cos(alpha_ * w_)), a{0.0, 0.0, 0.0} {}
  __device__ __forceinline__ void add(double dx, double dy, double q) {
    const double R2 = dx * dx + dy * dy;
    const double r2 = R2 + ww;
    if (r2 > 0.0) {
      const double r = sqrt(r2);
      const double t = q / (r2 * r);
      const double ar = alpha * r;
      double sr, cr;
      sincos(ar, &sr, &cr);
      a[0] = a[0] + (dx * t) * cr;
      a[1] = a[1] + (dy * t) * cr;
      a[2] = a[2] + (w * t) * (cr + ar * sr);
      if (R2 > 0.0) {
        const double u = alpha * (q / R2);
        const double e = sz - (ww / r2) * sr;
        const double f = (w / r) * cr - cz;
        a[0] = a[0] + u * (dx * e + dy * f);
        a[1] = a[1] + u * (dy * e - dx * f);
      }
    }
  }
};

struct ApTerm {
  static constexpr int nc = 2;
  double a[nc];
  __device__ __forceinline__ ApTerm(double, double) : a{0.0, 0.0} {}
  __device__ __forceinline__ void add(double dx, double dy, double q) {
    const double r2 = dx * dx + dy * dy;
    if (r2 > 0.0) {
      const double t = q / r2;
      a[0] = a[0] + (-dy) * t;
      a[1] = a[1] + dx * t;
    }
  }
};

// part[(s * nc + c) * cnt + (t - t0)]: slice s's sum of component c for the targets t0 .. t0 + cnt - 1
template <class Term>
__global__ __launch_bounds__(kBlock) void pairs_k(Source s, double alpha, Targets g, i64 t0, i64 cnt,
                                                  double *__restrict__ part) {
  __shared__ double lx[kBlock], ly[kBlock], lq[kBlock];
  const int l = threadIdx.x;
  const i64 lt = (i64)blockIdx.x * kBlock + l;
  const bool live = lt < cnt;
  double X = 0.0, Y = 0.0, Z = 0.0;
  if (live) {
    size_t at, stride;
    target_of(g, t0 + lt, X, Y, Z, at, stride);
  }
  Term term(Z - s.zs, alpha);
  const i64 p0 = (i64)blockIdx.y * s.len;
  const i64 p1 = p0 + s.len < s.npix ? p0 + s.len : s.npix;
  for (i64 tile = p0; tile < p1; tile += kBlock) {
    const i64 p = tile + l;
    if (p < p1) {
      const i64 j = p / s.nsx;
      lx[l] = s.xs[p - j * s.nsx];
      ly[l] = s.ys[j];
      lq[l] = s.bz[p] * s.c;
    }
    __syncthreads();
    const int m = p1 - tile < kBlock ? (int)(p1 - tile) : kBlock;
    for (int n = 0; n < m; ++n) term.add(X - lx[n], Y - ly[n], lq[n]);
    __syncthreads();
  }
  if (live) {
    double *o = part + (size_t)blockIdx.y * Term::nc * (size_t)cnt + (size_t)lt;
#pragma unroll
    for (int c = 0; c < Term::nc; ++c) o[(size_t)c * (size_t)cnt] = term.a[c];
  }
}

// the largest node i0 <= n - 2 with v[i0] <= q, for v[0] <= q <= v[n - 1]: an estimate from the spacing, corrected
__device__ __forceinline__ int bracket(const double *v, int n, double q) {
  const double e = floor((q - v[0]) / (v[1] - v[0]));
  int i0 = e < 0.0 ? 0 : (e > (double)(n - 2) ? n - 2 : (int)e);
  while (i0 > 0 && v[i0] > q) --i0;
  while (i0 < n - 2 && v[i0 + 1] <= q) ++i0;
  return i0;
}

// theta = 0 and theta = 1 copy an end: a target on a node gets the node's value bit for bit
__device__ __forceinline__ double lerp(double v0, double v1, double th) {
  if (th == 0.0) return v0;
  if (th == 1.0) return v1;
  return (1.0 - th) * v0 + th * v1;
}

__device__ __forceinline__ double plane_bz(const Source &s, double X, double Y) {
  if (!(X >= s.xs[0] && X <= s.xs[s.nsx - 1] && Y >= s.ys[0] && Y <= s.ys[s.nsy - 1])) return 0.0;
  const int i0 = bracket(s.xs, s.nsx, X), j0 = bracket(s.ys, s.nsy, Y);
  const double tx = (X - s.xs[i0]) / (s.xs[i0 + 1] - s.xs[i0]);
  const double ty = (Y - s.ys[j0]) / (s.ys[j0 + 1] - s.ys[j0]);
  const double *r0 = s.bz + (size_t)s.nsx * (size_t)j0 + (size_t)i0, *r1 = r0 + s.nsx;
  return lerp(lerp(r0[0], r0[1], tx), lerp(r1[0], r1[1], tx), ty);
}

__global__ __launch_bounds__(kBlock) void fold_k(Source s, Targets g, i64 t0, i64 cnt, const double *__restrict__ part,
                                                 double *__restrict__ out) {
  const i64 lt = (i64)blockIdx.x * kBlock + threadIdx.x;
  if (lt >= cnt) return;
  double X, Y, Z;
  size_t at, stride;
  target_of(g, t0 + lt, X, Y, Z, at, stride);
  double b[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    b[c] = 0.0;
    if (c >= g.nc) continue;
    const double *q = part + (size_t)c * (size_t)cnt + (size_t)lt;
    double acc = q[0];
    for (int sl = 1; sl < s.nslices; ++sl) acc = acc + q[(size_t)sl * (size_t)g.nc * (size_t)cnt];
    b[c] = acc;
  }
  if (g.nc == 3) {
    const double w = Z - s.zs;
    if (w < 0.0) {
      b[0] = b[1] = b[2] = __builtin_nan("");
    } else if (w == 0.0) {
      b[2] = plane_bz(s, X, Y);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (c < g.nc) out[at + (size_t)c * stride] = b[c];
}

int slices_of(i64 npix) {
  const i64 ns = (npix + kSliceMin - 1) / kSliceMin;
  return (int)(ns < kSliceCap ? ns : kSliceCap);
}

bool source_ok(const int32_t *nsrc2, const double *h_xs, const double *h_ys) {
  if (nsrc2[0] < 2 || nsrc2[1] < 2) return false;
  return h_xs[1] - h_xs[0] > 0.0 && h_ys[1] - h_ys[0] > 0.0;     // (false for a NaN as well)
}

// the targets of a box call, in doubles: three axes of up to 2^31 nodes overflow 64-bit whole numbers
double box_targets(const int32_t *n3, int which) {
  const double nx = n3[0], ny = n3[1], nz = n3[2];
  return which == 0 ? nx * ny * nz - (nx - 2.0) * (ny - 2.0) * (nz - 2.0) : nx * ny * nz;
}
constexpr double kMaxTargets = 4.0e15;   // above any device's memory at 24 B per target, exact in a double and an i64

// device bytes of a call besides the caller's own arrays: the mesh vectors and the scratch of the largest chunk
double own_bytes(const int32_t *nsrc2, const int32_t *n3, double ntargets) {
  const double chunk = ntargets < (double)kChunk ? ntargets : (double)kChunk;
  double b = 8.0 * ((double)nsrc2[0] + (double)nsrc2[1]);
  if (n3) b += 8.0 * ((double)n3[0] + (double)n3[1] + (double)n3[2]);
  return b + 24.0 * chunk * (double)slices_of((i64)nsrc2[0] * nsrc2[1]);
}

// the shared driver: mesh vectors up, then chunk after chunk the all-pairs launch and the fold.  alpha NULL: the
// potential field (GreenTerm); else the constant-alpha field (LfffTerm).  g.nc == 2: the plane's vector potential
// (ApTerm)
int run(const int32_t *nsrc2, const double *h_xs, const double *h_ys, double zs, const double *bz, const double *alpha,
        Targets g, const int32_t *n3, const double *h_x, const double *h_y, const double *h_z, double *out) {
  Source s;
  s.nsx = nsrc2[0];
  s.nsy = nsrc2[1];
  s.npix = (i64)s.nsx * s.nsy;
  s.nslices = slices_of(s.npix);
  s.len = (s.npix + s.nslices - 1) / s.nslices;
  s.zs = zs;
  s.c = ((h_xs[1] - h_xs[0]) * (h_ys[1] - h_ys[0])) / 6.283185307179586;
  s.bz = bz;
  const i64 chunk = g.count < kChunk ? g.count : kChunk;
  const size_t nmesh = (size_t)s.nsx + (size_t)s.nsy + (n3 ? (size_t)n3[0] + (size_t)n3[1] + (size_t)n3[2] : 0);
  void *buf = nullptr;
  int rc = ndsmk_alloc(&buf, 8 * (nmesh + (size_t)g.nc * (size_t)chunk * (size_t)s.nslices));
  if (rc != 0) return rc;
  double *d = (double *)buf;
  s.xs = d;
  s.ys = d + s.nsx;
  rc = ndsmk_h2d(d, h_xs, 8 * (size_t)s.nsx);
  if (rc == 0) rc = ndsmk_h2d(d + s.nsx, h_ys, 8 * (size_t)s.nsy);
  double *m = d + s.nsx + s.nsy;
  if (g.gen == GEN_PLANE) {
    g.x = s.xs;
    g.y = s.ys;
  }
  if (n3 && rc == 0) {
    g.x = m;
    g.y = m + n3[0];
    g.z = m + n3[0] + n3[1];
    rc = ndsmk_h2d(m, h_x, 8 * (size_t)n3[0]);
    if (rc == 0) rc = ndsmk_h2d(m + n3[0], h_y, 8 * (size_t)n3[1]);
    if (rc == 0) rc = ndsmk_h2d(m + n3[0] + n3[1], h_z, 8 * (size_t)n3[2]);
  }
  double *part = d + nmesh;
  const auto pairs = g.nc == ApTerm::nc ? pairs_k<ApTerm> : alpha ? pairs_k<LfffTerm> : pairs_k<GreenTerm>;
  for (i64 t0 = 0; t0 < g.count && rc == 0; t0 += chunk) {
    const i64 cnt = g.count - t0 < chunk ? g.count - t0 : chunk;
    const unsigned nb = (unsigned)((cnt + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(pairs, dim3(nb, (unsigned)s.nslices), dim3(kBlock), 0, ndsm::stream(), s, alpha ? *alpha : 0.0,
                       g, t0, cnt, part);
    hipLaunchKernelGGL(fold_k, dim3(nb), dim3(kBlock), 0, ndsm::stream(), s, g, t0, cnt, part, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) rc = ndsm::fail((int)e, hipGetErrorString(e), __FILE__, __LINE__);
  }
  const int rf = ndsmk_free(buf);       // (drains the stream first)
  return rc != 0 ? rc : rf;
}

// 9004 with the entry's name, what it asks of its arguments and, for an entry that takes one, the finite alpha
int bad_value(const char *name, const char *needs, const double *alpha) {
  char msg[256];
  std::snprintf(msg, sizeof(msg), "%s: %s%s", name, needs, alpha ? ", and a finite alpha" : "");
  return ndsmk_note_error(NDSMK_EVALUE, msg);
}

// the point-list entries: gen GEN_POINTS (nc 3) or GEN_POINTS2 (nc 2); alpha NULL or the constant alpha
int points_entry(const char *name, int gen, int nc, const int32_t *nsrc2, const double *h_xs, const double *h_ys,
                 double zs, const double *bz, const double *alpha, int npts, const double *pts, double *out) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(nsrc2 && h_xs && h_ys && bz);
  if (!source_ok(nsrc2, h_xs, h_ys) || npts < 0 || (alpha && !std::isfinite(*alpha)))
    return bad_value(name, "at least 2 source nodes per axis, spacings > 0 and npts >= 0", alpha);
  if (npts == 0) return 0;
  NDSM_CHECK_ARG(pts && out);
  Targets g = {};
  g.gen = gen;
  g.nc = nc;
  g.count = npts;
  g.pts = pts;
  return run(nsrc2, h_xs, h_ys, zs, bz, alpha, g, nullptr, nullptr, nullptr, nullptr, out);
}

// the box entries: which = 0 the face nodes (GEN_FACES), which = 1 all nodes (GEN_VOLUME); alpha as above
int box_entry(const char *name, const int32_t *nsrc2, const double *h_xs, const double *h_ys, double zs,
              const double *bz, const double *alpha, const int32_t *n3, const double *h_x, const double *h_y,
              const double *h_z, int which, double *B) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(nsrc2 && h_xs && h_ys && bz && n3 && h_x && h_y && h_z && B);
  if (!source_ok(nsrc2, h_xs, h_ys) || (which != 0 && which != 1) || n3[0] < 2 || n3[1] < 2 || n3[2] < 2 ||
      !(h_z[0] >= zs) || (alpha && !std::isfinite(*alpha)))
    return bad_value(name, "at least 2 source nodes per axis, spacings > 0, which 0 or 1, at least 2 box nodes per "
                           "axis and z[0] >= zs", alpha);
  if (box_targets(n3, which) > kMaxTargets) {
    char msg[96];
    std::snprintf(msg, sizeof(msg), "%s: more targets than any device holds", name);
    return ndsmk_note_error(NDSMK_ENODEV, msg);
  }
  Targets g = {};
  g.gen = which == 0 ? GEN_FACES : GEN_VOLUME;
  g.nc = 3;
  g.count = (i64)box_targets(n3, which);      // (exact: whole numbers below 2^53)
  g.nx = n3[0];
  g.ny = n3[1];
  g.nz = n3[2];
  return run(nsrc2, h_xs, h_ys, zs, bz, alpha, g, n3, h_x, h_y, h_z, B);
}

}  // namespace

// 0, or 9001 when the device cannot hold a call's arrays: caller_bytes of the caller's side (staged host arrays) plus
// the mesh vectors and the scratch, against the device's TOTAL memory - a screen that needs no allocation, all in
// doubles; what is free at the moment shows when the allocation itself fails.  n3 NULL: the points entry with ntargets
// points; else the box entry (which as there; positive axes).
extern "C" int ndsmk_green_fits(const int32_t *nsrc2, const int32_t *n3, int which, long long ntargets,
                                double caller_bytes) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(nsrc2);
  const double nt = n3 ? box_targets(n3, which) : (double)ntargets;
  size_t fr = 0, tot = 0;
  const int rc = ndsmk_mem_info(&fr, &tot);
  if (rc != 0) return rc;
  if (nt > kMaxTargets || caller_bytes + own_bytes(nsrc2, n3, nt) > (double)tot)
    return ndsmk_note_error(NDSMK_ENODEV, "green: the arrays and the scratch need more device memory than the device has");
  return 0;
}

// B (3,npts) = the field at pts (3,npts); bz (nsx,nsy), pts and B are DEVICE arrays, h_xs and h_ys on the HOST.
// Returns when B is complete.
extern "C" int ndsmk_green_points(const int32_t *nsrc2, const double *h_xs, const double *h_ys, double zs,
                                  const double *bz, int npts, const double *pts, double *B) {
  return points_entry("green_points", GEN_POINTS, 3, nsrc2, h_xs, h_ys, zs, bz, nullptr, npts, pts, B);
}

// B (nx,ny,nz,3): which = 0 the nodes with an index at either end of an axis (every other node keeps what it holds),
// which = 1 all nodes.  bz and B are DEVICE arrays, the five mesh vectors on the HOST.  Returns when B is complete.
extern "C" int ndsmk_green_box(const int32_t *nsrc2, const double *h_xs, const double *h_ys, double zs,
                               const double *bz, const int32_t *n3, const double *h_x, const double *h_y,
                               const double *h_z, int which, double *B) {
  return box_entry("green_box", nsrc2, h_xs, h_ys, zs, bz, nullptr, n3, h_x, h_y, h_z, which, B);
}

// The constant-alpha field (semantics: include/ndsm_hip.h, ndsm_hip_lfff_points): the arguments of ndsmk_green_points
// and alpha, a finite double.  alpha = 0 gives the bits of ndsmk_green_points for a finite bz.
extern "C" int ndsmk_lfff_points(const int32_t *nsrc2, const double *h_xs, const double *h_ys, double zs,
                                 const double *bz, double alpha, int npts, const double *pts, double *B) {
  return points_entry("lfff_points", GEN_POINTS, 3, nsrc2, h_xs, h_ys, zs, bz, &alpha, npts, pts, B);
}

// the arguments of ndsmk_green_box and alpha
extern "C" int ndsmk_lfff_box(const int32_t *nsrc2, const double *h_xs, const double *h_ys, double zs,
                              const double *bz, double alpha, const int32_t *n3, const double *h_x, const double *h_y,
                              const double *h_z, int which, double *B) {
  return box_entry("lfff_box", nsrc2, h_xs, h_ys, zs, bz, &alpha, n3, h_x, h_y, h_z, which, B);
}

// The potential field's vector potential on the plane of the magnetogram (semantics: include/ndsm_hip.h,
// ndsm_hip_green_ap_points): Ap (2,npts) at pts (2,npts); bz, pts and Ap DEVICE arrays.  Chunks, scratch and screen are
// ndsmk_green_points'.
extern "C" int ndsmk_green_ap_points(const int32_t *nsrc2, const double *h_xs, const double *h_ys, const double *bz,
                                     int npts, const double *pts, double *Ap) {
  return points_entry("green_ap_points", GEN_POINTS2, 2, nsrc2, h_xs, h_ys, 0.0, bz, nullptr, npts, pts, Ap);
}

// the same on the source's own nodes: Ap (nsx,nsy,2)
extern "C" int ndsmk_green_ap_plane(const int32_t *nsrc2, const double *h_xs, const double *h_ys, const double *bz,
                                    double *Ap) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(nsrc2 && h_xs && h_ys && bz && Ap);
  if (!source_ok(nsrc2, h_xs, h_ys))
    return ndsmk_note_error(NDSMK_EVALUE, "green_ap_plane: at least 2 source nodes per axis and spacings > 0");
  Targets g = {};
  g.gen = GEN_PLANE;
  g.nc = 2;
  g.count = (i64)nsrc2[0] * nsrc2[1];
  g.nx = nsrc2[0];
  g.ny = nsrc2[1];
  return run(nsrc2, h_xs, h_ys, 0.0, bz, nullptr, g, nullptr, nullptr, nullptr, nullptr, Ap);
}
