// Resampling of node arrays between two uniform meshes on the same box (DESIGN.md "Coarse-to-fine cascade";
// semantics: include/ndsm_hip.h, ndsm_hip_resample), and the face paste of the cascade driver.
//
//   resample_k : one thread per destination node and component.  The operator is separable: the same 1-D rule along
//                x, then y, then z, each axis normalised by itself - for every z tap, for every y tap, the finished x
//                value; then the finished y value; then z.  The taps and their weights come from integers in the
//                thread (64-bit): no tables, no LDS, no atomics.
//                  mode 0, linear interpolation: a = i (ns - 1), j = a div (nd - 1), r = a mod (nd - 1); r = 0 copies
//                    v[j] and reads nothing else, otherwise theta = double(r) / double(nd - 1) and the value is
//                    (1.0 - theta) v[j] + theta v[j + 1].
//                  mode 1, hat average (nd <= ns): the end nodes copy the end nodes; any other node takes the source
//                    nodes f, ascending, with q_f = (ns - 1) - |f (nd - 1) - i (ns - 1)| > 0: one such node is copied,
//                    several give (sum double(q_f) v[f]) / double(sum q_f), the sum left to right from its first term.
//                An axis of one node on both sides is copied.  A destination face, edge or corner reads the same
//                face, edge or corner of the source only.
//   resample_weighted_k : the confidence-weighted restriction of an observation v with its confidence w (nd <= ns;
//                DESIGN.md "Cascade of the measurement fit"), one thread per destination node and component, the grid
//                and the taps of mode 1.  NOT normalised axis by axis: three sums run over the tensor of taps, nested
//                as above, each level sum double(q_f) (inner value) left to right from its first term - num from
//                w[f] v[f], den from w[f], pln from v[f].  A node with one tap on an axis (an end node, an axis of one
//                node, an axis with ns = nd) copies it: q = 1 and qsum = 1 there.  Q = (qsum_x qsum_y) qsum_z in
//                doubles; wdst = den / Q; dst = num / den where den > 0.0, otherwise pln / Q (the plain hat average).
//                A node with one tap on every axis copies v[f] and w[f]: ns = nd returns both arrays bit for bit.
//   paste_k    : dst = src on the k = 0 plane (which = 0) or on all six faces (which = 1) of two arrays of one shape;
//                which = 2 and 3 are the same two minus the nodes of the k = 0 plane off its rim (the freed nodes).
//
// Plain C++ under -ffp-contract=off: the operand order above is the bits, and tests/cascade_model.py and
// tests/obs_cascade_model.py restate it.
#include "common.hpp"

namespace {

using ndsm::i64;

struct ResArgs {
  int ns[3], nd[3];
  int ncomp, mode;
};

// the taps of one destination node on one axis: source nodes lo .. lo + cnt - 1
struct Taps {
  i64 lo, a, S, D, qsum;   // a = i (ns - 1), S = ns - 1, D = nd - 1; qsum: mode 1 with cnt > 1
  int cnt;
  double theta;            // mode 0 with cnt = 2
};

// a div d and a mod d for 0 <= a, 0 < d < 2^31: 32-bit whenever a fits (64-bit division is a long routine on the device)
__device__ __forceinline__ i64 div_mod(i64 a, i64 d, i64 &r) {
  if (a <= 0x7fffffffLL) {
    const unsigned ua = (unsigned)a, ud = (unsigned)d;
    r = (i64)(ua % ud);
    return (i64)(ua / ud);
  }
  r = a % d;
  return a / d;
}

__device__ __forceinline__ i64 hat_q(const Taps &t, i64 f) {
  const i64 d = f * t.D - t.a;
  return t.S - (d < 0 ? -d : d);
}

__device__ __forceinline__ Taps taps_of(int i, int ns, int nd, int mode) {
  Taps t;
  t.S = (i64)ns - 1;
  t.D = (i64)nd - 1;
  t.a = (i64)i * t.S;
  t.qsum = 0;
  t.theta = 0.0;
  t.cnt = 1;
  if (nd == 1) {            // (ns = 1 as well)
    t.lo = 0;
  } else if (mode == 0) {
    i64 r;
    t.lo = div_mod(t.a, t.D, r);
    if (r != 0) {
      t.cnt = 2;
      t.theta = (double)r / (double)t.D;
    }
  } else if (i == 0) {
    t.lo = 0;
  } else if (i == nd - 1) {
    t.lo = t.S;
  } else {
    // f D > a - S and f D < a + S; 1 <= i <= nd - 2 keeps both ends inside 1 .. ns - 2
    i64 r;
    t.lo = div_mod(t.a - t.S, t.D, r) + 1;
    const i64 hi = div_mod(t.a + t.S - 1, t.D, r);
    t.cnt = (int)(hi - t.lo + 1);
    for (i64 f = t.lo; f <= hi; ++f) t.qsum += hat_q(t, f);
  }
  return t;
}

// the 1-D rule on the values val(f) of the taps
template <class F>
__device__ __forceinline__ double combine(const Taps &t, int mode, F val) {
  if (t.cnt == 1) return val(t.lo);
  if (mode == 0) {
    const double v0 = val(t.lo), v1 = val(t.lo + 1);
    return (1.0 - t.theta) * v0 + t.theta * v1;
  }
  double acc = (double)hat_q(t, t.lo) * val(t.lo);
  for (int m = 1; m < t.cnt; ++m) acc = acc + (double)hat_q(t, t.lo + m) * val(t.lo + m);
  return acc / (double)t.qsum;
}

__global__ __launch_bounds__(256) void resample_k(const double *__restrict__ src, double *__restrict__ dst, ResArgs p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.nd[0]) return;
  const int mode = p.mode;
  const size_t sxs = (size_t)p.ns[0], sys = sxs * (size_t)p.ns[1], Ns = sys * (size_t)p.ns[2];
  const size_t sxd = (size_t)p.nd[0], syd = sxd * (size_t)p.nd[1], Nd = syd * (size_t)p.nd[2];
  const Taps tx = taps_of(i, p.ns[0], p.nd[0], mode);
  const i64 planes = (i64)p.nd[2] * (i64)p.ncomp;
  for (int j = blockIdx.y * blockDim.y + threadIdx.y; j < p.nd[1]; j += gridDim.y * blockDim.y) {
    const Taps ty = taps_of(j, p.ns[1], p.nd[1], mode);
    for (i64 kc = blockIdx.z; kc < planes; kc += gridDim.z) {
      i64 kk;
      const size_t c = (size_t)div_mod(kc, (i64)p.nd[2], kk);
      const int k = (int)kk;
      const Taps tz = taps_of(k, p.ns[2], p.nd[2], mode);
      const double *v = src + c * Ns;
      dst[c * Nd + (size_t)i + sxd * (size_t)j + syd * (size_t)k] = combine(tz, mode, [&](i64 fz) {
        return combine(ty, mode, [&](i64 fy) {
          const double *row = v + sys * (size_t)fz + sxs * (size_t)fy;
          return combine(tx, mode, [&](i64 fx) { return row[fx]; });
        });
      });
    }
  }
}

// the three sums of the weighted rule over the taps seen so far
struct WSums {
  double num, den, pln;
};

// one level of the weighted rule: sum double(q_f) (inner sums), left to right from its first term; a single tap has q = 1
template <class F>
__device__ __forceinline__ WSums wcombine(const Taps &t, F val) {
  WSums a = val(t.lo);
  if (t.cnt == 1) return a;
  const double q0 = (double)hat_q(t, t.lo);
  a.num = q0 * a.num;
  a.den = q0 * a.den;
  a.pln = q0 * a.pln;
  for (int m = 1; m < t.cnt; ++m) {
    const double q = (double)hat_q(t, t.lo + m);
    const WSums b = val(t.lo + m);
    a.num = a.num + q * b.num;
    a.den = a.den + q * b.den;
    a.pln = a.pln + q * b.pln;
  }
  return a;
}

__device__ __forceinline__ double wq_sum(const Taps &t) { return t.cnt == 1 ? 1.0 : (double)t.qsum; }

__global__ __launch_bounds__(256) void resample_weighted_k(const double *__restrict__ src, const double *__restrict__ wsrc,
                                                           double *__restrict__ dst, double *__restrict__ wdst, ResArgs p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.nd[0]) return;
  const size_t sxs = (size_t)p.ns[0], sys = sxs * (size_t)p.ns[1], Ns = sys * (size_t)p.ns[2];
  const size_t sxd = (size_t)p.nd[0], syd = sxd * (size_t)p.nd[1], Nd = syd * (size_t)p.nd[2];
  const Taps tx = taps_of(i, p.ns[0], p.nd[0], 1);
  const i64 planes = (i64)p.nd[2] * (i64)p.ncomp;
  for (int j = blockIdx.y * blockDim.y + threadIdx.y; j < p.nd[1]; j += gridDim.y * blockDim.y) {
    const Taps ty = taps_of(j, p.ns[1], p.nd[1], 1);
    for (i64 kc = blockIdx.z; kc < planes; kc += gridDim.z) {
      i64 kk;
      const size_t c = (size_t)div_mod(kc, (i64)p.nd[2], kk);
      const int k = (int)kk;
      const Taps tz = taps_of(k, p.ns[2], p.nd[2], 1);
      const double *v = src + c * Ns, *w = wsrc + c * Ns;
      const WSums s = wcombine(tz, [&](i64 fz) {
        return wcombine(ty, [&](i64 fy) {
          const size_t row = sys * (size_t)fz + sxs * (size_t)fy;
          return wcombine(tx, [&](i64 fx) {
            const double wf = w[row + (size_t)fx], vf = v[row + (size_t)fx];
            return WSums{wf * vf, wf, vf};
          });
        });
      });
      const double Q = (wq_sum(tx) * wq_sum(ty)) * wq_sum(tz);
      const size_t at = c * Nd + (size_t)i + sxd * (size_t)j + syd * (size_t)k;
      wdst[at] = s.den / Q;
      // (one tap in all: the value itself, not (w v) / w)
      const bool copy = tx.cnt == 1 && ty.cnt == 1 && tz.cnt == 1;
      dst[at] = copy ? s.pln : (s.den > 0.0 ? s.num / s.den : s.pln / Q);
    }
  }
}

__global__ __launch_bounds__(256) void paste_k(const double *__restrict__ src, double *__restrict__ dst, int nx, int ny,
                                               int nz, int ncomp, int which) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nx) return;
  const size_t sy = (size_t)nx, sz = sy * (size_t)ny, N = sz * (size_t)nz;
  const bool box = which == 1 || which == 3;     // all six faces; otherwise the k = 0 plane alone
  const i64 planes = box ? (i64)nz * (i64)ncomp : (i64)ncomp;
  for (int j = blockIdx.y * blockDim.y + threadIdx.y; j < ny; j += gridDim.y * blockDim.y) {
    const bool rim = i == 0 || i == nx - 1 || j == 0 || j == ny - 1;
    for (i64 kc = blockIdx.z; kc < planes; kc += gridDim.z) {
      i64 kk = 0;
      const size_t c = (size_t)(box ? div_mod(kc, (i64)nz, kk) : kc);
      const int k = (int)kk;
      if (box && !(rim || k == 0 || k == nz - 1)) continue;
      if (which >= 2 && k == 0 && !rim) continue;      // the freed nodes keep what they hold
      const size_t at = c * N + (size_t)i + sy * (size_t)j + sz * (size_t)k;
      dst[at] = src[at];
    }
  }
}

dim3 grid_of(int nx, int ny, i64 planes) {
  const i64 gy = ((i64)ny + 3) / 4;
  return dim3((unsigned)((nx + 63) / 64), (unsigned)(gy < 65535 ? gy : 65535), (unsigned)(planes < 65535 ? planes : 65535));
}

}  // namespace

// dst (ndst, ncomp) = the resampled src (nsrc, ncomp), DEVICE arrays that do not overlap.  Asynchronous.
extern "C" int ndsmk_resample(const int32_t *nsrc3, const int32_t *ndst3, int ncomp, int mode, const double *src,
                              double *dst) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(nsrc3 && ndst3 && src && dst);
  ResArgs p;
  p.ncomp = ncomp;
  p.mode = mode;
  bool ok = ncomp >= 1 && (mode == 0 || mode == 1);
  for (int d = 0; d < 3; ++d) {
    p.ns[d] = nsrc3[d];
    p.nd[d] = ndst3[d];
    const bool one = nsrc3[d] == 1 && ndst3[d] == 1;
    ok = ok && (one || (nsrc3[d] >= 2 && ndst3[d] >= 2)) && !(mode == 1 && ndst3[d] > nsrc3[d]);
  }
  if (!ok)
    return ndsmk_note_error(NDSMK_EVALUE, "resample: ncomp >= 1, mode 0 or 1, at least 2 nodes per axis on both sides "
                                          "(or 1 on both), and no axis finer than its source in mode 1");
  hipLaunchKernelGGL(resample_k, grid_of(p.nd[0], p.nd[1], (i64)p.nd[2] * ncomp), dim3(64, 4, 1), 0, ndsm::stream(),
                     src, dst, p);
  NDSM_LAUNCH_CHECK();
  return 0;
}

// (dst, wdst) (ndst, ncomp) = the confidence-weighted restriction of (src, wsrc) (nsrc, ncomp), four DEVICE arrays that
// do not overlap; finite values.  Asynchronous.
extern "C" int ndsmk_resample_weighted(const int32_t *nsrc3, const int32_t *ndst3, int ncomp, const double *src,
                                       const double *wsrc, double *dst, double *wdst) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(nsrc3 && ndst3 && src && wsrc && dst && wdst);
  ResArgs p;
  p.ncomp = ncomp;
  p.mode = 1;
  bool ok = ncomp >= 1;
  for (int d = 0; d < 3; ++d) {
    p.ns[d] = nsrc3[d];
    p.nd[d] = ndst3[d];
    const bool one = nsrc3[d] == 1 && ndst3[d] == 1;
    ok = ok && (one || (nsrc3[d] >= 2 && ndst3[d] >= 2)) && ndst3[d] <= nsrc3[d];
  }
  if (!ok)
    return ndsmk_note_error(NDSMK_EVALUE, "resample_weighted: ncomp >= 1, at least 2 nodes per axis on both sides (or 1 "
                                          "on both), and no axis finer than its source");
  hipLaunchKernelGGL(resample_weighted_k, grid_of(p.nd[0], p.nd[1], (i64)p.nd[2] * ncomp), dim3(64, 4, 1), 0,
                     ndsm::stream(), src, wsrc, dst, wdst, p);
  NDSM_LAUNCH_CHECK();
  return 0;
}

// dst = src on the k = 0 plane (which = 0) or on the six faces (which = 1), or on those minus the nodes of the k = 0
// plane off its rim (which = 2, 3); both (n3, ncomp), DEVICE.  Asynchronous.
extern "C" int ndsmk_paste_faces(const int32_t *n3, int ncomp, int which, const double *src, double *dst) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(n3 && src && dst && ncomp >= 1 && which >= 0 && which <= 3 && n3[0] >= 1 && n3[1] >= 1 && n3[2] >= 1);
  const bool box = which == 1 || which == 3;
  hipLaunchKernelGGL(paste_k, grid_of(n3[0], n3[1], box ? (i64)n3[2] * ncomp : (i64)ncomp), dim3(64, 4, 1), 0,
                     ndsm::stream(), src, dst, n3[0], n3[1], n3[2], ncomp, which);
  NDSM_LAUNCH_CHECK();
  return 0;
}
