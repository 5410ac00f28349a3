// Vector potentials in the DeVore gauge A_z = 0 on the device (DESIGN.md "DeVore-gauge vector potentials"): A of
// B integrated up from the bottom plane, A_p of B_p integrated down from A's top plane (Valori et al. 2012).
// Trapezoid cumulative sums in fp64, the operand order of the recurrences below (no contraction: -ffp-contract=off):
//
//   base    : plane 0 of A, b_x(i,j) = b_x(i,j-1) - (Bz(i,j-1,0) + Bz(i,j,0)) * (h_y/4), b_x(i,0) = 0
//                           b_y(i,j) = b_y(i-1,j) + (Bz(i-1,j,0) + Bz(i,j,0)) * (h_x/4), b_y(0,j) = 0
//             Two 1-D scans of one plane: along y with threads over i, along x with threads over j.
//   columns : one thread per (i,j) column.  Up, k = 1 .. nz-1:
//               A_x(k) = A_x(k-1) + (B_y(k-1) + B_y(k)) * (h_z/2),  A_y(k) = A_y(k-1) - (B_x(k-1) + B_x(k)) * (h_z/2)
//             then A_p(nz-1) = A(nz-1) and down, k = nz-2 .. 0:
//               A_p,x(k) = A_p,x(k+1) - (B_p,y(k) + B_p,y(k+1)) * (h_z/2)
//               A_p,y(k) = A_p,y(k+1) + (B_p,x(k) + B_p,x(k+1)) * (h_z/2)
//             A_z = A_p,z = 0.  The loads of kDvUnroll planes are in flight ahead of the running sums.
//             B_x, B_y, B_p,x, B_p,y in, A and A_p out: 16 + 16 + 24 + 24 = 80 B/pt.
// The h/4 and h/2 factors are formed once on the host.
#include "common.hpp"

namespace {

constexpr int kDvBlock = 256;       // columns: 256 consecutive columns (i fastest) per block
constexpr int kDvBaseBlock = 64;    // base plane: one wave per block, so the few scans spread over CUs
constexpr int kDvUnroll = 8;        // columns: planes whose loads are in flight ahead of the running sums
constexpr int kDvBaseUnroll = 16;   // base plane: points loaded ahead (a few hundred threads in all: latency)

struct DvArgs {
  int n[3];
  double qx, qy;   // h_x / 4, h_y / 4
  double hz;       // h_z / 2
};

// plane 0 of A (its z-component is written by the columns kernel): thread t < nx integrates b_x along y for
// i = t, thread nx + j integrates b_y along x for row j
__global__ __launch_bounds__(kDvBaseBlock) void devore_base_k(const double *__restrict__ B, double *__restrict__ A,
                                                              DvArgs p) {
  const int t = blockIdx.x * kDvBaseBlock + threadIdx.x;
  const int nx = p.n[0], ny = p.n[1];
  const size_t N = (size_t)nx * (size_t)ny * (size_t)p.n[2];
  const double *__restrict__ Bz = B + 2 * N;
  // b_x = run - (prev + v) * (h_y/4) is run + (prev + v) * (-h_y/4) bit for bit: negation is exact
  size_t c0, s;
  int len;
  double q;
  double *__restrict__ out;
  if (t < nx) {                  // b_x: along y, stride nx; a wave reads 64 consecutive i
    c0 = (size_t)t, s = (size_t)nx, len = ny, q = -p.qy, out = A;
  } else if (t < nx + ny) {      // b_y: along x, stride 1
    c0 = (size_t)(t - nx) * (size_t)nx, s = 1, len = nx, q = p.qx, out = A + N;
  } else {
    return;
  }
  double run = 0.0, prev = Bz[c0];
  out[c0] = 0.0;
  auto step = [&](int m, double v) {
    run = run + (prev + v) * q;
    prev = v;
    out[c0 + s * (size_t)m] = run;
  };
  int m = 1;
  for (; m + kDvBaseUnroll <= len; m += kDvBaseUnroll) {
    double v[kDvBaseUnroll];
#pragma unroll
    for (int u = 0; u < kDvBaseUnroll; ++u) v[u] = Bz[c0 + s * (size_t)(m + u)];
#pragma unroll
    for (int u = 0; u < kDvBaseUnroll; ++u) step(m + u, v[u]);
  }
  for (; m < len; ++m) step(m, Bz[c0 + s * (size_t)m]);
}

// one thread per (i,j) column q = i + nx j: A up from plane 0 (the base plane), then A_p down from A's top plane.
// The loads of kDvUnroll planes are issued before the sums that need them (guide: hide latency by ILP).
__global__ __launch_bounds__(kDvBlock) void devore_columns_k(const double *__restrict__ B, const double *__restrict__ Bp,
                                                             double *__restrict__ A, double *__restrict__ Ap,
                                                             DvArgs p) {
  const size_t ncol = (size_t)p.n[0] * (size_t)p.n[1];
  const size_t q = (size_t)blockIdx.x * kDvBlock + threadIdx.x;
  if (q >= ncol) return;
  const int nz = p.n[2];
  const size_t N = ncol * (size_t)nz;
  const double hz = p.hz;
  // up: A_x(k) = A_x(k-1) + (B_y(k-1) + B_y(k)) h_z/2, A_y(k) = A_y(k-1) - (B_x(k-1) + B_x(k)) h_z/2
  double ax = A[q], ay = A[q + N];
  double bx0 = B[q], by0 = B[q + N];
  A[q + 2 * N] = 0.0;
  auto up = [&](int k, double bx, double by) {
    const size_t c = q + ncol * (size_t)k;
    ax = ax + (by0 + by) * hz;
    ay = ay - (bx0 + bx) * hz;
    bx0 = bx;
    by0 = by;
    A[c] = ax;
    A[c + N] = ay;
    A[c + 2 * N] = 0.0;
  };
  int k = 1;
  for (; k + kDvUnroll <= nz; k += kDvUnroll) {
    double bx[kDvUnroll], by[kDvUnroll];
#pragma unroll
    for (int u = 0; u < kDvUnroll; ++u) {
      const size_t c = q + ncol * (size_t)(k + u);
      bx[u] = B[c];
      by[u] = B[c + N];
    }
#pragma unroll
    for (int u = 0; u < kDvUnroll; ++u) up(k + u, bx[u], by[u]);
  }
  for (; k < nz; ++k) up(k, B[q + ncol * (size_t)k], B[q + ncol * (size_t)k + N]);
  // down: A_p(nz-1) = A(nz-1), then A_p,x(k) = A_p,x(k+1) - (B_p,y(k) + B_p,y(k+1)) h_z/2,
  //                                  A_p,y(k) = A_p,y(k+1) + (B_p,x(k) + B_p,x(k+1)) h_z/2
  const size_t ct = q + ncol * (size_t)(nz - 1);
  Ap[ct] = ax;
  Ap[ct + N] = ay;
  Ap[ct + 2 * N] = 0.0;
  double px1 = Bp[ct], py1 = Bp[ct + N];
  auto down = [&](int k, double px, double py) {
    const size_t c = q + ncol * (size_t)k;
    ax = ax - (py + py1) * hz;
    ay = ay + (px + px1) * hz;
    px1 = px;
    py1 = py;
    Ap[c] = ax;
    Ap[c + N] = ay;
    Ap[c + 2 * N] = 0.0;
  };
  k = nz - 2;
  for (; k - kDvUnroll + 1 >= 0; k -= kDvUnroll) {
    double px[kDvUnroll], py[kDvUnroll];
#pragma unroll
    for (int u = 0; u < kDvUnroll; ++u) {
      const size_t c = q + ncol * (size_t)(k - u);
      px[u] = Bp[c];
      py[u] = Bp[c + N];
    }
#pragma unroll
    for (int u = 0; u < kDvUnroll; ++u) down(k - u, px[u], py[u]);
  }
  for (; k >= 0; --k) down(k, Bp[q + ncol * (size_t)k], Bp[q + ncol * (size_t)k + N]);
}

}  // namespace

// A, Ap (nx,ny,nz,3) of B, Bp (nx,ny,nz,3) in the DeVore gauge, all DEVICE arrays; A and Ap distinct from each
// other and from B, Bp.  h_dq3: the handle's spacings.  Asynchronous.
extern "C" int ndsmk_devore(const double *B, const double *Bp, double *A, double *Ap, const int32_t *n3,
                            const double *h_dq3) {
  NDSM_REQUIRE_READY();
  NDSM_CHECK_ARG(B && Bp && A && Ap && A != Ap && n3[0] >= 3 && n3[1] >= 3 && n3[2] >= 3);
  DvArgs p;
  for (int d = 0; d < 3; ++d) p.n[d] = n3[d];
  p.qx = 0.25 * h_dq3[0];
  p.qy = 0.25 * h_dq3[1];
  p.hz = 0.5 * h_dq3[2];
  const size_t ncol = (size_t)n3[0] * (size_t)n3[1];
  const unsigned nbase = (unsigned)((n3[0] + n3[1] + kDvBaseBlock - 1) / kDvBaseBlock);
  const unsigned ncolb = (unsigned)((ncol + kDvBlock - 1) / kDvBlock);
  hipStream_t s = ndsm::stream();
  hipLaunchKernelGGL(devore_base_k, dim3(nbase), dim3(kDvBaseBlock), 0, s, B, A, p);
  NDSM_LAUNCH_CHECK();
  hipLaunchKernelGGL(devore_columns_k, dim3(ncolb), dim3(kDvBlock), 0, s, B, Bp, A, Ap, p);
  NDSM_LAUNCH_CHECK();
  return 0;
}
