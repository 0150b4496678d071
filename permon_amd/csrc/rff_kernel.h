// k_rff<TX, TZ, EPI, NG>, the one kernel that stores epi(X Omega), and its launches: Z[i][k] = epi(x_i . omega_k, row value of i, column value of k).  The random
// Fourier features (rff.hip) and stage A of the Nystroem map (nys.hip: Omega := L', Z := C) differ in the epilogue functor alone:
//   struct EPI {
//     static constexpr bool cols, rows;  // cols: the launch's column vector (beta; |l|^2) is staged in LDS beside Omega; rows: the functor has a value per row
//     double row(long long i) const;     // rows only: the value of row i of this launch (|x_i|^2: the array is the functor's member, not a kernel argument)
//     double operator()(double t, double rowv, double colv) const;  // t = x_i . omega_k; rowv, colv: 0.0 where the functor takes none
//   };
// rff_cos, rff_arg (rff_internal.h): cols.  nys_rbf, nys_q (nys_internal.h): cols and rows.  nys_poly, nys_t: neither.
// The layouts, the order of a row's sum and the shape of the epilogue loop are described in rff.hip; the product phase is RFF_PRODUCT_ROW_BLOCK (rff_internal.h).
// Device code: included by rff.hip and nys.hip only.
#pragma once
#include "rff_internal.h"

static __device__ __forceinline__ void rff_store4(double *z, const double v[4]) { *(rff_d4 *)z = rff_d4{v[0], v[1], v[2], v[3]}; }
static __device__ __forceinline__ void rff_store4(float *z, const double v[4]) { *(rff_f4 *)z = rff_f4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]}; }

template <class TX, class TZ, class EPI, int NG>
__global__ __launch_bounds__(RFF_NT) void k_rff(long long n, int d, int D, const TX *__restrict__ X, const double *__restrict__ Om, const double *__restrict__ beta, TZ *__restrict__ Z, EPI epi,
                                                int xvec, int zvec, int c0base)
{
  extern __shared__ double rff_lds[];
  double   *Ws = rff_lds, *Bs = rff_lds + RFF_KB * RFF_LDW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int c0 = c0base + blockIdx.y * RFF_CT, Dt = min(64 * NG, D - c0); // the launch's tiles have at most NG groups of 64 columns in use
  const int nkb = (d + RFF_KB - 1) / RFF_KB;
  const long long nrb = (n + RFF_RW - 1) / RFF_RW;
  const int sc = threadIdx.x & (RFF_CT - 1), sp = rff_pos(sc); // staging: this thread's column of the tile and its LDS position
  if (EPI::cols && threadIdx.x < 64 * NG) Bs[sp] = sc < Dt ? beta[c0 + sc] : 0.0;
  bool staged = false;
  for (long long rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    RFF_PRODUCT_ROW_BLOCK(acc, rb)
    // the epilogue on the accumulators: group q of 64 columns sits in acc[0 .. 3] on trip q
    const long long r0 = rb * RFF_RW + wave * 16 + g;
    double          rv[4] = {0.0, 0.0, 0.0, 0.0}; // the row values of the lane's rows g + 4 r: a row >= n has none to load
    if constexpr (EPI::rows) {
#pragma unroll
      for (int r = 0; r < 4; r++)
        if (r0 + 4 * r < n) rv[r] = epi.row(r0 + 4 * r);
    }
#pragma nounroll
    for (int q = 0; q < NG; q++) {
      const int cc = 64 * q + 4 * c; // the lane's 4 columns of the tile: cc .. cc + 3
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const long long i = r0 + 4 * r;
        if (i < n && cc < Dt) {
          double v[4];
#pragma unroll
          for (int jm = 0; jm < 4; jm++) {
            v[jm] = epi(acc[jm][r], rv[r], EPI::cols ? Bs[64 * q + 16 * jm + c] : 0.0);
            __builtin_amdgcn_sched_barrier(0); // one cosine or exponential at a time: interleaved, their temporaries do not fit beside 128 accumulator registers
          }
          TZ *z = Z + (size_t)i * D + c0 + cc;
          if (zvec) {
            rff_store4(z, v); // (D % 4 == 0: the 4 columns are inside together)
          } else {
#pragma unroll
            for (int jm = 0; jm < 4; jm++)
              if (cc + jm < Dt) z[jm] = (TZ)v[jm];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4 * NG - 4; j++) acc[j] = acc[j + 4];
    }
  }
}

// what a launch multiplies: X (n x d) Omega (d x D, row-major) and the column vector of D entries (read only where EPI::cols), all on the device
struct rff_operands {
  pmh_ctx       ctx;
  int           d, D;
  const double *omega, *colv;
};

// one launch over ntiles column tiles from column c0base on, each with at most NG groups of 64 columns in use
template <class TX, class TZ, class EPI, int NG> static int rff_launch_ng(const rff_operands &o, long long n, const void *X, void *Z, EPI epi, int c0base, int ntiles)
{
  auto *k = k_rff<TX, TZ, EPI, NG>;
  PMH_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, RFF_LDS_BYTES));
  const rff_shape s    = rff_launch_shape<TX>(o.ctx, n, o.d, X, ntiles);
  const int       zvec = o.D % 4 == 0 && (uintptr_t)Z % (4 * sizeof(TZ)) == 0;
  hipLaunchKernelGGL(k, s.grid, dim3(RFF_NT), RFF_LDS_BYTES, o.ctx->stream, n, o.d, o.D, (const TX *)X, o.omega, o.colv, (TZ *)Z, epi, s.xvec, zvec, c0base);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}
// the launches that cover the D columns
template <class TX, class TZ, class EPI> static int rff_launch(const rff_operands &o, long long n, const void *X, void *Z, EPI epi)
{
  return rff_tile_launches(o.D, [&](auto ng, int tile0, int ntiles) { return rff_launch_ng<TX, TZ, EPI, decltype(ng)::value>(o, n, X, Z, epi, tile0 * RFF_CT, ntiles); });
}
