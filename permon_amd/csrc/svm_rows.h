// The two row sweeps of the dense SVM kernels (svm.hip, svm_train.hip), each written once: what a kernel does with row i's dot product x_i . w is a functor
// f(i, dot).  Device code only (svm_internal.h is what qppf.hip sees).  The loads, their order and the summation order are the kernels' bits: k ascending
// then pmh_wave_sum for any d, the two products then the 16-8-4-2-1 tree of the half-wave for d = 64.
#pragma once
#include "reduce.h"
#include "svm_internal.h"

// 1 / (1 + e^z) without overflow: the two-branch form of Lin, Lin and Weng (svm_proba.hip), which the Platt fit and every probability kernel share
static __device__ __forceinline__ double svm_sigmoid(double z)
{
  if (z >= 0.0) {
    const double e = exp(-z);
    return e / (1.0 + e);
  }
  return 1.0 / (1.0 + exp(z));
}

// any d <= 64 * SVM_KMAX: one wavefront per row, lane j owns columns j, j + 64, ...; f(i, x_i . w) in lane 0 of the wave that owns row i
template <class F>
static __device__ __forceinline__ void svm_sweep_rows(int n, int d, const double *__restrict__ X, const double *__restrict__ w, F f)
{
  const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  double          wr[SVM_KMAX];
#pragma unroll
  for (int k = 0; k < SVM_KMAX; k++) wr[k] = (lane + 64 * k < d) ? w[lane + 64 * k] : 0.0;
  for (long long i = gw; i < n; i += nw) {
    const double *xr = X + (size_t)i * d;
    double        s  = 0.0;
#pragma unroll
    for (int k = 0; k < SVM_KMAX; k++) {
      const int c = lane + 64 * k;
      if (c < d) s += __builtin_nontemporal_load(&xr[c]) * wr[k];
    }
    s = pmh_wave_sum(s);
    if (lane == 0) f(i, s);
  }
}

// ---- d == 64: 16-byte loads, two rows per wave-instruction (lanes 0-31 row r, lanes 32-63 row r + 1), UNR row pairs in flight ----
typedef double dbl2 __attribute__((ext_vector_type(2))); // native 16-byte vector: accepted by the non-temporal builtins

// the UNR row pairs from row r0 on: v[u] = columns 2 l2, 2 l2 + 1 of row r0 + 2 u + half (zero past the last row)
template <int UNR>
static __device__ __forceinline__ void svm_load_rows64(int n, const double *__restrict__ X, long long r0, dbl2 (&v)[UNR])
{
  const int lane = threadIdx.x & 63, half = lane >> 5, l2 = lane & 31;
#pragma unroll
  for (int u = 0; u < UNR; u++) {
    const long long i = r0 + 2 * u + half;
    v[u] = (i < n) ? __builtin_nontemporal_load((const dbl2 *)(X + (size_t)i * 64) + l2) : dbl2{0.0, 0.0};
  }
}
// the row's dot product in the first lane of its half-wave
static __device__ __forceinline__ double svm_row_dot(dbl2 v, dbl2 wr)
{
  double s = v.x * wr.x + v.y * wr.y;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) s += __shfl_down(s, o, 32);
  return s;
}
// the dot products of the loaded rows, handed out one per lane: lane j < 2 UNR gets that of row r0 + j (u = j >> 1, half = j & 1)
template <int UNR>
static __device__ __forceinline__ double svm_row_dots_to_lanes(const dbl2 (&v)[UNR], dbl2 wr)
{
  const int lane = threadIdx.x & 63;
  double    su[UNR], sm = 0.0;
#pragma unroll
  for (int u = 0; u < UNR; u++) su[u] = svm_row_dot(v[u], wr);
#pragma unroll
  for (int u = 0; u < UNR; u++) {
    const double q = __shfl(su[u], (lane & 1) << 5, 64);
    if ((lane >> 1) == u) sm = q;
  }
  return sm;
}
// f(i, x_i . w) in the first lane of the half-wave that owns row i
template <int UNR, class F>
static __device__ __forceinline__ void svm_sweep_rows64(int n, const double *__restrict__ X, const double *__restrict__ w, F f)
{
  const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l2 = lane & 31;
  const long long gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  const dbl2      wr = ((const dbl2 *)w)[l2];
  for (long long r0 = gw * 2 * UNR; r0 < n; r0 += nw * 2 * UNR) {
    dbl2 v[UNR];
    svm_load_rows64<UNR>(n, X, r0, v);
#pragma unroll
    for (int u = 0; u < UNR; u++) {
      const long long i = r0 + 2 * u + half;
      const double    s = svm_row_dot(v[u], wr);
      if (l2 == 0 && i < n) f(i, s);
    }
  }
}
