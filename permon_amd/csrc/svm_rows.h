// The row sweeps of the dense SVM kernels (svm.hip, svm_train.hip), each written once:
//   svm_sweep_rows<SUB>            any d: one wavefront per row; what a kernel does with row i's dot product x_i . w is a functor f(i, dot)
//   svm_sweep_rows64<UNR, SUB>     d = 64: two rows per wave-instruction, UNR row pairs in flight; f(i, dot) as above
//   svm_sweep_rows64_lanes<UNR, SUB, NEXT>  d = 64, the paired passes: the rows' dot products handed out one per lane, the row's scalars asked for up front by a
//                                  functor pre, the elementwise work a functor row; NEXT: the rows' weights t_i accumulated into the column sums X't on the way
// (k_svm_xt64, pass 1 for d = 64, keeps a row loop of its own in svm.hip: it needs y_i a_i in every lane of the half-wave.)
// Device code only (svm_internal.h is what qppf.hip sees).  The loads, their order and the summation order are the kernels' bits: k ascending then pmh_wave_sum
// for any d, the two products then the 16-8-4-2-1 tree of the half-wave for d = 64.
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

// A sample subset (pmh_op_svm_dual_set_subset) reaches the sweeps as the template argument SUB and the operator's masked labels ym (m_i y_i: 0 on a held-out
// row).  SUB = 0: ym is not read and the code is the sweep without subsets.  SUB = 1: ym_i is read first and the loads of a held-out row are not issued (its
// dot product is 0, f is still called: it writes the row's 0)
// any d <= 64 * SVM_KMAX: one wavefront per row, lane j owns columns j, j + 64, ...; f(i, x_i . w) in lane 0 of the wave that owns row i
template <int SUB = 0, class F>
static __device__ __forceinline__ void svm_sweep_rows(int n, int d, const double *__restrict__ X, const double *__restrict__ w, F f, const double *__restrict__ ym = nullptr)
{
  const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  double          wr[SVM_KMAX];
#pragma unroll
  for (int k = 0; k < SVM_KMAX; k++) wr[k] = (lane + 64 * k < d) ? w[lane + 64 * k] : 0.0;
  for (long long i = gw; i < n; i += nw) {
    const double *xr = X + (size_t)i * d;
    double        s  = 0.0;
    if (SUB && ym[i] == 0.0) { // (uniform over the wave)
      if (lane == 0) f(i, 0.0);
      continue;
    }
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
// SUB: bit j of live says that row r0 + j is in the subset (svm_live_rows64); a row that is not is not loaded (zero)
template <int UNR, int SUB = 0>
static __device__ __forceinline__ void svm_load_rows64(int n, const double *__restrict__ X, long long r0, dbl2 (&v)[UNR], unsigned long long live = ~0ull)
{
  const int      lane = threadIdx.x & 63, half = lane >> 5, l2 = lane & 31;
  const unsigned lh = SUB ? (unsigned)(live >> half) : ~0u; // bit 2 u: this half-wave's row of pair u is in the subset
#pragma unroll
  for (int u = 0; u < UNR; u++) {
    const long long i = r0 + 2 * u + half;
    v[u] = (i < n && (!SUB || ((lh >> (2 * u)) & 1))) ? __builtin_nontemporal_load((const dbl2 *)(X + (size_t)i * 64) + l2) : dbl2{0.0, 0.0};
  }
}
// lane j < 2 UNR reads the masked label of row r0 + j (ONE coalesced load for the 2 UNR rows; 0 past the last row) -> yi; bit j of the result: row r0 + j is in the subset
template <int UNR>
static __device__ __forceinline__ unsigned long long svm_live_rows64(int n, const double *__restrict__ ym, long long r0, double &yi)
{
  const int       lane = threadIdx.x & 63;
  const long long i = r0 + lane;
  yi = (lane < 2 * UNR && i < n) ? ym[i] : 0.0;
  return __ballot(yi != 0.0);
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
// the rows from r0 on with or without a subset, the one place that chooses: SUB = 0 loads them all and leaves yi alone; SUB = 1 takes the masked labels first
// (svm_live_rows64: lane j < 2 UNR gets that of row r0 + j in yi) and loads the rows of the subset only
template <int UNR, int SUB>
static __device__ __forceinline__ void svm_load_rows64_sub(int n, const double *__restrict__ X, const double *__restrict__ ym, long long r0, dbl2 (&v)[UNR], double &yi)
{
  if (SUB) svm_load_rows64<UNR, SUB>(n, X, r0, v, svm_live_rows64<UNR>(n, ym, r0, yi));
  else svm_load_rows64<UNR>(n, X, r0, v);
}
// f(i, x_i . w) in the first lane of the half-wave that owns row i
template <int UNR, int SUB = 0, class F>
static __device__ __forceinline__ void svm_sweep_rows64(int n, const double *__restrict__ X, const double *__restrict__ w, F f, const double *__restrict__ ym = nullptr)
{
  const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l2 = lane & 31;
  const long long gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  const dbl2      wr = ((const dbl2 *)w)[l2];
  for (long long r0 = gw * 2 * UNR; r0 < n; r0 += nw * 2 * UNR) {
    dbl2   v[UNR];
    double yi;
    svm_load_rows64_sub<UNR, SUB>(n, X, ym, r0, v, yi);
#pragma unroll
    for (int u = 0; u < UNR; u++) {
      const long long i = r0 + 2 * u + half;
      const double    s = svm_row_dot(v[u], wr);
      if (l2 == 0 && i < n) f(i, s);
    }
  }
}

// The row loop of the paired passes (k_svm_x64_grad, k_svm_x64_p1 in svm.hip).  The rows' dot products land in the first lane of each half-wave; lane
// j < 2 UNR then takes row i = r0 + j (u = j >> 1, half = j & 1; act: it has one) and does the row's elementwise work once: ONE coalesced load per vector
// for the 2 UNR rows (a load per row costs the address unit a whole instruction each: measured 2 x the time of the plain pass).
//   sc = pre(i, act, ym)   asks for the row's scalars, the label among them, BEFORE the dot products, so that they travel with the rows of X.  SUB: ym is the
//                          row's masked label, which the loads have read already (a held-out row is not loaded); SUB = 0: ym is 0 and pre reads the label
//   t = row(i, act, dot, sc)  the elementwise work; t is the row's weight in the column sums that the NEXT pass 1 would form (0 where !act)
// NEXT: a0, a1 += t_i x_i for the two columns this lane holds of its half-wave's rows (svm_fold_cols finishes them)
template <int UNR, int SUB, int NEXT, class PRE, class ROW>
static __device__ __forceinline__ void svm_sweep_rows64_lanes(int n, const double *__restrict__ X, const double *__restrict__ y, const double *__restrict__ w, double &a0, double &a1, PRE pre, ROW row)
{
  const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l2 = lane & 31;
  const long long gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  const dbl2      wr = ((const dbl2 *)w)[l2];
  for (long long r0 = gw * 2 * UNR; r0 < n; r0 += nw * 2 * UNR) {
    dbl2   v[UNR];
    double ym = 0.0;
    svm_load_rows64_sub<UNR, SUB>(n, X, y, r0, v, ym);
    const long long i   = r0 + lane;
    const bool      act = lane < 2 * UNR && i < n;
    const auto      sc  = pre(i, act, ym);
    const double    sm  = svm_row_dots_to_lanes<UNR>(v, wr);
    const double    t   = row(i, act, sm, sc);
    if (NEXT) {
#pragma unroll
      for (int u = 0; u < UNR; u++) {
        const double tu = __shfl(t, 2 * u + half, 64);
        a0 += tu * v[u].x, a1 += tu * v[u].y;
      }
    }
  }
}
