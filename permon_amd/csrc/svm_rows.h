// The row sweeps of the dense SVM kernels (svm.hip, svm_train.hip), each written once:
//   svm_sweep_rows<SUB>            any d: one wavefront per row; what a kernel does with row i's dot product x_i . w is a functor f(i, dot)
//   svm_sweep_rows64<UNR, SUB>     d = 64: two (float samples: four) rows per wave-instruction, UNR row groups in flight; f(i, dot) as above
//   svm_sweep_rows64_lanes<UNR, SUB, NEXT>  d = 64, the paired passes: the rows' dot products handed out one per lane, the row's scalars asked for up front by a
//                                  functor pre, the elementwise work a functor row; NEXT: the rows' weights t_i accumulated into the column sums X't on the way
// (k_svm_xt64, pass 1 for d = 64, keeps a row loop of its own in svm.hip: it needs y_i a_i in every lane that holds a part of row i.)
// Device code only (svm_internal.h is what qppf.hip sees).  The loads, their order and the summation order are the kernels' bits: k ascending then pmh_wave_sum
// for any d, the two products then the 16-8-4-2-1 tree of the half-wave for d = 64.
// The samples are stored as T = double or float (the kernels' last template argument); a float is widened on arrival, (double)x, which is exact, and all
// arithmetic is fp64.  Any d: the float instances differ from the double ones in the load alone, so with -ffp-contract=off they give bit for bit what the
// double instances give on the widened samples.  d = 64: the float layout is another one (svm_row64<float>: four products then the 8-4-2-1 tree of the
// quarter-wave), with another, equally fixed, summation order.
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
// (T = float: rows are only 4-byte aligned unless d % 4 == 0, so the loads stay scalar)
template <int SUB = 0, class T, class F>
static __device__ __forceinline__ void svm_sweep_rows(int n, int d, const T *__restrict__ X, const double *__restrict__ w, F f, const double *__restrict__ ym = nullptr)
{
  const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  double          wr[SVM_KMAX];
#pragma unroll
  for (int k = 0; k < SVM_KMAX; k++) wr[k] = (lane + 64 * k < d) ? w[lane + 64 * k] : 0.0;
  for (long long i = gw; i < n; i += nw) {
    const T *xr = X + (size_t)i * d;
    double   s  = 0.0;
    if (SUB && ym[i] == 0.0) { // (uniform over the wave)
      if (lane == 0) f(i, 0.0);
      continue;
    }
#pragma unroll
    for (int k = 0; k < SVM_KMAX; k++) {
      const int c = lane + 64 * k;
      if (c < d) s += (double)__builtin_nontemporal_load(&xr[c]) * wr[k];
    }
    s = pmh_wave_sum(s);
    if (lane == 0) f(i, s);
  }
}

// ---- d == 64: 16-byte loads, RPI rows per wave-instruction, UNR row groups in flight ----
// The layout of a row depends on the type the samples are stored in (svm_row64<T>): LPR lanes hold one row, CPL adjacent columns each as ONE 16-byte
// non-temporal load, so that a wave-instruction covers RPI = 64 / LPR rows
//   double: a row is 512 B; lanes 0-31 row r, lanes 32-63 row r + 1; lane l2 = lane & 31 holds columns 2 l2, 2 l2 + 1
//   float:  a row is 256 B; lanes 0-15 row r, 16-31 row r + 1, 32-47 row r + 2, 48-63 row r + 3; lane q = lane & 15 holds columns 4 q .. 4 q + 3
// A float enters the arithmetic as (double)x: every product and every sum below is fp64 whatever T is.
typedef double dbl2 __attribute__((ext_vector_type(2))); // native 16-byte vectors: accepted by the non-temporal builtins
typedef float  flt4 __attribute__((ext_vector_type(4)));
typedef double dbl4 __attribute__((ext_vector_type(4))); // the four weights of a float lane's columns (two 16-byte loads, once per kernel)
template <class T> struct svm_row64;
template <> struct svm_row64<double> {
  typedef dbl2 vec;  // what a lane holds of a row
  typedef dbl2 wvec; // w in the lane's columns
  enum { LPR = 32, RPI = 2, CPL = 2 };
  static __device__ __forceinline__ vec    zero() { return vec{0.0, 0.0}; }
  static __device__ __forceinline__ double col(vec v, int c) { return c == 0 ? v.x : v.y; }
};
template <> struct svm_row64<float> {
  typedef flt4 vec;
  typedef dbl4 wvec;
  enum { LPR = 16, RPI = 4, CPL = 4 };
  static __device__ __forceinline__ vec    zero() { return vec{0.0f, 0.0f, 0.0f, 0.0f}; }
  static __device__ __forceinline__ double col(vec v, int c) { return (double)(c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w); }
};

// the UNR row groups from row r0 on: v[u] = this lane's CPL columns of row r0 + RPI u + sub, sub = lane / LPR (zero past the last row)
// SUB: bit j of live says that row r0 + j is in the subset (svm_live_rows64); a row that is not is not loaded (zero)
template <int UNR, int SUB = 0, class T>
static __device__ __forceinline__ void svm_load_rows64(int n, const T *__restrict__ X, long long r0, typename svm_row64<T>::vec (&v)[UNR], unsigned long long live = ~0ull)
{
  typedef svm_row64<T> R;
  const int      lane = threadIdx.x & 63, sub = lane / R::LPR, lq = lane & (R::LPR - 1);
  const unsigned lh = SUB ? (unsigned)(live >> sub) : ~0u; // bit RPI u: this lane's row of group u is in the subset
#pragma unroll
  for (int u = 0; u < UNR; u++) {
    const long long i = r0 + R::RPI * u + sub;
    v[u] = (i < n && (!SUB || ((lh >> (R::RPI * u)) & 1))) ? __builtin_nontemporal_load((const typename R::vec *)(X + (size_t)i * 64) + lq) : R::zero();
  }
}
// lane j < NR (the rows of one group sweep, RPI UNR) reads the masked label of row r0 + j (ONE coalesced load; 0 past the last row) -> yi; bit j of the result:
// row r0 + j is in the subset
template <int NR>
static __device__ __forceinline__ unsigned long long svm_live_rows64(int n, const double *__restrict__ ym, long long r0, double &yi)
{
  const int       lane = threadIdx.x & 63;
  const long long i = r0 + lane;
  yi = (lane < NR && i < n) ? ym[i] : 0.0;
  return __ballot(yi != 0.0);
}
// the row's dot product in the first lane of the LPR lanes that hold it
// double: the two products, then the 16-8-4-2-1 tree of the half-wave
static __device__ __forceinline__ double svm_row_dot(dbl2 v, dbl2 wr)
{
  double s = v.x * wr.x + v.y * wr.y;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) s += __shfl_down(s, o, 32);
  return s;
}
// float: the four products summed left to right, ((x0 w0 + x1 w1) + x2 w2) + x3 w3, then the 8-4-2-1 tree of the quarter-wave
static __device__ __forceinline__ double svm_row_dot(flt4 v, dbl4 wr)
{
  double s = (double)v.x * wr.x + (double)v.y * wr.y + (double)v.z * wr.z + (double)v.w * wr.w;
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_down(s, o, 16);
  return s;
}
// the dot products of the loaded rows, handed out one per lane: lane j < RPI UNR gets that of row r0 + j (u = j / RPI, sub = j % RPI)
template <int UNR, class T>
static __device__ __forceinline__ double svm_row_dots_to_lanes(const typename svm_row64<T>::vec (&v)[UNR], typename svm_row64<T>::wvec wr)
{
  typedef svm_row64<T> R;
  const int lane = threadIdx.x & 63;
  double    su[UNR], sm = 0.0;
#pragma unroll
  for (int u = 0; u < UNR; u++) su[u] = svm_row_dot(v[u], wr);
#pragma unroll
  for (int u = 0; u < UNR; u++) {
    const double q = __shfl(su[u], (lane & (R::RPI - 1)) * R::LPR, 64);
    if ((lane / R::RPI) == u) sm = q;
  }
  return sm;
}
// the rows from r0 on with or without a subset, the one place that chooses: SUB = 0 loads them all and leaves yi alone; SUB = 1 takes the masked labels first
// (svm_live_rows64: lane j < RPI UNR gets that of row r0 + j in yi) and loads the rows of the subset only
template <int UNR, int SUB, class T>
static __device__ __forceinline__ void svm_load_rows64_sub(int n, const T *__restrict__ X, const double *__restrict__ ym, long long r0, typename svm_row64<T>::vec (&v)[UNR], double &yi)
{
  if (SUB) svm_load_rows64<UNR, SUB>(n, X, r0, v, svm_live_rows64<svm_row64<T>::RPI * UNR>(n, ym, r0, yi));
  else svm_load_rows64<UNR>(n, X, r0, v);
}
// f(i, x_i . w) in the first lane of the LPR lanes that own row i
template <int UNR, int SUB = 0, class T, class F>
static __device__ __forceinline__ void svm_sweep_rows64(int n, const T *__restrict__ X, const double *__restrict__ w, F f, const double *__restrict__ ym = nullptr)
{
  typedef svm_row64<T> R;
  const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / R::LPR, lq = lane & (R::LPR - 1);
  const long long gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  const typename R::wvec wr = ((const typename R::wvec *)w)[lq];
  for (long long r0 = gw * R::RPI * UNR; r0 < n; r0 += nw * R::RPI * UNR) {
    typename R::vec v[UNR];
    double          yi;
    svm_load_rows64_sub<UNR, SUB>(n, X, ym, r0, v, yi);
#pragma unroll
    for (int u = 0; u < UNR; u++) {
      const long long i = r0 + R::RPI * u + sub;
      const double    s = svm_row_dot(v[u], wr);
      if (lq == 0 && i < n) f(i, s);
    }
  }
}

// ---- the column sums of a pass 1 for d = 64 (k_svm_xt64 and the paired passes in svm.hip, k_svr_xt64 in svr.hip) ----
// the CPL column sums a lane holds (double: columns 2 l2, 2 l2 + 1; float: columns 4 q .. 4 q + 3, of the rows its LPR lanes visited) -> part[workgroup][64]:
// lanes l, l + LPR, ... hold the same columns of different rows: fold by halving, double: l + (l + 32); float: (q + (q + 32)) + ((q + 16) + (q + 48)); then
// across the 4 waves in order
template <class T>
static __device__ __forceinline__ void svm_fold_cols(double (&acc)[svm_row64<T>::CPL], double (*lds)[64], double *__restrict__ part)
{
  typedef svm_row64<T> R;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / R::LPR, lq = lane & (R::LPR - 1);
#pragma unroll
  for (int o = 32; o >= R::LPR; o >>= 1) {
#pragma unroll
    for (int c = 0; c < R::CPL; c++) acc[c] += __shfl_down(acc[c], o, 64);
  }
  if (sub == 0) {
#pragma unroll
    for (int c = 0; c < R::CPL; c++) lds[wave][R::CPL * lq + c] = acc[c];
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    double v = lds[0][threadIdx.x];
#pragma unroll
    for (int wv = 1; wv < PMH_BLOCK / 64; wv++) v += lds[wv][threadIdx.x];
    part[(size_t)blockIdx.x * 64 + threadIdx.x] = v;
  }
}

// The row loop of the paired passes (k_svm_x64_grad, k_svm_x64_p1 in svm.hip).  The rows' dot products land in the first lane of the LPR lanes of each row; lane
// j < RPI UNR then takes row i = r0 + j (u = j / RPI, sub = j % RPI; act: it has one) and does the row's elementwise work once: ONE coalesced load per vector
// for the RPI UNR rows (a load per row costs the address unit a whole instruction each: measured 2 x the time of the plain pass).
//   sc = pre(i, act, ym)   asks for the row's scalars, the label among them, BEFORE the dot products, so that they travel with the rows of X.  SUB: ym is the
//                          row's masked label, which the loads have read already (a held-out row is not loaded); SUB = 0: ym is 0 and pre reads the label
//   t = row(i, act, dot, sc)  the elementwise work; t is the row's weight in the column sums that the NEXT pass 1 would form (0 where !act)
// NEXT: acc[c] += t_i x_i for the CPL columns this lane holds of the rows its LPR lanes visit, u ascending (svm_fold_cols finishes them)
template <int UNR, int SUB, int NEXT, class T, class PRE, class ROW>
static __device__ __forceinline__ void svm_sweep_rows64_lanes(int n, const T *__restrict__ X, const double *__restrict__ y, const double *__restrict__ w, double (&acc)[svm_row64<T>::CPL], PRE pre, ROW row)
{
  typedef svm_row64<T> R;
  const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / R::LPR, lq = lane & (R::LPR - 1);
  const long long gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  const typename R::wvec wr = ((const typename R::wvec *)w)[lq];
  for (long long r0 = gw * R::RPI * UNR; r0 < n; r0 += nw * R::RPI * UNR) {
    typename R::vec v[UNR];
    double          ym = 0.0;
    svm_load_rows64_sub<UNR, SUB>(n, X, y, r0, v, ym);
    const long long i   = r0 + lane;
    const bool      act = lane < R::RPI * UNR && i < n;
    const auto      sc  = pre(i, act, ym);
    const double    sm  = svm_row_dots_to_lanes<UNR, T>(v, wr);
    const double    t   = row(i, act, sm, sc);
    if (NEXT) {
#pragma unroll
      for (int u = 0; u < UNR; u++) {
        const double tu = __shfl(t, R::RPI * u + sub, 64);
#pragma unroll
        for (int c = 0; c < R::CPL; c++) acc[c] += tu * R::col(v[u], c);
      }
    }
  }
}
