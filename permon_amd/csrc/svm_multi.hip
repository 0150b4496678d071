// SVM with more than two classes: K-column scoring in one pass over the test samples, and the one-vs-rest front end (pmh_svm_multi_*) over ONE binary handle.
//
// Scoring: S[i,k] = x_i . W_k + b_k (n x K, row-major) and label[i] = the class value of the greatest score of row i (ties: the lowest class index; NaN scores
// are not a case).  Either output may be NULL.  The classes go through a sweep in chunks of SVMM_KC: the chunk's weights sit in registers (dense) or are
// gathered as SVMM_KC contiguous doubles per stored entry (CSR), so one read of a sample serves SVMM_KC dot products.  K > SVMM_KC: one sweep per chunk, chunks
// ascending; the running greatest score of a row travels in a workspace of n doubles (best), and a later chunk takes the label only with a strictly greater
// score, so the lowest class index wins a tie across chunks as inside one.  No float atomics; the order of every sum is fixed (below), so two calls give the
// same bits, and a class's score does not depend on where in its chunk it sits, nor on which outputs were asked for.
//
//   dense, d = 64 (k_svmm_rows64): the row-pair layout and 16-byte non-temporal loads of svm_rows.h (lanes 0-31 row r, lanes 32-63 row r + 1, lane l2 holds
//     columns 2 l2, 2 l2 + 1).  Per class the lane's partial sum is x_0 w_0 + x_1 w_1 (two products, one addition), then the halving butterfly over the 32
//     lanes of the row (svmm_halve): at offset 16 a lane keeps the sums of one half of the chunk's classes and gives the other half to its partner, at 8 and 4
//     again (4 + 2 + 1 shuffles for a chunk of 8; for the chunk of 4 in use: offsets 16 and 8, 2 + 1 shuffles), every step kept + received; then the sum of the
//     one class left is completed over the remaining offsets (.., 2, 1: t + partner's t).  The class c of the chunk ends in lanes c (32 / KC) .. of the row.  Last: + b_k.
//   dense, any d <= 256 (k_svmm_rows): one wavefront per row as svm_sweep_rows, lane j holds columns j, j + 64, ..; per class 0 + x_j w_j + x_{j+64} w_{j+64} + ..
//     (columns past d count as 0 * 0), then the same butterfly over 64 lanes (a chunk of 4: offsets 32, 16 halving; 8, 4, 2, 1 completing), + b_k.
//   CSR (k_svmm_seg / k_svmm_fin): the entry-partitioned segmented sum of svm_csr.hip (svc_segments / svc_finish of svm_csr_seg.h) with SVMM_KC sums per sample.
//     A workgroup stages its span's values and column indices in LDS (24 KiB); a stored entry adds val * Wt[col][class] to each class's sum.  Last: + b_k.  Wt is
//     the chunk's weights as d x SVMM_KC, class index fastest: 8 SVMM_KC contiguous bytes per stored entry.  A sample without entries scores b_k.
//
// Algorithmic bytes of one call: dense 8 n d ceil(K / KC) + 8 n K (scores) + 8 n (labels), against K (8 n d + 8 n) for K binary calls; CSR 12 nnz ceil(K / KC)
// + 4 n + 8 n K + 8 n, the gathers of Wt (8 KC bytes per entry) served by the caches where 8 KC d bytes fit.
//
// Probabilities (pmh_svm_multi_predict_proba): the same sweeps instantiated on svmm_out_proba write sigma_ik = 1 / (1 + exp(A_k S[i,k] + B_k)) where they write
// S[i,k] -- S[i,k] the very sum the scoring instance forms -- and k_svmm_normalise divides every row by its sum, k ascending: 16 n K bytes more.  The scoring
// instances (svmm_out) are what they were: the probability is a separate instance, not a branch.
//
// One-vs-rest training: the K binary problems "class k against the rest" are trained one after the other on ONE pmh_svm handle over X -- X is uploaded once and
// the CSR operator's column-ordered copy is built once; pmh_svm_set_labels re-labels the handle between the classes -- and give W (K x d) and b (K).
//
// Subsets and the handle's own rows (pmh_svm_multi_set_subset, _predict_own, _test_own): the subset is the binary handle's, which keeps it across the re-labelling,
// so training over S is the binary handle's SUB = 1 kernels and nothing new here but k_svmm_class_count.  pmh_svm_multi_predict_own runs the sweeps above over the
// X the binary handle borrows (CSR: the handle's own pmh_csr).  pmh_svm_multi_test_own over the held-out rows or the subset runs the dense sweeps' SEL = 1 instances:
// the row's selector (n doubles, non-zero = selected: the binary handle's mask, or its complement 1 - m kept here) is read before anything of the row, an
// unselected row of X is never loaded and nothing is stored for it, and k_svmm_confusion<1> counts the selected rows alone.  Bytes: dense share (8 n d + 8 n)
// ceil(K / KC) + 8 n ceil(K / KC) (the selector) + 8 n + 16 share n (confusion), share the selected rows' part of n.  CSR: no row skipping, as on the binary
// handle -- every stored entry is swept and every row written, 12 nnz ceil(K / KC) + 4 n as above, and the selection happens in the confusion kernel alone.
#include <algorithm>
#include <cmath>
#include <vector>

#include "svm_csr_seg.h"
#include "svm_internal.h"
#include "svm_rows.h"

// classes per sweep (SVMM_KC in the text above), a power of two >= 2, per path: dense d = 64 (<= 32), dense any d (<= 64), CSR.  Measured with 4, 8 and 16
// on every path (docs/LAB_NOTEBOOK.md, "SVM multiclass"): the sweeps are bound by their instructions, not by HBM, a sweep's time grows about in proportion
// to its chunk, and 4 is the one value with which one call beats K binary calls at K = 4 and K = 10 on all three paths (8 is ahead only at K = 32, by <= 20 %)
#ifndef SVMM_KC64
#define SVMM_KC64 4
#endif
#ifndef SVMM_KCD
#define SVMM_KCD 4
#endif
#ifndef SVMM_KCC
#define SVMM_KCC 4
#endif

// where a chunk's results go
struct svmm_out {
  int           K, k0, kc; // classes in all; the chunk's first class and its number of classes (<= SVMM_KC)
  const double *b, *classes; // K each
  double       *scores, *labels; // n x K / n, either may be nullptr
  double       *best;            // n: the greatest score of the chunks so far (K > SVMM_KC and labels asked for), else nullptr
  static constexpr bool PROBA = false;
};
// probabilities in place of the scores: scores[i K + k] = svm_sigmoid(A[k] S[i,k] + B[k]); no labels
struct svmm_out_proba : svmm_out {
  const double *A, *B; // K each: the classes' Platt pairs
  static constexpr bool PROBA = true;
};
// what a lane that ends with the sum of class c needs beside b_c
template <class OUT> static __device__ __forceinline__ void svmm_lane_cal(const OUT &o, int c, double &ca, double &cb)
{
  ca = cb = 0.0;
  if constexpr (OUT::PROBA)
    if (c < o.kc) ca = o.A[o.k0 + c], cb = o.B[o.k0 + c];
}

// row i's greatest score of this chunk, bv of class index bk: the label, unless an earlier chunk holds a score at least as great
static __device__ __forceinline__ void svmm_label(const svmm_out &o, long long i, double bv, int bk)
{
  if (o.k0 > 0 && !(bv > o.best[i])) return;
  if (o.best) o.best[i] = bv;
  o.labels[i] = o.classes[bk];
}

// all KC sums of row i in one lane (the CSR kernels): + b_k, scores, the chunk's first maximum
template <int KC, class OUT> static __device__ __forceinline__ void svmm_row_done(const OUT &o, long long i, const double (&s)[KC])
{
  if constexpr (OUT::PROBA) {
#pragma unroll
    for (int j = 0; j < KC; j++)
      if (j < o.kc) o.scores[(size_t)i * o.K + o.k0 + j] = svm_sigmoid(o.A[o.k0 + j] * (s[j] + o.b[o.k0 + j]) + o.B[o.k0 + j]);
    return;
  }
  double bv = -INFINITY;
  int    bk = o.k0;
#pragma unroll
  for (int j = 0; j < KC; j++)
    if (j < o.kc) {
      const double t = s[j] + o.b[o.k0 + j];
      if (o.scores) o.scores[(size_t)i * o.K + o.k0 + j] = t;
      if (t > bv) bv = t, bk = o.k0 + j;
    }
  if (o.labels) svmm_label(o, i, bv, bk);
}

// The halving butterfly: each of LW lanes (l = the lane's index among them) holds KC partial sums; returns the full sum of class l / (LW / KC) in every
// lane.  KC / 2 + KC / 4 + .. + 1 shuffles to one class per lane, then log2(LW / KC) to complete it
template <int KC, int LW> static __device__ __forceinline__ double svmm_halve(double (&s)[KC], int l)
{
  static_assert((KC & (KC - 1)) == 0 && KC <= LW, "SVMM_KC: a power of two, at most the lanes of a row");
#pragma unroll
  for (int m = KC / 2, off = LW / 2; m >= 1; m >>= 1, off >>= 1) {
    const bool up = (l & off) != 0;
#pragma unroll
    for (int j = 0; j < m; j++) {
      const double give = up ? s[j] : s[j + m], keep = up ? s[j + m] : s[j];
      s[j] = keep + __shfl_xor(give, off, 64);
    }
  }
  double t = s[0];
#pragma unroll
  for (int off = LW / KC / 2; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
  return t;
}

// the LW lanes of row i after svmm_halve: lane l holds t = the sum of the chunk's class l / (LW / KC).  Every lane of the wavefront calls this (shuffles);
// live: the row exists.  ca, cb: the Platt pair of the lane's class (svmm_lane_cal; the probability instances)
template <int KC, int LW, class OUT> static __device__ __forceinline__ void svmm_lanes_done(const OUT &o, long long i, bool live, int l, double t, double bc, double ca, double cb)
{
  constexpr int LPC = LW / KC; // lanes per class
  const int     c   = l / LPC;
  t += bc;
  if constexpr (OUT::PROBA) {
    if (live && (l % LPC) == 0 && c < o.kc) o.scores[(size_t)i * o.K + o.k0 + c] = svm_sigmoid(ca * t + cb);
    return;
  }
  if (o.labels) { // (uniform: a kernel argument)
    double bv = c < o.kc ? t : -INFINITY;
    int    bk = o.k0 + c;
#pragma unroll
    for (int off = LPC; off < LW; off <<= 1) {
      const double v2 = __shfl_xor(bv, off, 64);
      const int    k2 = __shfl_xor(bk, off, 64);
      if (v2 > bv || (v2 == bv && k2 < bk)) bv = v2, bk = k2;
    }
    if (live && l == 0) svmm_label(o, i, bv, bk);
  }
  if (o.scores && live && (l % LPC) == 0 && c < o.kc) o.scores[(size_t)i * o.K + o.k0 + c] = t;
}

// A row selector on the two dense sweeps (pmh_svm_multi_test_own: the held-out rows or the subset of the handle's own samples): the template argument SEL and
// sel, n doubles, non-zero = the row is selected.  SEL = 0: sel is not read and the code is the sweep without a selector.  SEL = 1: the selector is read before
// anything of the row; a row that is not selected is not loaded and nothing is stored for it, neither score nor label nor best.  A selected row gets the bits
// of the SEL = 0 instance: the same loads, products and butterflies, in which every lane takes part whatever its row is.  Instantiated for svmm_out only.
// d == 64: W is the model (K x 64, row-major).  SEL: the selectors of the 2 UNR rows in flight come in ONE coalesced load and a ballot (svm_live_rows64); a
// row group without a selected row is passed over (uniform over the wave: the ballot)
template <int KC, int UNR, class OUT, int SEL = 0>
__global__ __launch_bounds__(PMH_BLOCK) void k_svmm_rows64(int n, const double *__restrict__ X, const double *__restrict__ W, OUT o, const double *__restrict__ sel = nullptr)
{
  static_assert(!SEL || !OUT::PROBA, "the row selector is for the scoring instances");
  const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l2 = lane & 31;
  const long long gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  dbl2            wr[KC];
#pragma unroll
  for (int c = 0; c < KC; c++) wr[c] = c < o.kc ? ((const dbl2 *)(W + (size_t)(o.k0 + c) * 64))[l2] : dbl2{0.0, 0.0};
  const int    myc = l2 / (32 / KC);
  const double bc  = myc < o.kc ? o.b[o.k0 + myc] : 0.0;
  double       ca, cb;
  svmm_lane_cal(o, myc, ca, cb);
  for (long long r0 = gw * 2 * UNR; r0 < n; r0 += nw * 2 * UNR) {
    dbl2               v[UNR];
    unsigned long long live = ~0ull; // SEL: bit j says that row r0 + j is selected (0 past the last row)
    if constexpr (SEL) {
      double si;
      live = svm_live_rows64<2 * UNR>(n, sel, r0, si);
      svm_load_rows64<UNR, 1>(n, X, r0, v, live);
    } else svm_load_rows64<UNR>(n, X, r0, v);
    const unsigned lh = SEL ? (unsigned)(live >> half) : ~0u; // bit 2 u: this lane's row of group u is selected (shifted once: a constant bit per u)
#pragma unroll
    for (int u = 0; u < UNR; u++) {
      if (SEL && !((live >> (2 * u)) & 3)) continue; // (uniform over the wave)
      const long long i = r0 + 2 * u + half;
      double          s[KC];
#pragma unroll
      for (int c = 0; c < KC; c++) s[c] = v[u].x * wr[c].x + v[u].y * wr[c].y;
      const double t = svmm_halve<KC, 32>(s, l2);
      svmm_lanes_done<KC, 32>(o, i, i < n && ((lh >> (2 * u)) & 1), l2, t, bc, ca, cb);
    }
  }
}

// any d <= 64 SVM_KMAX: W is the model (K x d, row-major).  SEL: the row's selector is uniform over the wave that owns the row, as the masked label is in
// svm_sweep_rows
template <int KC, class OUT, int SEL = 0>
__global__ __launch_bounds__(PMH_BLOCK) void k_svmm_rows(int n, int d, const double *__restrict__ X, const double *__restrict__ W, OUT o, const double *__restrict__ sel = nullptr)
{
  static_assert(!SEL || !OUT::PROBA, "the row selector is for the scoring instances");
  const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  double          wr[KC][SVM_KMAX];
#pragma unroll
  for (int c = 0; c < KC; c++)
#pragma unroll
    for (int k = 0; k < SVM_KMAX; k++) wr[c][k] = (c < o.kc && lane + 64 * k < d) ? W[(size_t)(o.k0 + c) * d + lane + 64 * k] : 0.0;
  const int    myc = lane / (64 / KC);
  const double bc  = myc < o.kc ? o.b[o.k0 + myc] : 0.0;
  double       ca, cb;
  svmm_lane_cal(o, myc, ca, cb);
  for (long long i = gw; i < n; i += nw) {
    if (SEL && sel[i] == 0.0) continue; // (uniform over the wave)
    const double *xr = X + (size_t)i * d;
    double        x[SVM_KMAX], s[KC];
#pragma unroll
    for (int k = 0; k < SVM_KMAX; k++) x[k] = (lane + 64 * k < d) ? __builtin_nontemporal_load(&xr[lane + 64 * k]) : 0.0;
#pragma unroll
    for (int c = 0; c < KC; c++) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < SVM_KMAX; k++) a += x[k] * wr[c][k];
      s[c] = a;
    }
    const double t = svmm_halve<KC, 64>(s, lane);
    svmm_lanes_done<KC, 64>(o, i, true, lane, t, bc, ca, cb);
  }
}

// CSR: span b's pieces of the samples' KC sums (svc_segments; Wt: d x KC, class index fastest; head / tail: KC doubles per span)
template <int KC, class OUT>
__global__ __launch_bounds__(PMH_BLOCK) void k_svmm_seg(int nent, int nseg, int nb, const int *__restrict__ ptr, const int *__restrict__ idx, const double *__restrict__ val, const double *__restrict__ Wt,
                                                        const int *__restrict__ first, double *__restrict__ head, double *__restrict__ tail, OUT o)
{
  __shared__ dbl2  sval2[SVC_SPAN / 2];
  __shared__ int2v sidx2[SVC_SPAN / 2];
  const int        b = blockIdx.x, start = b * SVC_SPAN, end = min(start + SVC_SPAN, nent);
  // the span's values and indices (entries past the end: 0, column 0, never read)
#pragma unroll
  for (int j = 0; j < SVC_SPAN / PMH_BLOCK / 2; j++) {
    const int q = j * PMH_BLOCK + (int)threadIdx.x;
    dbl2      v;
    int2v     ix;
    svc_load_pair(j, start, end, val, idx, v, ix);
    sval2[q] = v, sidx2[q] = ix;
  }
  __syncthreads();
  const double *sval = (const double *)sval2;
  const int    *sidx = (const int *)sidx2;
  svc_segments<KC>(
    b, nb, nseg, start, end, ptr, first, head, tail,
    [&](int k, double(&s)[KC]) { // two classes per load of the entry's row of Wt
      const double xv = sval[k];
      const dbl2  *wr = (const dbl2 *)(Wt + (size_t)sidx[k] * KC);
#pragma unroll
      for (int j = 0; j < KC / 2; j++) {
        const dbl2 w2 = wr[j];
        s[2 * j] += xv * w2.x, s[2 * j + 1] += xv * w2.y;
      }
    },
    [&](int c, const double(&s)[KC]) { svmm_row_done<KC>(o, c, s); });
}

// the samples shared between spans, each completed in the span where it ends (svc_finish)
template <int KC, class OUT>
__global__ __launch_bounds__(PMH_BLOCK) void k_svmm_fin(int nent, int nseg, int nb, const int *__restrict__ ptr, const int *__restrict__ first, const double *__restrict__ head,
                                                        const double *__restrict__ tail, OUT o)
{
  svc_finish<KC>(nent, nseg, nb, ptr, first, head, tail, [&](int c, const double(&s)[KC]) { svmm_row_done<KC>(o, c, s); });
}

// mapped samples (rff_score.hip): the chunk's dot products x_i . W_k come ready in dots (n x K, row-major: the chunk's columns k0 .. k0 + kc); one thread per row
// hands them to svmm_row_done.  (no __restrict__ on dots: the scores may be written over them)
template <int KC, class OUT> __global__ __launch_bounds__(PMH_BLOCK) void k_svmm_dots(int n, const double *dots, OUT o)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    double s[KC];
#pragma unroll
    for (int j = 0; j < KC; j++) s[j] = j < o.kc ? dots[(size_t)i * o.K + o.k0 + j] : 0.0;
    svmm_row_done<KC>(o, i, s);
  }
}

// proba[i][k] /= sum_k proba[i][k], the sum taken k ascending; a row whose sum is 0 (every sigma underflowed) becomes 1 / K everywhere.  One row per thread
__global__ __launch_bounds__(PMH_BLOCK) void k_svmm_normalise(int n, int K, double *__restrict__ proba)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    double *p = proba + (size_t)i * K;
    double  s = 0.0;
    for (int k = 0; k < K; k++) s += p[k];
    for (int k = 0; k < K; k++) p[k] = s == 0.0 ? 1.0 / K : p[k] / s;
  }
}

// Wt[ch][col][j] = W[ch KC + j][col] (0 past the last class): the model as the CSR sweep gathers it
template <int KC> __global__ __launch_bounds__(PMH_BLOCK) void k_svmm_pack(int K, int d, long long total, const double *__restrict__ W, double *__restrict__ Wt)
{
  for (long long t = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * PMH_BLOCK) {
    const int       j = (int)(t % KC);
    const long long r = t / KC;
    const int       col = (int)(r % d), k = (int)(r / d) * KC + j;
    Wt[t] = k < K ? W[(size_t)k * d + col] : 0.0;
  }
}

// y_i = +1 where label_i == c, else -1: the binary problem "class c against the rest"
__global__ __launch_bounds__(PMH_BLOCK) void k_svmm_relabel(int n, const double *__restrict__ labels, double c, double *__restrict__ y)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) y[i] = labels[i] == c ? 1.0 : -1.0;
}

// the index of v in the ascending classes, or K
static __device__ __forceinline__ int svmm_class_index(int K, const double *__restrict__ classes, double v)
{
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (classes[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return (lo < K && classes[lo] == v) ? lo : K;
}
// conf[t K + p]++ for the true class t and the predicted class p of every sample; conf[K K]++ where the true label is no class (counts: integer atomics, any
// order gives the same integers).  SEL: only the samples with sel[i] != 0 (the selector of the dense sweeps); pred of any other sample is not read -- the
// dense sweeps have stored nothing there
template <int SEL = 0>
__global__ __launch_bounds__(PMH_BLOCK) void k_svmm_confusion(int n, int K, const double *__restrict__ classes, const double *__restrict__ pred, const double *__restrict__ ytrue,
                                                              unsigned long long *__restrict__ conf, const double *__restrict__ sel = nullptr)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    if (SEL && sel[i] == 0.0) continue;
    const int t = svmm_class_index(K, classes, ytrue[i]), p = svmm_class_index(K, classes, pred[i]);
    atomicAdd(&conf[(t < K && p < K) ? (size_t)t * K + p : (size_t)K * K], 1ull);
  }
}
// cnt[k]++ for the class k of every sample inside the subset (msk[i] != 0); cnt[K] stays 0: every training label is a class (integer atomics)
__global__ __launch_bounds__(PMH_BLOCK) void k_svmm_class_count(int n, int K, const double *__restrict__ classes, const double *__restrict__ labels, const double *__restrict__ msk,
                                                                unsigned long long *__restrict__ cnt)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK)
    if (msk[i] != 0.0) atomicAdd(&cnt[svmm_class_index(K, classes, labels[i])], 1ull);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------
struct pmh_svm_multi_s {
  pmh_ctx       ctx;
  int           n = 0, d = 0, K = 0, nchc = 0, balanced = 0; // nchc: chunks of the CSR sweep
  int           cur = 0; // the class the binary handle is labelled for
  pmh_svm_opts  o;
  const double *labels = nullptr; // the training labels, borrowed
  pmh_svm       bin    = nullptr; // the one binary handle over X
  double       *y = nullptr, *W = nullptr, *Wt = nullptr, *b = nullptr, *classes = nullptr; // device: n (the binary handle borrows it), K d, nch d KC, K, K
  std::vector<double>        h_classes, h_W, h_b;
  std::vector<long long>     count; // samples per class
  std::vector<pmh_svm_stats> st;    // per class, of the last pmh_svm_multi_train
  int           trained = 0, have_stats = 0;
  // pmh_svm_multi_set_subset: the mask itself is the binary handle's (pmh_svm_own_samples); here the subset's size (0: no subset), its samples per class and
  // the complement 1 - m (n doubles, device: the selector of the held-out rows; allocated by the first subset)
  long long              n_sub = 0;
  std::vector<long long> count_sub;
  double                *cmsk = nullptr;
  // the probability model of the current (W, b): the classes' Platt pairs (svm_proba.hip); a new model clears it
  int                              calibrated = 0;
  double                          *cal = nullptr; // device: A (K) then B (K)
  std::vector<double>              h_A, h_B;
  std::vector<pmh_svm_platt_stats> cal_st;
};

extern "C" int pmh_svm_multi_chunk(int path, int *KC)
{
  PMH_ARG(KC && path >= 0 && path <= 2);
  *KC = path == 0 ? SVMM_KC64 : (path == 1 ? SVMM_KCD : SVMM_KCC);
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_multi_destroy(pmh_svm_multi m)
{
  if (!m) return PMH_SUCCESS;
  if (m->bin) pmh_svm_destroy(m->bin);
  double *v[] = {m->y, m->W, m->Wt, m->b, m->classes, m->cal, m->cmsk};
  for (double *p : v)
    if (p) pmh_free(m->ctx, p);
  delete m;
  return PMH_SUCCESS;
}

static int svmm_relabel(pmh_svm_multi m, int k)
{
  if (m->n > 0) hipLaunchKernelGGL(k_svmm_relabel, dim3(pmh_vec_grid(m->n)), dim3(PMH_BLOCK), 0, m->ctx->stream, m->n, m->labels, m->h_classes[(size_t)k], m->y);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

static int svmm_create(pmh_ctx ctx, int n, int d, const double *X_dev, pmh_csr Xcsr, const double *labels_dev, const pmh_svm_opts *opts, int balanced, pmh_svm_multi *out)
{
  const char *who = Xcsr ? "pmh_svm_multi_create_csr" : "pmh_svm_multi_create";
  if (pmh_comm_on(ctx)) return pmh_set_error(PMH_ERR_ARG, "%s: a communicator is on; the one-vs-rest front end runs on one GPU", who);
  std::vector<double> lab((size_t)n);
  if (n > 0) PMH_CHK(pmh_memcpy_d2h(ctx, lab.data(), labels_dev, sizeof(double) * lab.size()));
  for (int i = 0; i < n; i++)
    if (!std::isfinite(lab[(size_t)i])) return pmh_set_error(PMH_ERR_ARG, "%s: the label of sample %d is not finite", who, i);
  std::vector<double> cls(lab);
  std::sort(cls.begin(), cls.end());
  cls.erase(std::unique(cls.begin(), cls.end()), cls.end());
  if (cls.size() < 2) return pmh_set_error(PMH_ERR_ARG, "%s: %d distinct labels, a classifier needs at least two", who, (int)cls.size());
  pmh_svm_multi m = new pmh_svm_multi_s();
  m->ctx = ctx, m->n = n, m->d = d, m->K = (int)cls.size(), m->nchc = (m->K + SVMM_KCC - 1) / SVMM_KCC, m->balanced = balanced ? 1 : 0, m->o = *opts, m->labels = labels_dev;
  m->h_classes = cls;
  m->count.assign((size_t)m->K, 0);
  for (int i = 0; i < n; i++) m->count[(size_t)(std::lower_bound(cls.begin(), cls.end(), lab[(size_t)i]) - cls.begin())]++;
  m->h_W.assign((size_t)m->K * d, 0.0), m->h_b.assign((size_t)m->K, 0.0);
  m->st.resize((size_t)m->K);
  m->h_A.assign((size_t)m->K, 0.0), m->h_B.assign((size_t)m->K, 0.0), m->cal_st.resize((size_t)m->K);
  int rc = PMH_SUCCESS;
  do {
    if ((rc = pmh_malloc(ctx, sizeof(double) * (size_t)n, (void **)&m->y)) || (rc = pmh_malloc(ctx, sizeof(double) * (size_t)m->K * d, (void **)&m->W)) ||
        (rc = pmh_malloc(ctx, sizeof(double) * (size_t)m->nchc * d * SVMM_KCC, (void **)&m->Wt)) || (rc = pmh_malloc(ctx, sizeof(double) * (size_t)m->K, (void **)&m->b)) ||
        (rc = pmh_malloc(ctx, sizeof(double) * (size_t)m->K, (void **)&m->classes)) || (rc = pmh_malloc(ctx, sizeof(double) * 2 * (size_t)m->K, (void **)&m->cal)))
      break;
    if ((rc = pmh_memcpy_h2d(ctx, m->classes, cls.data(), sizeof(double) * cls.size()))) break;
    if ((rc = svmm_relabel(m, 0))) break; // the binary handle is created on the labels of class 0
    rc = Xcsr ? pmh_svm_create_csr(ctx, Xcsr, m->y, opts, &m->bin) : pmh_svm_create(ctx, n, d, X_dev, m->y, opts, &m->bin);
  } while (0);
  if (rc) {
    pmh_svm_multi_destroy(m);
    return rc;
  }
  *out = m;
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_multi_create(pmh_ctx ctx, int n, int d, const double *X_dev, const double *labels_dev, const pmh_svm_opts *opts, int balanced, pmh_svm_multi *out)
{
  PMH_ARG(ctx && out && opts && n >= 1 && d >= 1 && d <= 64 * SVM_KMAX && X_dev && labels_dev);
  return svmm_create(ctx, n, d, X_dev, nullptr, labels_dev, opts, balanced, out);
}

extern "C" int pmh_svm_multi_create_csr(pmh_ctx ctx, pmh_csr X, const double *labels_dev, const pmh_svm_opts *opts, int balanced, pmh_svm_multi *out)
{
  PMH_ARG(ctx && out && opts && X && labels_dev && X->ctx == ctx && X->nrows >= 1);
  if (X->ncols < 1) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_multi_create_csr: the sample matrix has no columns");
  return svmm_create(ctx, X->nrows, X->ncols, nullptr, X, labels_dev, opts, balanced, out);
}

// the penalties of the binary problem of class k: the counts over the samples that train, n_S and n_{k,S} under a subset
static void svmm_penalties(pmh_svm_multi m, int k, double *C_pos, double *C_neg)
{
  const double C = m->o.C, n = (double)(m->n_sub ? m->n_sub : m->n), nk = (double)(m->n_sub ? m->count_sub[(size_t)k] : m->count[(size_t)k]);
  *C_pos = m->balanced ? C * n / (2.0 * nk) : C;
  *C_neg = m->balanced ? C * n / (2.0 * (n - nk)) : C;
}

// the host model -> W, b and the CSR sweep's Wt on the device
static int svmm_upload_model(pmh_svm_multi m)
{
  PMH_CHK(pmh_memcpy_h2d(m->ctx, m->W, m->h_W.data(), sizeof(double) * m->h_W.size()));
  PMH_CHK(pmh_memcpy_h2d(m->ctx, m->b, m->h_b.data(), sizeof(double) * m->h_b.size()));
  const long long total = (long long)m->nchc * m->d * SVMM_KCC, nbl = (total + PMH_BLOCK - 1) / PMH_BLOCK;
  hipLaunchKernelGGL(k_svmm_pack<SVMM_KCC>, dim3((unsigned)std::min<long long>(nbl, PMH_MAX_VEC_BLOCKS)), dim3(PMH_BLOCK), 0, m->ctx->stream, m->K, m->d, total, (const double *)m->W, m->Wt);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_multi_train(pmh_svm_multi m)
{
  PMH_ARG(m);
  m->trained = m->have_stats = m->calibrated = 0;
  for (int k = 0; k < m->K; k++) {
    if (k != m->cur) { // (a fresh handle is labelled for class 0 already)
      m->cur = -1;
      PMH_CHK(svmm_relabel(m, k)); // into the buffer the handle borrows already
      PMH_CHK(pmh_svm_set_labels(m->bin, m->y));
      m->cur = k;
    }
    if (m->balanced) {
      double cp, cn;
      svmm_penalties(m, k, &cp, &cn);
      PMH_CHK(pmh_svm_set_penalties(m->bin, cp, cn, nullptr));
    }
    PMH_CHK(pmh_svm_train(m->bin));
    PMH_CHK(pmh_svm_get_model(m->bin, m->h_W.data() + (size_t)k * m->d, &m->h_b[(size_t)k]));
    PMH_CHK(pmh_svm_get_stats(m->bin, &m->st[(size_t)k]));
  }
  PMH_CHK(svmm_upload_model(m));
  m->trained = m->have_stats = 1;
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_multi_get_classes(pmh_svm_multi m, int *K, double *classes_host)
{
  PMH_ARG(m);
  if (K) *K = m->K;
  if (classes_host) memcpy(classes_host, m->h_classes.data(), sizeof(double) * (size_t)m->K);
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_multi_get_model(pmh_svm_multi m, double *W_host, double *b_host)
{
  PMH_ARG(m);
  if (!m->trained) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_multi_get_model: call pmh_svm_multi_train or pmh_svm_multi_set_model first");
  if (W_host) memcpy(W_host, m->h_W.data(), sizeof(double) * m->h_W.size());
  if (b_host) memcpy(b_host, m->h_b.data(), sizeof(double) * m->h_b.size());
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_multi_set_model(pmh_svm_multi m, const double *W_host, const double *b_host)
{
  PMH_ARG(m && W_host && b_host);
  m->trained = m->have_stats = m->calibrated = 0;
  memcpy(m->h_W.data(), W_host, sizeof(double) * m->h_W.size());
  memcpy(m->h_b.data(), b_host, sizeof(double) * m->h_b.size());
  PMH_CHK(svmm_upload_model(m));
  m->trained = 1;
  return PMH_SUCCESS;
}

// ---- sample subsets ----------------------------------------------------------------------------------------------------------------------------------------
// Train the K problems on the subset S of the handle's samples (the binary handle's pmh_svm_set_subset, which pmh_svm_set_labels and pmh_svm_set_penalties
// keep).  The classes stay those of all training labels; a class without a sample in S is refused before anything changes, as is whatever the binary handle
// refuses, which changes nothing either
extern "C" int pmh_svm_multi_set_subset(pmh_svm_multi m, const double *m_dev)
{
  PMH_ARG(m);
  pmh_ctx ctx = m->ctx;
  const int n = m->n, K = m->K;
  if (!m_dev) {
    PMH_CHK(pmh_svm_set_subset(m->bin, nullptr));
    m->n_sub = 0, m->count_sub.clear();
    m->trained = m->have_stats = m->calibrated = 0;
    return PMH_SUCCESS;
  }
  std::vector<long long> cnt((size_t)K + 1, 0);
  unsigned long long    *d_cnt = nullptr;
  PMH_CHK(pmh_malloc(ctx, sizeof(unsigned long long) * cnt.size(), (void **)&d_cnt));
  int rc = pmh_memset(ctx, d_cnt, 0, sizeof(unsigned long long) * cnt.size());
  if (!rc) {
    hipLaunchKernelGGL(k_svmm_class_count, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, K, (const double *)m->classes, m->labels, m_dev, d_cnt);
    if (hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "pmh_svm_multi_set_subset: the launch that counts the classes failed");
  }
  if (!rc) rc = pmh_memcpy_d2h(ctx, cnt.data(), d_cnt, sizeof(long long) * cnt.size());
  pmh_free(ctx, d_cnt);
  PMH_CHK(rc);
  for (int k = 0; k < K; k++)
    if (cnt[(size_t)k] == 0)
      return pmh_set_error(PMH_ERR_ARG, "pmh_svm_multi_set_subset: the subset holds no sample of class %g (class %d of %d): its problem against the rest has no positive sample", m->h_classes[(size_t)k],
                           k, K);
  if (!m->cmsk) PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)n, (void **)&m->cmsk));
  PMH_CHK(pmh_svm_set_subset(m->bin, m_dev)); // (checks the mask before anything changes)
  m->trained = m->have_stats = m->calibrated = 0;
  cnt.resize((size_t)K);
  m->count_sub = cnt;
  m->n_sub     = 0;
  for (long long c : cnt) m->n_sub += c;
  // the selector of the held-out rows: 1 - m from the mask the binary handle holds now
  const double *msk = nullptr;
  pmh_svm_own_samples(m->bin, nullptr, nullptr, nullptr, &msk);
  PMH_CHK(pmh_vec_set(ctx, n, m->cmsk, 1.0));
  return pmh_vec_axpy(ctx, n, m->cmsk, -1.0, msk);
}

extern "C" int pmh_svm_multi_get_subset(pmh_svm_multi m, double *m_dev, long long *n_in, long long *class_counts_host)
{
  PMH_ARG(m);
  if (m_dev) PMH_CHK(pmh_svm_get_subset(m->bin, m_dev, nullptr));
  if (n_in) *n_in = m->n_sub ? m->n_sub : m->n;
  if (class_counts_host) memcpy(class_counts_host, (m->n_sub ? m->count_sub : m->count).data(), sizeof(long long) * (size_t)m->K);
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_multi_get_stats(pmh_svm_multi m, int k, pmh_svm_stats *st, double *C_pos, double *C_neg)
{
  PMH_ARG(m && k >= 0 && k < m->K);
  if (st) {
    if (!m->have_stats) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_multi_get_stats: call pmh_svm_multi_train first (a model that was set has no statistics)");
    *st = m->st[(size_t)k];
  }
  double cp, cn;
  svmm_penalties(m, k, &cp, &cn);
  if (C_pos) *C_pos = cp;
  if (C_neg) *C_neg = cn;
  return PMH_SUCCESS;
}

// the launches of one chunk of classes on the instances of OUT.  sel (dense rows, scoring only): the SEL = 1 instances, which sweep the selected rows alone
template <class OUT> static void svmm_launch_chunk(pmh_svm_multi m, int n, const double *X, pmh_csr Xt, const svc_tab &t, int ch, const OUT &o, const double *sel = nullptr)
{
  pmh_ctx ctx = m->ctx;
  if constexpr (!OUT::PROBA) {
    if (!Xt && sel) {
      if (m->d == 64) hipLaunchKernelGGL((k_svmm_rows64<SVMM_KC64, 4, OUT, 1>), dim3(SVM_NB(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, X, (const double *)m->W, o, sel);
      else hipLaunchKernelGGL((k_svmm_rows<SVMM_KCD, OUT, 1>), dim3(SVM_NB(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, m->d, X, (const double *)m->W, o, sel);
      return;
    }
  }
  if (Xt) {
    const int nb = t.nb;
    hipLaunchKernelGGL((k_svmm_seg<SVMM_KCC, OUT>), dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, (int)Xt->nnz, n, nb, (const int *)Xt->d_rowptr, (const int *)Xt->d_col, (const double *)Xt->d_val,
                       (const double *)(m->Wt + (size_t)ch * m->d * SVMM_KCC), (const int *)t.first, t.head, t.tail, o);
    hipLaunchKernelGGL((k_svmm_fin<SVMM_KCC, OUT>), dim3((nb + PMH_BLOCK / 64 - 1) / (PMH_BLOCK / 64)), dim3(PMH_BLOCK), 0, ctx->stream, (int)Xt->nnz, n, nb, (const int *)Xt->d_rowptr, (const int *)t.first,
                       (const double *)t.head, (const double *)t.tail, o);
  } else if (m->d == 64) hipLaunchKernelGGL((k_svmm_rows64<SVMM_KC64, 4, OUT>), dim3(SVM_NB(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, X, (const double *)m->W, o);
  else hipLaunchKernelGGL((k_svmm_rows<SVMM_KCD, OUT>), dim3(SVM_NB(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, m->d, X, (const double *)m->W, o);
}

// X (dense rows, n x d) or Xt (CSR): one sweep per chunk of classes, chunks ascending.  proba: scores receives the classes' sigmoids (m->cal), labels is nullptr
// sel (n doubles, or nullptr: every row): dense rows are swept, and scores, labels and best written, only where sel[i] != 0; CSR has no row skipping, as on
// the binary handle: every stored entry is swept and every row written, and the selection is k_svmm_confusion's alone
// mp: mapped samples (then X and Xt are nullptr): all K dot products of a row by one pmh_rffdots into a buffer of the call, then k_svmm_dots per chunk
static int svmm_predict(pmh_svm_multi m, int n, const double *X, pmh_csr Xt, double *scores, double *labels, bool proba = false, const double *sel = nullptr, const sv_mapped *mp = nullptr)
{
  PMH_ARG(m && n >= 0 && (X || Xt || n == 0 || mp));
  if (!m->trained) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_multi_predict: call pmh_svm_multi_train or pmh_svm_multi_set_model first");
  if (mp) PMH_CHK(sv_check_mapped("pmh_svm_multi_predict", *mp, n, m->d));
  else PMH_CHK(pmh_svm_check_test_samples("pmh_svm_multi_predict", m->d, Xt));
  if (n == 0 || (!scores && !labels)) return PMH_SUCCESS;
  pmh_ctx ctx  = m->ctx;
  double *best = nullptr, *dots = nullptr;
  const int kcp = (mp || Xt) ? SVMM_KCC : (m->d == 64 ? SVMM_KC64 : SVMM_KCD), nch = (m->K + kcp - 1) / kcp; // the path's chunk
  if (labels && nch > 1) PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)n, (void **)&best));
  svc_tab t;
  int     rc = Xt ? svc_tab_build(ctx, n, Xt->d_rowptr, Xt->nnz, &t, SVMM_KCC) : PMH_SUCCESS;
  if (mp && !rc) rc = pmh_malloc(ctx, sizeof(double) * (size_t)n * m->K, (void **)&dots);
  if (mp && !rc) rc = pmh_rffdots(mp->map, n, mp->X, mp->x_type, m->K, m->W, m->d, dots);
  for (int ch = 0; ch < nch && !rc; ch++) {
    svmm_out o{m->K, ch * kcp, std::min(kcp, m->K - ch * kcp), m->b, m->classes, scores, labels, best};
    if (proba) {
      svmm_out_proba op;
      static_cast<svmm_out &>(op) = o;
      op.A = m->cal, op.B = m->cal + m->K;
      if (mp) hipLaunchKernelGGL((k_svmm_dots<SVMM_KCC, svmm_out_proba>), dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, (const double *)dots, op);
      else svmm_launch_chunk(m, n, X, Xt, t, ch, op);
    } else if (mp) hipLaunchKernelGGL((k_svmm_dots<SVMM_KCC, svmm_out>), dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, (const double *)dots, o);
    else svmm_launch_chunk(m, n, X, Xt, t, ch, o, sel);
    if (hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "pmh_svm_multi_predict: the launch failed");
  }
  if (Xt) svc_tab_free(ctx, &t); // (waits for the stream)
  if (dots) pmh_free(ctx, dots); // (waits for the stream)
  if (best) pmh_free(ctx, best);
  return rc;
}

extern "C" int pmh_svm_multi_predict(pmh_svm_multi m, int n, const double *X_dev, double *scores_dev, double *labels_dev) { return svmm_predict(m, n, X_dev, nullptr, scores_dev, labels_dev); }

extern "C" int pmh_svm_multi_predict_csr(pmh_svm_multi m, pmh_csr Xt, double *scores_dev, double *labels_dev)
{
  PMH_ARG(m && Xt);
  return svmm_predict(m, Xt->nrows, nullptr, Xt, scores_dev, labels_dev);
}

// sel: the rows that are scored (dense) and counted, or nullptr: every row
static int svmm_test(pmh_svm_multi m, int n, const double *X, pmh_csr Xt, const double *ytrue, long long *confusion, long long *n_unknown, const double *sel = nullptr, const sv_mapped *mp = nullptr)
{
  PMH_ARG(m && ytrue && confusion && n >= 0);
  pmh_ctx             ctx = m->ctx;
  const size_t        nc  = (size_t)m->K * m->K + 1;
  double             *pred = nullptr;
  unsigned long long *conf = nullptr;
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)(n ? n : 1), (void **)&pred));
  int rc = pmh_malloc(ctx, sizeof(unsigned long long) * nc, (void **)&conf);
  if (!rc) rc = pmh_memset(ctx, conf, 0, sizeof(unsigned long long) * nc);
  if (!rc) rc = svmm_predict(m, n, X, Xt, nullptr, pred, false, sel, mp);
  if (!rc && n > 0) {
    if (sel) hipLaunchKernelGGL(k_svmm_confusion<1>, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, m->K, (const double *)m->classes, (const double *)pred, ytrue, conf, sel);
    else hipLaunchKernelGGL(k_svmm_confusion<0>, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, m->K, (const double *)m->classes, (const double *)pred, ytrue, conf);
    if (hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "pmh_svm_multi_test: the launch failed");
  }
  std::vector<long long> h(nc, 0);
  if (!rc) rc = pmh_memcpy_d2h(ctx, h.data(), conf, sizeof(long long) * nc);
  pmh_free(ctx, pred);
  if (conf) pmh_free(ctx, conf);
  PMH_CHK(rc);
  memcpy(confusion, h.data(), sizeof(long long) * (nc - 1));
  if (n_unknown) *n_unknown = h[nc - 1];
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_multi_test(pmh_svm_multi m, int n, const double *X_dev, const double *labels_true_dev, long long *confusion, long long *n_unknown)
{
  return svmm_test(m, n, X_dev, nullptr, labels_true_dev, confusion, n_unknown);
}

extern "C" int pmh_svm_multi_test_csr(pmh_svm_multi m, pmh_csr Xt, const double *labels_true_dev, long long *confusion, long long *n_unknown)
{
  PMH_ARG(m && Xt);
  return svmm_test(m, Xt->nrows, nullptr, Xt, labels_true_dev, confusion, n_unknown);
}

// ---- the handle's own samples ------------------------------------------------------------------------------------------------------------------------------
// nothing uploaded: the scoring sweeps over the X the binary handle borrows, or over the handle's own pmh_csr
extern "C" int pmh_svm_multi_predict_own(pmh_svm_multi m, double *scores_dev, double *labels_dev)
{
  PMH_ARG(m);
  const void *X    = nullptr;
  pmh_csr     Xcsr = nullptr;
  pmh_svm_own_samples(m->bin, &X, nullptr, &Xcsr, nullptr);
  return svmm_predict(m, m->n, (const double *)X, Xcsr, scores_dev, labels_dev);
}

// the confusion matrix of the own samples against the training labels over the held-out rows, the subset or all rows.  Dense: the unselected rows of X are
// not loaded (the SEL = 1 sweeps); CSR: all rows are scored and the confusion kernel selects
extern "C" int pmh_svm_multi_test_own(pmh_svm_multi m, int which, long long *confusion, long long *n_counted)
{
  PMH_ARG(m && confusion);
  if (which != PMH_SVM_OWN_HELD_OUT && which != PMH_SVM_OWN_SUBSET && which != PMH_SVM_OWN_ALL)
    return pmh_set_error(PMH_ERR_ARG, "pmh_svm_multi_test_own: which = %d (PMH_SVM_OWN_HELD_OUT | PMH_SVM_OWN_SUBSET | PMH_SVM_OWN_ALL)", which);
  const void   *X    = nullptr;
  pmh_csr       Xcsr = nullptr;
  const double *msk  = nullptr;
  pmh_svm_own_samples(m->bin, &X, nullptr, &Xcsr, &msk);
  if (which == PMH_SVM_OWN_HELD_OUT && !msk) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_multi_test_own: no subset is set (pmh_svm_multi_set_subset), so no sample is held out");
  const double *sel = (which == PMH_SVM_OWN_ALL || !msk) ? nullptr : (which == PMH_SVM_OWN_SUBSET ? msk : (const double *)m->cmsk);
  long long     unk = 0;
  PMH_CHK(svmm_test(m, m->n, (const double *)X, Xcsr, m->labels, confusion, &unk, sel));
  if (n_counted) {
    *n_counted = unk; // (0: every training label is a class)
    for (size_t j = 0; j < (size_t)m->K * m->K; j++) *n_counted += confusion[j];
  }
  return PMH_SUCCESS;
}

// ---- probabilities (Platt scaling, svm_proba.hip) ---------------------------------------------------------------------------------------------------------------
static int svmm_upload_cal(pmh_svm_multi m)
{
  PMH_CHK(pmh_memcpy_h2d(m->ctx, m->cal, m->h_A.data(), sizeof(double) * (size_t)m->K));
  return pmh_memcpy_h2d(m->ctx, m->cal + m->K, m->h_B.data(), sizeof(double) * (size_t)m->K);
}

// one scoring call for all K classes, then fit k on column k of the scores in place, "label == class k" against the rest
static int svmm_calibrate(pmh_svm_multi m, int n, const double *X, pmh_csr Xt, const double *labels, const sv_mapped *mp = nullptr)
{
  PMH_ARG(m && n >= 0 && (labels || n == 0));
  if (!m->trained) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_multi_calibrate: call pmh_svm_multi_train or pmh_svm_multi_set_model first");
  m->calibrated  = 0;
  double *scores = nullptr;
  PMH_CHK(pmh_malloc(m->ctx, sizeof(double) * (size_t)(n ? n : 1) * m->K, (void **)&scores));
  int rc = svmm_predict(m, n, X, Xt, scores, nullptr, false, nullptr, mp);
  for (int k = 0; k < m->K && !rc; k++)
    rc = pmh_svm_platt_fit_strided(m->ctx, n, scores + k, m->K, labels, m->h_classes[(size_t)k], 0, &m->h_A[(size_t)k], &m->h_B[(size_t)k], &m->cal_st[(size_t)k]);
  pmh_free(m->ctx, scores);
  PMH_CHK(rc);
  PMH_CHK(svmm_upload_cal(m));
  m->calibrated = 1;
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_multi_calibrate(pmh_svm_multi m, int n, const double *X_dev, const double *labels_dev) { return svmm_calibrate(m, n, X_dev, nullptr, labels_dev); }

extern "C" int pmh_svm_multi_calibrate_csr(pmh_svm_multi m, pmh_csr Xt, const double *labels_dev)
{
  PMH_ARG(m && Xt);
  return svmm_calibrate(m, Xt->nrows, nullptr, Xt, labels_dev);
}

extern "C" int pmh_svm_multi_set_calibration(pmh_svm_multi m, const double *A_host, const double *B_host)
{
  PMH_ARG(m && A_host && B_host);
  if (!m->trained) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_multi_set_calibration: call pmh_svm_multi_train or pmh_svm_multi_set_model first (a calibration belongs to a model)");
  for (int k = 0; k < m->K; k++)
    if (!std::isfinite(A_host[k]) || !std::isfinite(B_host[k])) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_multi_set_calibration: class %d: A = %g, B = %g, both must be finite", k, A_host[k], B_host[k]);
  m->calibrated = 0;
  memcpy(m->h_A.data(), A_host, sizeof(double) * (size_t)m->K);
  memcpy(m->h_B.data(), B_host, sizeof(double) * (size_t)m->K);
  memset(m->cal_st.data(), 0, sizeof(pmh_svm_platt_stats) * (size_t)m->K);
  PMH_CHK(svmm_upload_cal(m));
  m->calibrated = 1;
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_multi_get_calibration(pmh_svm_multi m, double *A_host, double *B_host, pmh_svm_platt_stats *st_host)
{
  PMH_ARG(m);
  if (!m->calibrated) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_multi_get_calibration: call pmh_svm_multi_calibrate or pmh_svm_multi_set_calibration first");
  if (A_host) memcpy(A_host, m->h_A.data(), sizeof(double) * (size_t)m->K);
  if (B_host) memcpy(B_host, m->h_B.data(), sizeof(double) * (size_t)m->K);
  if (st_host) memcpy(st_host, m->cal_st.data(), sizeof(pmh_svm_platt_stats) * (size_t)m->K);
  return PMH_SUCCESS;
}

static int svmm_predict_proba(pmh_svm_multi m, int n, const double *X, pmh_csr Xt, double *proba, const sv_mapped *mp = nullptr)
{
  PMH_ARG(m && (proba || n == 0));
  if (m->trained && !m->calibrated) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_multi_predict_proba: call pmh_svm_multi_calibrate or pmh_svm_multi_set_calibration first");
  PMH_CHK(svmm_predict(m, n, X, Xt, proba, nullptr, true, nullptr, mp));
  if (n > 0) {
    hipLaunchKernelGGL(k_svmm_normalise, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, m->ctx->stream, n, m->K, proba);
    PMH_HIP(hipGetLastError());
  }
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_multi_predict_proba(pmh_svm_multi m, int n, const double *X_dev, double *proba_dev) { return svmm_predict_proba(m, n, X_dev, nullptr, proba_dev); }

extern "C" int pmh_svm_multi_predict_proba_csr(pmh_svm_multi m, pmh_csr Xt, double *proba_dev)
{
  PMH_ARG(m && Xt);
  return svmm_predict_proba(m, Xt->nrows, nullptr, Xt, proba_dev);
}

// ---- mapped samples (rff_score.hip) -------------------------------------------------------------------------------------------------------------------------------
extern "C" int pmh_svm_multi_predict_rff(pmh_svm_multi m, pmh_rff map, int n, const void *X_dev, int x_type, double *scores_dev, double *labels_dev)
{
  const sv_mapped mp{map, X_dev, x_type};
  return svmm_predict(m, n, nullptr, nullptr, scores_dev, labels_dev, false, nullptr, &mp);
}
extern "C" int pmh_svm_multi_test_rff(pmh_svm_multi m, pmh_rff map, int n, const void *X_dev, int x_type, const double *labels_true_dev, long long *confusion, long long *n_unknown)
{
  const sv_mapped mp{map, X_dev, x_type};
  return svmm_test(m, n, nullptr, nullptr, labels_true_dev, confusion, n_unknown, nullptr, &mp);
}
extern "C" int pmh_svm_multi_calibrate_rff(pmh_svm_multi m, pmh_rff map, int n, const void *X_dev, int x_type, const double *labels_dev)
{
  const sv_mapped mp{map, X_dev, x_type};
  return svmm_calibrate(m, n, nullptr, nullptr, labels_dev, &mp);
}
extern "C" int pmh_svm_multi_predict_proba_rff(pmh_svm_multi m, pmh_rff map, int n, const void *X_dev, int x_type, double *proba_dev)
{
  const sv_mapped mp{map, X_dev, x_type};
  return svmm_predict_proba(m, n, nullptr, nullptr, proba_dev, &mp);
}
