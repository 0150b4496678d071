// The SVM dual Hessian for samples held in CSR (fp64 values, int32 indices, n rows, any number d of columns):
//   H = diag(y) X X' diag(y) + shift I + (sigma + sigma_fold) y y',
// applied matrix-free in two sweeps over the stored entries, as the dense operator of svm.hip:
//   pass 1  w = X'(y o a)  (d doubles) and, in the augmented form, s = sum_i y_i a_i in the same sweep;
//   all-reduce of w (d or d + 1 doubles) under a communicator;
//   pass 2  (H a)_i = y_i (x_i . w) + sigma s y_i + shift a_i  (svm_aug_row; with a diagonal set, diag_i a_i: MODE 3 of the finishing step).
// Both passes, the bias pass of the model and prediction are ONE kernel pair, a segmented sum over a compressed array (ptr / idx / val): segments are the
// samples (the caller's CSR) in pass 2 and in prediction, and the features in pass 1, which runs over a column-ordered device copy built once at creation.
// The sum's code is in svm_csr_seg.h (svc_segments, svc_finish), where the K-column scoring of svm_multi.hip shares it; its description is here.
//
// Work is divided by stored entries, not by segments: workgroup b owns the SVC_SPAN entries [b SVC_SPAN, (b + 1) SVC_SPAN) (k_svc_seg).  It forms their
// products with the gathered vector in LDS, sums every segment's piece inside the span with G lanes per segment (G = 1 .. 64, from the span's mean piece
// length: a span that is one piece of a popular feature is summed by a whole wavefront, a span of three hundred rare features by one lane each) and stores
// the sums of whole segments.  The at most two pieces it shares with its neighbours (its first segment where that began earlier or goes on, its last where
// that goes on) go to head[b] / tail[b]; k_svc_fin completes every shared segment in the span where it ends: the pieces of spans b0 .. b1 in this order over the
// lanes of one wavefront (lane l takes b0 + l, b0 + l + 64, ..), then the fixed shuffle tree.  No float atomics, no order that depends on scheduling: the same
// input gives the same bits.  Segments without entries lie in exactly one span's range and get the sum 0 (an empty feature: w_c = 0; a sample without
// entries: (H a)_i = sigma s y_i + shift a_i).
//
// The column-ordered copy holds y_i x_ic (the labels are +-1: an exact sign flip), rows ascending inside a column, so pass 1 gathers a alone; one more
// column, d, holds y_i for every sample, so s = sum_i y_i a_i = w[d] is a segment like the others and a long one like the others.  The plain operator
// (shift = sigma = sigma_fold = 0) stops the sweep before that column and runs the pass-2 kernel without the extra terms (MODE 1 instead of 2).  The copy
// costs 12 (nnz + n) bytes of device memory beside the caller's matrix (8 value + 4 row index per entry); the labels are read at creation, not later.
// New labels (pmh_op_svm_dual_set_labels) re-sign the copy in place: the operator keeps the signs it built the copy with (ysign, 8 n bytes more, its own
// memory: the caller may hand over the very buffer it lent before, overwritten), and every stored value is multiplied by ysign_i y_i(new) = +-1, an exact
// sign flip, so the copy equals the one a fresh operator builds from the new labels bit for bit (k_svc_resign).
// The first segment of every span is found once, at creation, by binary search (k_svc_first): 4 bytes per span.
//
// Algorithmic bytes of one application: 24 nnz + 4 (n + d) + 8 (3 n + 2 d) (both copies' values and indices, the two pointer arrays, a, y, H a, w written
// and read); HBM-bound, the gathers of a (pass 1) and w (pass 2) are served by the caches where the vectors fit.
//
// Out of scope here: the fused MPGP epilogues of the dense d = 64 path (mult_epi, "paired passes" in svm.hip).  mult_epi returns PMH_EPI_UNSUPPORTED and MPGP
// runs its separate vector kernels; the ||B u|| rider of the penalised operator is declined too (the one-row projector's own dot runs).
#include <algorithm>

#include "svm_csr_seg.h"

// first[b] = the segment that holds entry b SVC_SPAN (the smallest c with ptr[c + 1] > b SVC_SPAN); first[0] = 0, so that leading empty segments belong to span 0
__global__ __launch_bounds__(PMH_BLOCK) void k_svc_first(int nb, int nseg, const int *__restrict__ ptr, int *__restrict__ first)
{
  const int b = blockIdx.x * PMH_BLOCK + threadIdx.x;
  if (b >= nb) return;
  const long long start = (long long)b * SVC_SPAN;
  int             lo = 0, hi = nseg - 1; // the answer lies in [lo, hi]: ptr[nseg] > start for every span of a non-empty array
  while (b > 0 && lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (ptr[mid + 1] > start) hi = mid;
    else lo = mid + 1;
  }
  first[b] = b > 0 ? lo : 0;
}

// what a finished segment sum becomes.  MODE 0: out[c] = sum; 1: out[c] = y_c sum; 2: out[c] = svm_aug_row(y_c, sum, sigma s, shift, a_c); 3: the same with diag_c
// where shift was (pmh_op_svm_dual_set_diag)
struct svc_out {
  double       *out;
  const double *y, *a, *s; // s: device scalar (w[d])
  double        sigma, shift;
  const double *diag = nullptr; // MODE 3
};
template <int MODE> static __device__ __forceinline__ void svc_store(const svc_out &o, int c, double v, double sS)
{
  if (MODE == 0) o.out[c] = v;
  else if (MODE == 1) o.out[c] = o.y[c] * v;
  else o.out[c] = svm_aug_row(o.y[c], v, sS, MODE == 3 ? o.diag[c] : o.shift, o.a[c]);
}

template <int MODE>
__global__ __launch_bounds__(PMH_BLOCK) void k_svc_seg(int nent, int nseg, int nb, const int *__restrict__ ptr, const int *__restrict__ idx, const double *__restrict__ val, const double *__restrict__ x,
                                                       const int *__restrict__ first, double *__restrict__ head, double *__restrict__ tail, svc_out o)
{
  __shared__ double prod[SVC_SPAN];
  const int         b = blockIdx.x, start = b * SVC_SPAN, end = min(start + SVC_SPAN, nent);
  // the span's products: every load of values and indices asked for before the gathers
  dbl2  v[SVC_SPAN / PMH_BLOCK / 2];
  int2v ix[SVC_SPAN / PMH_BLOCK / 2];
#pragma unroll
  for (int j = 0; j < SVC_SPAN / PMH_BLOCK / 2; j++) svc_load_pair(j, start, end, val, idx, v[j], ix[j]);
#pragma unroll
  for (int j = 0; j < SVC_SPAN / PMH_BLOCK / 2; j++) {
    const int k = 2 * (j * PMH_BLOCK + (int)threadIdx.x);
    prod[k]     = v[j].x * x[ix[j].x]; // (entries past the end: 0 * x[0], never read below)
    prod[k + 1] = v[j].y * x[ix[j].y];
  }
  __syncthreads();
  const double sS = MODE >= 2 ? o.sigma * *o.s : 0.0;
  svc_segments<1>(
    b, nb, nseg, start, end, ptr, first, head, tail, [&](int k, double(&s)[1]) { s[0] += prod[k]; }, [&](int c, const double(&s)[1]) { svc_store<MODE>(o, c, s[0], sS); });
}

// the shared segments, each completed in the span where it ends
template <int MODE>
__global__ __launch_bounds__(PMH_BLOCK) void k_svc_fin(int nent, int nseg, int nb, const int *__restrict__ ptr, const int *__restrict__ first, const double *__restrict__ head,
                                                       const double *__restrict__ tail, svc_out o)
{
  svc_finish<1>(nent, nseg, nb, ptr, first, head, tail, [&](int c, const double(&s)[1]) { svc_store<MODE>(o, c, s[0], MODE >= 2 ? o.sigma * *o.s : 0.0); });
}

// new labels: cval[q] = y_i(old) y_i(new) cval[q] for the entry q of sample i = crow[q] (column d included: y_i(old)^2 y_i(new) = y_i(new)); the products
// with +-1 are exact.  ysign is brought up to date by k_svc_copy afterwards (every entry of a sample needs the old sign)
__global__ __launch_bounds__(PMH_BLOCK) void k_svc_resign(long long nent, const int *__restrict__ crow, const double *__restrict__ ysign, const double *__restrict__ ynew, double *__restrict__ cval)
{
  for (long long q = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; q < nent; q += (long long)gridDim.x * PMH_BLOCK) {
    const int i = crow[q];
    cval[q]     = (ysign[i] * ynew[i]) * cval[q];
  }
}
__global__ __launch_bounds__(PMH_BLOCK) void k_svc_copy(int n, const double *__restrict__ src, double *__restrict__ dst)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) dst[i] = src[i];
}

// a sample subset: am_i = m_i != 0 ? a_i : +0, the operand both passes see (whatever a holds on a held-out sample, a NaN included, has no effect)
__global__ __launch_bounds__(PMH_BLOCK) void k_svc_mask_operand(int n, const double *__restrict__ a, const double *__restrict__ m, double *__restrict__ am)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) am[i] = m[i] != 0.0 ? a[i] : 0.0;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------
int svc_tab_free(pmh_ctx ctx, svc_tab *t)
{
  if (t->first) pmh_free(ctx, t->first), pmh_free(ctx, t->head), pmh_free(ctx, t->tail);
  t->first = nullptr, t->head = t->tail = nullptr;
  return PMH_SUCCESS;
}
int svc_tab_build(pmh_ctx ctx, int nseg, const int *ptr, long long nent, svc_tab *t, int ncol)
{
  t->nb = svc_nb(nent);
  PMH_CHK(pmh_malloc(ctx, sizeof(int) * (size_t)t->nb, (void **)&t->first));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)t->nb * ncol, (void **)&t->head));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)t->nb * ncol, (void **)&t->tail));
  hipLaunchKernelGGL(k_svc_first, dim3((t->nb + PMH_BLOCK - 1) / PMH_BLOCK), dim3(PMH_BLOCK), 0, ctx->stream, t->nb, nseg, ptr, t->first);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}
// out[c] = MODE(sum of segment c) for the first nseg segments / nent entries of the array the table was built for
template <int MODE> static int svc_sweep(pmh_ctx ctx, const svc_tab &t, int nseg, long long nent, const int *ptr, const int *idx, const double *val, const double *x, const svc_out &o)
{
  const int nb = std::min(t.nb, svc_nb(nent));
  hipLaunchKernelGGL(k_svc_seg<MODE>, dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, (int)nent, nseg, nb, ptr, idx, val, x, (const int *)t.first, t.head, t.tail, o);
  hipLaunchKernelGGL(k_svc_fin<MODE>, dim3((nb + PMH_BLOCK / 64 - 1) / (PMH_BLOCK / 64)), dim3(PMH_BLOCK), 0, ctx->stream, (int)nent, nseg, nb, ptr, (const int *)t.first, (const double *)t.head,
                     (const double *)t.tail, o);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

struct SvmCsrOp : SvmDualBase {
  pmh_csr   X = nullptr; // borrowed: the samples by rows
  long long nnz = 0;
  int      *cptr = nullptr, *crow = nullptr; // the column-ordered copy: [d + 2], [nnz + n]
  double   *cval = nullptr, *w = nullptr;    // [nnz + n] (y_i x_ic; column d: y_i), [d + 1]
  double   *ysign = nullptr;                 // [n] the labels cval was signed with (the operator's own copy)
  // A sample subset (SvmDualBase::msk, ym): the column-ordered copy and ysign stay those of all samples (new labels re-sign them bit for bit as before); pass 1
  // gathers am = a o m in place of a (one n-vector kernel before the sweep, 24 n bytes beside the sweep's 12 (nnz + n): no second gather per stored entry), so
  // held-out samples add nothing to w and s; pass 2 reads ym for y and am for a: (0 (x_i . w) + sigma s 0) + shift 0 = 0 on a held-out sample, shift or
  // diagonal.  Every stored entry is still swept: no row is skipped on this path
  double   *am = nullptr; // [n], allocated by the first product under a subset
  int       mask_operand(const double *a, const double **out)
  {
    *out = a;
    if (!ym || n <= 0) return PMH_SUCCESS;
    if (!am) PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)n, (void **)&am));
    hipLaunchKernelGGL(k_svc_mask_operand, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, a, (const double *)msk, am);
    PMH_HIP(hipGetLastError());
    *out = am;
    return PMH_SUCCESS;
  }
  svc_tab   rows, cols;
  ~SvmCsrOp() override
  {
    pmh_free(ctx, cptr), pmh_free(ctx, crow), pmh_free(ctx, cval), pmh_free(ctx, w);
    if (ysign) pmh_free(ctx, ysign);
    if (am) pmh_free(ctx, am);
    svc_tab_free(ctx, &rows), svc_tab_free(ctx, &cols);
  }
  // w[0 .. d) = X'(y o a); with_s: also w[d] = sum_i y_i a_i (the sweep goes on through column d)
  int pass1(const double *a, bool with_s)
  {
    npass++;
    svc_out o{w, nullptr, nullptr, nullptr, 0.0, 0.0};
    return svc_sweep<0>(ctx, cols, with_s ? d + 1 : d, with_s ? nnz + n : nnz, cptr, crow, cval, a, o);
  }
  int set_labels(const double *y_dev) override
  {
    if (n > 0) {
      const long long nent = nnz + n, nbl = (nent + PMH_BLOCK - 1) / PMH_BLOCK;
      hipLaunchKernelGGL(k_svc_resign, dim3((unsigned)std::min<long long>(nbl, 8 * PMH_MAX_VEC_BLOCKS)), dim3(PMH_BLOCK), 0, ctx->stream, nent, (const int *)crow, (const double *)ysign, y_dev, cval);
      hipLaunchKernelGGL(k_svc_copy, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, y_dev, ysign);
      PMH_HIP(hipGetLastError());
    }
    y = y_dev;
    return refresh_ym();
  }
  int mult(const double *a, double *Ha) override
  {
    if (n == 0 && pmh_comm_on(ctx)) return pmh_set_error(PMH_ERR_ARG, "SVM dual operator: this rank holds no samples; with a communicator every rank needs at least one row");
    if (n == 0) return PMH_SUCCESS;
    const bool AG = aug();
    PMH_CHK(mask_operand(a, &a));
    PMH_CHK(pass1(a, AG));
    PMH_CHK(pmh_comm_allreduce_sum(ctx, w, (size_t)d + (AG ? 1 : 0))); // samples sharded over GPUs: the one exchange step, as in the dense operator
    npass++;
    svc_out o{Ha, yk(), a, w + d, sigma + sigma_fold, shift, diag};
    if (diag) return svc_sweep<3>(ctx, rows, n, nnz, X->d_rowptr, X->d_col, X->d_val, w, o);
    if (AG) return svc_sweep<2>(ctx, rows, n, nnz, X->d_rowptr, X->d_col, X->d_val, w, o);
    return svc_sweep<1>(ctx, rows, n, nnz, X->d_rowptr, X->d_col, X->d_val, w, o);
  }
  int mult_epi(const double *, double *, const pmh_vec_epi &) override
  {
    if (n <= 0 && pmh_comm_on(ctx)) return pmh_set_error(PMH_ERR_ARG, "SVM dual operator: this rank holds no samples; with a communicator every rank needs at least one row (an empty shard would skip the collectives the other ranks issue)");
    return PMH_EPI_UNSUPPORTED;
  }
  int form_w(const double *a, const double **w_dev) override
  {
    PMH_CHK(mask_operand(a, &a));
    if (n > 0) PMH_CHK(pass1(a, false));
    else PMH_CHK(pmh_memset(ctx, w, 0, sizeof(double) * (size_t)d));
    PMH_CHK(pmh_comm_allreduce_sum(ctx, w, (size_t)d));
    *w_dev = w;
    return PMH_SUCCESS;
  }
};

int pmh_svm_csr_op_row_dots(SvmDualBase *op, const double *wv, double *dots)
{
  SvmCsrOp *o = dynamic_cast<SvmCsrOp *>(op);
  PMH_ARG(o && wv && dots);
  if (o->n == 0) return PMH_SUCCESS;
  o->npass++;
  svc_out so{dots, nullptr, nullptr, nullptr, 0.0, 0.0};
  return svc_sweep<0>(o->ctx, o->rows, o->n, o->nnz, o->X->d_rowptr, o->X->d_col, o->X->d_val, wv, so);
}

// the kernels' 32-bit offsets: an array of nent entries, and the span past its end, must stay below 2^31
static bool svc_too_many(long long nent) { return nent >= (1LL << 31) - SVC_SPAN; }
static int  svc_check_entries(long long nnz) { return svc_too_many(nnz) ? pmh_set_error(PMH_ERR_ARG, "SVM on CSR samples: %lld stored entries, the count must stay below 2^31 (32-bit offsets)", nnz) : PMH_SUCCESS; }

int pmh_svm_check_test_samples(const char *who, int d, pmh_csr Xt)
{
  if (Xt && Xt->ncols != d) return pmh_set_error(PMH_ERR_ARG, "%s_csr: the test samples have %d features, the model has %d", who, Xt->ncols, d);
  if (!Xt && d > 64 * SVM_KMAX) return pmh_set_error(PMH_ERR_ARG, "%s: dense test samples need d <= %d, the model has d = %d: hand them over in CSR (%s_csr)", who, 64 * SVM_KMAX, d, who);
  return Xt ? svc_check_entries(Xt->nnz) : PMH_SUCCESS;
}

int sv_check_mapped(const char *who, const sv_mapped &mp, int n, int d)
{
  if (!mp.map) return pmh_set_error(PMH_ERR_ARG, "%s_rff: the map is NULL", who);
  if (n < 0 || (n > 0 && !mp.X)) return pmh_set_error(PMH_ERR_ARG, "%s_rff: n = %d, X_dev %s", who, n, mp.X ? "given" : "NULL");
  int D = 0;
  PMH_CHK(pmh_rff_get(mp.map, nullptr, &D, nullptr, nullptr, nullptr));
  if (D != d) return pmh_set_error(PMH_ERR_ARG, "%s_rff: the map has D = %d features, the model has d = %d", who, D, d);
  return PMH_SUCCESS;
}

int pmh_svm_csr_row_dots(pmh_csr X, const double *wv, double *dots)
{
  PMH_ARG(X && wv && dots);
  if (X->nrows == 0) return PMH_SUCCESS;
  PMH_CHK(svc_check_entries(X->nnz));
  svc_tab t;
  int     rc = svc_tab_build(X->ctx, X->nrows, X->d_rowptr, X->nnz, &t);
  svc_out so{dots, nullptr, nullptr, nullptr, 0.0, 0.0};
  if (!rc) rc = svc_sweep<0>(X->ctx, t, X->nrows, X->nnz, X->d_rowptr, X->d_col, X->d_val, wv, so);
  svc_tab_free(X->ctx, &t); // (waits for the stream)
  return rc;
}

extern "C" int pmh_op_create_svm_dual_csr(pmh_ctx ctx, pmh_csr X, const double *y_dev, pmh_op *op)
{
  PMH_ARG(ctx && X && op && y_dev && X->ctx == ctx);
  const int       n = X->nrows, d = X->ncols;
  const long long nnz = X->nnz;
  if (d < 1) return pmh_set_error(PMH_ERR_ARG, "pmh_op_create_svm_dual_csr: the sample matrix has no columns");
  if (svc_too_many(nnz + n)) return pmh_set_error(PMH_ERR_ARG, "pmh_op_create_svm_dual_csr: %lld stored entries and %d samples: the entry count must stay below 2^31 (32-bit offsets)", nnz, n);
  // the caller's matrix on the host: checked (columns ascending inside a row; their range was checked by pmh_csr_create) and turned by columns
  std::vector<int>    rp((size_t)n + 1, 0), col((size_t)nnz);
  std::vector<double> val((size_t)nnz), yh((size_t)n);
  PMH_CHK(pmh_memcpy_d2h(ctx, rp.data(), X->d_rowptr, sizeof(int) * rp.size()));
  if (nnz) PMH_CHK(pmh_memcpy_d2h(ctx, col.data(), X->d_col, sizeof(int) * col.size()));
  if (nnz) PMH_CHK(pmh_memcpy_d2h(ctx, val.data(), X->d_val, sizeof(double) * val.size()));
  if (n) PMH_CHK(pmh_memcpy_d2h(ctx, yh.data(), y_dev, sizeof(double) * yh.size()));
  std::vector<int> cp((size_t)d + 2, 0);
  for (int i = 0; i < n; i++)
    for (int k = rp[i]; k < rp[i + 1]; k++) {
      if (col[k] < 0 || col[k] >= d) return pmh_set_error(PMH_ERR_ARG, "pmh_op_create_svm_dual_csr: column index %d of sample %d is outside [0, %d)", col[k], i, d);
      if (k > rp[i] && col[k] < col[k - 1]) return pmh_set_error(PMH_ERR_ARG, "pmh_op_create_svm_dual_csr: the column indices of sample %d are not sorted (%d after %d)", i, col[k], col[k - 1]);
      cp[(size_t)col[k] + 1]++;
    }
  for (int c = 0; c < d; c++) cp[(size_t)c + 1] += cp[c];
  cp[(size_t)d + 1] = (int)(nnz + n);
  std::vector<int>    cr((size_t)(nnz + n)), next(cp.begin(), cp.begin() + d);
  std::vector<double> cv((size_t)(nnz + n));
  for (int i = 0; i < n; i++) { // samples in ascending order: rows ascending inside every column
    for (int k = rp[i]; k < rp[i + 1]; k++) {
      const int q = next[col[k]]++;
      cr[q] = i, cv[q] = yh[i] * val[k];
    }
    cr[(size_t)nnz + i] = i, cv[(size_t)nnz + i] = yh[i];
  }
  SvmCsrOp *o = new SvmCsrOp();
  o->ctx = ctx, o->n = n, o->d = d, o->y = y_dev, o->X = X, o->nnz = nnz;
  int rc = PMH_SUCCESS;
  do {
    if ((rc = pmh_malloc(ctx, sizeof(int) * cp.size(), (void **)&o->cptr)) || (rc = pmh_malloc(ctx, sizeof(int) * (cr.size() + 2), (void **)&o->crow)) ||
        (rc = pmh_malloc(ctx, sizeof(double) * (cv.size() + 2), (void **)&o->cval)) || (rc = pmh_malloc(ctx, sizeof(double) * ((size_t)d + 1), (void **)&o->w)) ||
        (rc = pmh_malloc(ctx, sizeof(double) * (size_t)(n ? n : 1), (void **)&o->ysign)))
      break;
    if (n > 0 && (rc = pmh_memcpy_h2d(ctx, o->ysign, yh.data(), sizeof(double) * yh.size()))) break;
    if ((rc = pmh_memcpy_h2d(ctx, o->cptr, cp.data(), sizeof(int) * cp.size()))) break;
    if (!cr.empty() && ((rc = pmh_memcpy_h2d(ctx, o->crow, cr.data(), sizeof(int) * cr.size())) || (rc = pmh_memcpy_h2d(ctx, o->cval, cv.data(), sizeof(double) * cv.size())))) break;
    if ((rc = pmh_memset(ctx, o->w, 0, sizeof(double) * ((size_t)d + 1)))) break;
    if (n > 0 && ((rc = svc_tab_build(ctx, n, X->d_rowptr, nnz, &o->rows)) || (rc = svc_tab_build(ctx, d + 1, o->cptr, nnz + n, &o->cols)))) break;
  } while (0);
  if (rc) {
    delete o;
    return rc;
  }
  *op = o;
  return PMH_SUCCESS;
}
