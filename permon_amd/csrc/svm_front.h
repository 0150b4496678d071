// What the SVM front end (svm_train.hip), the SVR front end (svr_train.hip) and the Platt fit (svm_proba.hip) share, each written once:
//   svm_store<K, MINROW>    K sums of a thread -> part[K][grid]; pmh_svm_sum_rows / pmh_svm_finish_part: one workgroup finishes them in a fixed order
//   sv_front                the training core both handles derive from: samples, operator, projector, solver, the vectors of the QP, the model
//   sv_build_solver, sv_solve, sv_model_tail, sv_count_bad, sv_alloc_common, sv_free   the steps of create / train / model that do not depend on what is trained
//   sv_count_subset, sv_refresh_row, sv_get_subset, svm_sel, sv_own_selector   what a sample subset needs on either side: n_S, the equality's row over the
//                           operator's masked labels, the mask handed back, the selector of test_own
// What is particular to a side stays in its file: labels, the subset's right-hand side and diagonal, warm starts and calibration (svm_train.hip); epsilon, the
// doubled right-hand side and the metrics (svr_train.hip).  Definitions: svm_front.hip.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#include "svm_rows.h"
#include "svr_internal.h"

// ---- the sums ---------------------------------------------------------------------------------------------------------------------------------------------------
// K sums of a thread reduced over the workgroup one after the other -> part[K][gridDim.x]; MINROW: that row is a minimum (a maximum travels negated)
template <int K, int MINROW = -1> static __device__ __forceinline__ void svm_store(const double (&s)[K], double *red, double *__restrict__ part)
{
#pragma unroll
  for (int k = 0; k < K; k++) {
    const double r = k == MINROW ? pmh_block_reduce<PMH_RED_MIN>(s[k], red) : pmh_block_reduce<PMH_RED_SUM>(s[k], red);
    if (threadIdx.x == 0) part[(size_t)k * gridDim.x + blockIdx.x] = r;
  }
}
// out[k] = sum (k == minrow: min) over b of part[k][b], k < K (k_svm_finish: one workgroup, fixed order; the counts are sums of ones: exact below 2^53),
// enqueue only
int pmh_svm_sum_rows(pmh_ctx ctx, int nb, int K, const double *part, double *out, int minrow = -1);
// scal[0 .. K) = the K rows a kernel left in part[K][nb], finished and joined over the ranks (n == 0: no kernel ran: zeros).  All sums: one
// pmh_comm_allreduce_sum; with a minimum row: pmh_comm_allreduce_scalars with the row's operation
int pmh_svm_finish_part(pmh_ctx ctx, int n, int nb, int K, int minrow, const double *part, double *scal);

// ---- the training core ----------------------------------------------------------------------------------------------------------------------------------------
struct sv_front {
  pmh_ctx       ctx = nullptr;
  int           n = 0, nu = 0, d = 0; // samples of this rank, length of the dual (n, or 2 n for the regression), features
  long long     n_global = 0;
  const void   *X = nullptr; // dense rows: doubles, or floats where f32
  int           f32 = 0;
  pmh_csr       Xcsr = nullptr; // the samples in CSR (then X == nullptr), borrowed
  pmh_op        H    = nullptr;
  pmh_qppf      pf   = nullptr;
  pmh_mpgp      mpgp = nullptr;
  pmh_smalxe    sx   = nullptr;
  double       *u = nullptr, *rhs = nullptr, *lb = nullptr, *ub = nullptr, *row = nullptr; // nu each (ub: L1 only; row: bias only)
  double       *w = nullptr, *part = nullptr, *scal = nullptr;
  double       *dots = nullptr;                // CSR: x_i . w of the training samples (n doubles, allocated by the first model)
  double       *Cv = nullptr, *Cinv = nullptr; // set_penalties: C_i and, L2, 1 / C_i (n doubles); nullptr: C everywhere
  std::vector<double> h_w;
  double        b = 0.0;
  int           trained = 0;
  pmh_qps_opts    o_qps;
  pmh_mpgp_opts   o_mpgp;
  pmh_smalxe_opts o_smalxe;
  int             bias = 0, loss_type = 0;
  double          astol() const { return sx ? o_smalxe.inner.astol : o_mpgp.astol; } // of the solver that trains
  // a sample subset (pmh_svm_set_subset, pmh_svr_set_subset): the mask and the masked labels are the operator's (SvmDualBase::msk, ym); n_sub: the subset's
  // samples over all ranks (0: no subset)
  long long       n_sub = 0;
};

// ---- sample subsets ---------------------------------------------------------------------------------------------------------------------------------------------
// the samples the problem is posed over, all ranks: the subset's, or all
static inline long long sv_n_posed(const sv_front *f) { return f->n_sub > 0 ? f->n_sub : f->n_global; }
// n_sub from the operator's mask, all-reduced as n_global is (0 where the operator holds none)
int sv_count_subset(sv_front *f);
// the equality's row c (labels) over the nu entries of the dual and its one-row projector, built anew: the operator's labels as its kernels read them (yk():
// the masked ones under a subset, zero on the held-out entries).  Classification: c = 1 / sqrt(n_S); regression: the labels are [m; -m], c = 1 / sqrt(2 n_S)
int sv_refresh_row(sv_front *f, double c);
// row = c y (n doubles each, device)
int sv_fill_row(pmh_ctx ctx, int n, const double *y, double c, double *row);
// the mask (n doubles, device; all 1 without a subset; may be NULL) and n_S over all ranks (n without a subset; may be NULL)
int sv_get_subset(sv_front *f, double *m_dev, long long *n_in);
// The selector of pmh_svm_test_own / pmh_svr_test_own: with m given, a sample is counted only where m_i == want (the handle's subset mask: 1 the subset, 0 the
// held-out rows)
struct svm_sel {
  const double *m = nullptr;
  double        want = 0.0;
};
// the selector of `which` (PMH_SVM_OWN_*, checked here in the name of who: PMH_ERR_ARG; HELD_OUT without a subset: PMH_ERR_STATE) over the handle's own samples
int sv_own_selector(sv_front *f, const char *who, const char *set_subset, int which, svm_sel *sel);

// the solvers hold the operator and the projector: whoever changes or replaces either drops them first
void sv_drop_solver(sv_front *f);
// The solver over the core's operator, vectors and projector: SMALXE (bias) or MPGP.  Both size their steps and penalties by the operator's largest
// eigenvalue, estimated at creation: whoever changes the operator's terms builds the solver anew
int sv_build_solver(sv_front *f);
// One solve from the current u: SMALXE is reset first; then reason .. rnorm and passes_X of ST (pmh_svm_stats or pmh_svr_stats) from whichever solver ran.
// What differs between the callers comes before: the regression resets MPGP's counters, a warm classification sets SMALXE's multiplier
template <class ST> int sv_solve(sv_front *f, ST *st);
// After the bias pass left its four sums in scal[0..3]: the equality's multiplier through pmh_onerow_dot -> scal[4], the five doubles and w to the host,
// n_free_sv, n_sv, b_free, b_multiplier = multiplier / row_scale and b of ST.  row_scale: the equality's row is (labels) / row_scale.  h[0..5) are the five
// doubles: h[1] is the caller's (y'alpha, sum beta)
template <class ST> int sv_model_tail(sv_front *f, double row_scale, ST *st, double (&h)[5]);
// device memory of a create: u, rhs, lb (nu each; u and lb zeroed), w, part (part_rows rows: the most sums a kernel of the handle leaves), scal; L1: ub = C
int sv_alloc_common(sv_front *f, int part_rows, double C);
// n_global = the samples over all ranks; with a bias at least one is needed (PMH_ERR_ARG in the name of who)
int sv_count_samples(sv_front *f, const char *who);
// set_penalties: Cv and, L2, Cinv (n doubles each), allocated once
int sv_alloc_penalties(sv_front *f);
// the options both pmh_svm_opts and pmh_svr_opts carry
template <class O> static void sv_take_opts(sv_front *f, const O &o) { f->loss_type = o.loss_type, f->bias = o.bias, f->o_qps = o.qps, f->o_mpgp = o.mpgp, f->o_smalxe = o.smalxe; }
// the solver, the projector, the operator and every buffer of the core
void sv_free(sv_front *f);
// pre: "pmh_svm" / "pmh_svr", for the message of an untrained handle
int sv_get_model(sv_front *f, const char *pre, double *w_host, double *b);
int sv_get_solver(sv_front *f, pmh_op *H, pmh_qppf *pf, pmh_mpgp *mpgp, pmh_smalxe *smalxe);

// the count an int-counting kernel leaves (launch: what runs it on d_bad), summed over the ranks so that every rank decides alike; what: the values checked
template <class L> static int sv_count_bad(pmh_ctx ctx, const char *who, const char *what, L launch, long long *nbad)
{
  int  bad   = 0;
  int *d_bad = nullptr;
  PMH_CHK(pmh_malloc(ctx, sizeof(int), (void **)&d_bad));
  int rc = pmh_memset(ctx, d_bad, 0, sizeof(int));
  if (!rc) {
    launch(d_bad);
    if (hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "%s: the launch that checks the %s failed", who, what);
  }
  if (!rc) rc = pmh_memcpy_d2h(ctx, &bad, d_bad, sizeof(int));
  pmh_free(ctx, d_bad);
  PMH_CHK(rc);
  double c = (double)bad;
  PMH_CHK(pmh_comm_sum_host(ctx, &c, 1));
  *nbad = (long long)c;
  return PMH_SUCCESS;
}

// ---- the row kernels ------------------------------------------------------------------------------------------------------------------------------------------
// What a kernel does with row i's dot product x_i . w is a functor F, passed by value: it carries its arguments and its per-thread sums; f.row(i, dot) takes the
// row, f.done(red) leaves the sums (svm_store) or nothing.  Three shells: any d, d == 64, and one thread per ready dot product (samples in CSR).
// T: the type the samples are stored in, double or float (widened in the sweep, svm_rows.h)
template <class T, class F> __global__ __launch_bounds__(PMH_BLOCK) void k_svm_rows(int n, int d, const T *__restrict__ X, const double *__restrict__ w, F f)
{
  __shared__ double red[PMH_BLOCK / 64];
  svm_sweep_rows(n, d, X, w, [&](long long i, double dot) { f.row(i, dot); });
  f.done(red);
}
// d == 64: the row layout of k_svm_x64 (svm.hip), four row groups in flight
template <class T, class F> __global__ __launch_bounds__(PMH_BLOCK) void k_svm_rows64(int n, const T *__restrict__ X, const double *__restrict__ w, F f)
{
  __shared__ double red[PMH_BLOCK / 64];
  svm_sweep_rows64<4>(n, X, w, [&](long long i, double dot) { f.row(i, dot); });
  f.done(red);
}
// (no __restrict__ on dots: the scores and the probabilities are written over the dot products)
template <class F> __global__ __launch_bounds__(PMH_BLOCK) void k_svm_dots(int n, const double *dots, F f)
{
  __shared__ double red[PMH_BLOCK / 64];
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) f.row(i, dots[i]);
  f.done(red);
}

// One pass of f over n samples against w, SVM_NB(n) workgroups: dense rows X (doubles, or floats where f32: the generic sweep or, LAY64 and d == 64, the
// 64-column layout, whose dot products sum in another order: the scoring passes take it, the bias pass never did) or ready dot products: of the CSR samples Xt,
// of the rows of the operator own, or of the mapped samples mp, which go through dots first (nullptr: a buffer of this call).  who names the entry in the messages
template <bool LAY64, class F>
static int sv_sweep(pmh_ctx ctx, const char *who, int n, int d, const void *X, int f32, pmh_csr Xt, SvmDualBase *own, const double *w, double *dots, F f, const sv_mapped *mp = nullptr)
{
  if (n <= 0) return PMH_SUCCESS;
  const int nb = SVM_NB(n);
  if (Xt || own || mp) {
    double *buf = dots;
    if (!buf) PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)n, (void **)&buf));
    int rc = mp   ? pmh_rffdots(mp->map, n, mp->X, mp->x_type, 1, w, d, buf)
             : Xt ? pmh_svm_csr_row_dots(Xt, w, buf)
                  : own->doubled() ? static_cast<SvrDualBase *>(own)->row_dots(w, buf) : pmh_svm_csr_op_row_dots(own, w, buf);
    if (!rc) {
      hipLaunchKernelGGL(k_svm_dots<F>, dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, n, (const double *)buf, f);
      if (hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "%s%s: the launch failed", who, mp ? "_rff" : "_csr");
    }
    if (!dots) pmh_free(ctx, buf); // (waits for the stream)
    return rc;
  }
  svm_const<2>(f32, [&](auto V) {
    using T = svm_sample_t<decltype(V)>;
    if constexpr (LAY64) {
      if (d == 64) {
        hipLaunchKernelGGL((k_svm_rows64<T, F>), dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, n, (const T *)X, w, f);
        return;
      }
    }
    hipLaunchKernelGGL((k_svm_rows<T, F>), dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, n, d, (const T *)X, w, f);
  });
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

// w, b and the counts from the current u: w by the operator's pass 1, the four sums of the bias functor (the generic sweep at every d; CSR: the operator's own
// row sweep into f->dots) by one pass over X, then sv_model_tail
template <class F, class ST> static int sv_model(sv_front *f, const char *who, F bias, double row_scale, ST *st, double (&h)[5])
{
  SvmDualBase  *H = static_cast<SvmDualBase *>(f->H);
  const double *w = nullptr;
  PMH_CHK(H->form_w(f->u, &w));
  PMH_CHK(pmh_vec_copy(f->ctx, f->d, w, f->w));
  if (f->n > 0 && f->Xcsr && !f->dots) PMH_CHK(pmh_malloc(f->ctx, sizeof(double) * (size_t)f->n, (void **)&f->dots));
  if (f->n > 0 && !f->Xcsr) H->npass++;
  PMH_CHK(sv_sweep<false>(f->ctx, who, f->n, f->d, f->X, f->f32, nullptr, f->Xcsr ? H : nullptr, f->w, f->dots, bias));
  PMH_CHK(pmh_svm_finish_part(f->ctx, f->n, SVM_NB(f->n), 4, -1, f->part, f->scal));
  return sv_model_tail(f, row_scale, st, h);
}
