// SVM front end (PermonSVM's role: train, model, predict) over the dual operators of svm.hip (dense rows) and svm_csr.hip (samples in CSR):
//   L1: min 1/2 a'Ha - 1'a,          0 <= a <= C   (primal 1/2 |w|^2 + C sum xi)
//   L2: min 1/2 a'(H + I/C)a - 1'a,  0 <= a        (primal 1/2 |w|^2 + C/2 sum xi^2)
//   penalties (pmh_svm_set_penalties): C_i = (y_i > 0 ? C_pos : C_neg) weight_i per sample: L1 the upper bounds, L2 the diagonal 1 / C_i of the operator
//   bias: additionally y'a = 0, posed as (y / sqrt(n))'a = 0 -- a one-row projector (onerow.hip) under SMALXE, whose penalty term the operator absorbs (qppf.hip)
// H = diag(y) X X' diag(y).  No bias: MPGP on the box alone.  Model: w = X'(y o a) by the operator's pass-1 kernels; b by one pass over X (k_svm_bias);
// prediction by one pass over the test samples (k_svm_predict: svm_sweep_rows, any d the operator accepts; k_svm_predict64 for d = 64: svm_sweep_rows64, the
// sweeps of the operator's own pass 2, svm_rows.h).  Samples in CSR: x_i . w by the entry-balanced sweep of svm_csr.hip (one pass over the stored entries), then
// one kernel over the n dot products (k_svm_bias_dots, k_svm_predict_dots).  What a row's dot product is used for is written once whichever kernel found it:
// svm_bias_row, svm_classify_row; their four sums per thread leave every kernel through svm_store4.
// Probabilities (pmh_svm_calibrate, pmh_svm_predict_proba): A, B of the Platt fit (svm_proba.hip) on the handle; 1 / (1 + exp(A (x_i . w + b) + B)) is one more
// functor on the same sweeps (k_svm_proba, k_svm_proba64, k_svm_proba_dots), so a probability costs the one pass over X that a score costs.
// Dense samples in float32 (pmh_svm_create_f32; test samples: pmh_svm_predict_f32, _test_f32, _predict_proba_f32, _calibrate_f32): the same kernels with the
// sample type as template argument, picked where they are launched; alpha, w, b, the solvers and the model are fp64 either way.
#include <cmath>

#include "svm_internal.h"
#include "svm_rows.h"

struct pmh_svm_s {
  pmh_ctx       ctx;
  int           n, d;
  long long     n_global;
  const void   *X; // dense rows: doubles, or floats where f32 (pmh_svm_create_f32)
  int           f32 = 0;
  const double *y;
  pmh_csr       Xcsr = nullptr; // the samples in CSR (then X == nullptr), borrowed
  double       *dots = nullptr; // CSR: x_i . w of the training samples (n doubles, allocated by the first model)
  pmh_svm_opts  o;
  pmh_op        H     = nullptr;
  pmh_qppf      pf    = nullptr;
  pmh_mpgp      mpgp  = nullptr;
  pmh_smalxe    sx    = nullptr;
  double       *alpha = nullptr, *rhs = nullptr, *lb = nullptr, *ub = nullptr, *row = nullptr, *w = nullptr, *part = nullptr, *scal = nullptr;
  double       *Cv = nullptr, *Cinv = nullptr; // pmh_svm_set_penalties: C_i (n doubles) and, L2, 1 / C_i (the operator's diagonal); nullptr: opts.C everywhere
  // pmh_svm_set_subset: the mask and the masked labels are the operator's (SvmDualBase::msk, ym); n_sub: the subset's samples over all ranks (0: no subset);
  // Dm: L2, the operator's diagonal m_i / C_i under a subset (n doubles)
  long long     n_sub = 0;
  double       *Dm = nullptr;
  std::vector<double> h_w;
  double        b = 0.0;
  int           trained = 0;
  pmh_svm_stats st;
  // warm starts (pmh_svm_train_warm): has_dual: alpha is the dual of a training with the current labels (pmh_svm_set_labels clears it; set_penalties and
  // set_subset keep alpha and the flag); b_mult: that training's bias from the equality's multiplier; ws_cnt / ws_masked, ws_clipped: the two counts of the
  // last start vector, on the device and (over all ranks) on the host
  int           has_dual = 0;
  double        b_mult   = 0.0;
  int          *ws_cnt   = nullptr;
  long long     ws_masked = 0, ws_clipped = 0;
  // the probability model of the current (w, b): whatever gives the handle another model clears it
  int                 calibrated = 0;
  double              cal_A = 0.0, cal_B = 0.0;
  pmh_svm_platt_stats cal_st;
};

__global__ __launch_bounds__(PMH_BLOCK) void k_svm_fill_row(int n, const double *__restrict__ y, double c, double *__restrict__ row)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) row[i] = c * y[i];
}

// the four sums a thread holds, reduced over the workgroup one after the other -> part[4][gridDim.x]
static __device__ __forceinline__ void svm_store4(double s0, double s1, double s2, double s3, double *red, double *__restrict__ part)
{
  const double r0 = pmh_block_reduce<PMH_RED_SUM>(s0, red), r1 = pmh_block_reduce<PMH_RED_SUM>(s1, red), r2 = pmh_block_reduce<PMH_RED_SUM>(s2, red), r3 = pmh_block_reduce<PMH_RED_SUM>(s3, red);
  if (threadIdx.x == 0) {
    const size_t g = gridDim.x;
    part[blockIdx.x] = r0, part[g + blockIdx.x] = r1, part[2 * g + blockIdx.x] = r2, part[3 * g + blockIdx.x] = r3;
  }
}

// sample i with dot = x_i . w in the sums of the bias: sb over the free support vectors of y_i - x_i . w, sya = y'a, nf the number of free support vectors, ns of
// support vectors; free: astol < a_i and (ubound > 0: a_i < ubound - astol)
static __device__ __forceinline__ void svm_bias_row(long long i, double dot, const double *__restrict__ y, const double *__restrict__ alpha, double astol, double ubound, double &sb, double &sya,
                                                    double &nf, double &ns)
{
  const double ai = alpha[i], yi = y[i];
  sya += yi * ai;
  if (ai > astol) {
    ns += 1.0;
    if (!(ubound > 0.0) || ai < ubound - astol) nf += 1.0, sb += yi - dot;
  }
}
// One pass over X for the bias: per workgroup the partial sums of svm_bias_row -> part[4][gridDim.x].  UBV: the upper bound of sample i is ubv[i] (per-sample
// penalties, L1), not the scalar
// T (this kernel and the predict / proba kernels below): the type the samples are stored in, double or float (widened in the sweep, svm_rows.h)
template <int UBV, class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_bias(int n, int d, const T *__restrict__ X, const double *__restrict__ y, const double *__restrict__ w, const double *__restrict__ alpha, double astol,
                                                        double ubound, const double *__restrict__ ubv, double *__restrict__ part)
{
  __shared__ double red[PMH_BLOCK / 64];
  double            sb = 0.0, sya = 0.0, nf = 0.0, ns = 0.0;
  svm_sweep_rows(n, d, X, w, [&](long long i, double dot) { svm_bias_row(i, dot, y, alpha, astol, UBV ? ubv[i] : ubound, sb, sya, nf, ns); });
  svm_store4(sb, sya, nf, ns, red, part);
}
// out[k] = sum_b part[k][b], k < K: one workgroup, fixed order (the counts are sums of ones: exact below 2^53)
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_sum_rows(int nb, int K, const double *__restrict__ part, double *__restrict__ out)
{
  __shared__ double red[PMH_BLOCK / 64];
  for (int k = 0; k < K; k++) {
    double v = 0.0;
    for (int b = threadIdx.x; b < nb; b += PMH_BLOCK) v += part[(size_t)k * nb + b];
    v = pmh_block_reduce<PMH_RED_SUM>(v, red);
    if (threadIdx.x == 0) out[k] = v;
  }
}

struct svm_counts {
  double tp = 0.0, fp = 0.0, tn = 0.0, fn = 0.0;
};
// sample i with the score s = x_i . w + b: label_i = +-1 (s >= 0: +1) and, with the true labels, the confusion counts.  scores / labels / ytrue may each be
// nullptr; no __restrict__ on scores: the CSR form reads the dot products from the array the scores go to.  The counts go in and out by value: through
// references the choice (pos ? tp : fp) is one between addresses, and the compiler then keeps the counts in memory (40 bytes of scratch per lane, or 8 KiB of LDS)
// The selector of pmh_svm_test_own: with sel.m given, a sample is counted only where m_i == sel.want (the handle's subset mask: 1 the subset, 0 the held-out rows)
struct svm_sel {
  const double *m = nullptr;
  double        want = 0.0;
};
static __device__ __forceinline__ svm_counts svm_classify_row(long long i, double s, double *scores, double *__restrict__ labels, const double *__restrict__ ytrue, svm_counts c, svm_sel sel)
{
  const double l = s >= 0.0 ? 1.0 : -1.0;
  if (scores) scores[i] = s;
  if (labels) labels[i] = l;
  if (ytrue && (!sel.m || sel.m[i] == sel.want)) {
    const bool pos = ytrue[i] > 0.0;
    if (l > 0.0) (pos ? c.tp : c.fp) += 1.0;
    else (pos ? c.fn : c.tn) += 1.0;
  }
  return c;
}
// One pass over the test samples: scores, labels and per workgroup the confusion counts -> part[4][gridDim.x] (svm_classify_row)
template <class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_predict(int n, int d, const T *__restrict__ X, const double *__restrict__ w, double b, double *__restrict__ scores, double *__restrict__ labels,
                                                           const double *__restrict__ ytrue, double *__restrict__ part, svm_sel sel)
{
  __shared__ double red[PMH_BLOCK / 64];
  svm_counts        c;
  svm_sweep_rows(n, d, X, w, [&](long long i, double dot) { c = svm_classify_row(i, dot + b, scores, labels, ytrue, c, sel); });
  if (ytrue) svm_store4(c.tp, c.fp, c.tn, c.fn, red, part); // (uniform: a kernel argument)
}
// d == 64: the row layout of k_svm_x64 (svm.hip), four row groups in flight
template <class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_predict64(int n, const T *__restrict__ X, const double *__restrict__ w, double b, double *__restrict__ scores, double *__restrict__ labels,
                                                             const double *__restrict__ ytrue, double *__restrict__ part, svm_sel sel)
{
  __shared__ double red[PMH_BLOCK / 64];
  svm_counts        c;
  svm_sweep_rows64<4>(n, X, w, [&](long long i, double dot) { c = svm_classify_row(i, dot + b, scores, labels, ytrue, c, sel); });
  if (ytrue) svm_store4(c.tp, c.fp, c.tn, c.fn, red, part); // (uniform: a kernel argument)
}

// One pass over the test samples: proba[i] = 1 / (1 + exp(A (x_i . w + b) + B)), the dot product summed as k_svm_predict / k_svm_predict64 sum it
template <class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_proba(int n, int d, const T *__restrict__ X, const double *__restrict__ w, double b, double A, double B, double *__restrict__ proba)
{
  svm_sweep_rows(n, d, X, w, [&](long long i, double dot) { proba[i] = svm_sigmoid(A * (dot + b) + B); });
}
template <class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_proba64(int n, const T *__restrict__ X, const double *__restrict__ w, double b, double A, double B, double *__restrict__ proba)
{
  svm_sweep_rows64<4>(n, X, w, [&](long long i, double dot) { proba[i] = svm_sigmoid(A * (dot + b) + B); });
}

// ---- samples in CSR: the same sums as k_svm_bias / k_svm_predict from the rows' dot products x_i . w (svm_csr.hip), one entry per thread ----
template <int UBV>
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_bias_dots(int n, const double *__restrict__ dots, const double *__restrict__ y, const double *__restrict__ alpha, double astol, double ubound,
                                                             const double *__restrict__ ubv, double *__restrict__ part)
{
  __shared__ double red[PMH_BLOCK / 64];
  double            sb = 0.0, sya = 0.0, nf = 0.0, ns = 0.0;
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) svm_bias_row(i, dots[i], y, alpha, astol, UBV ? ubv[i] : ubound, sb, sya, nf, ns);
  svm_store4(sb, sya, nf, ns, red, part);
}
// (dots and scores may be the same array)
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_predict_dots(int n, const double *dots, double b, double *scores, double *__restrict__ labels, const double *__restrict__ ytrue, double *__restrict__ part, svm_sel sel)
{
  __shared__ double red[PMH_BLOCK / 64];
  svm_counts        c;
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) c = svm_classify_row(i, dots[i] + b, scores, labels, ytrue, c, sel);
  if (ytrue) svm_store4(c.tp, c.fp, c.tn, c.fn, red, part); // (uniform: a kernel argument)
}

// (in place: the dot products lie where the probabilities go)
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_proba_dots(int n, double b, double A, double B, double *proba)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) proba[i] = svm_sigmoid(A * (proba[i] + b) + B);
}

int pmh_svm_sum_rows(pmh_ctx ctx, int nb, int K, const double *part, double *out)
{
  hipLaunchKernelGGL(k_svm_sum_rows, dim3(1), dim3(PMH_BLOCK), 0, ctx->stream, nb, K, part, out);
  PMH_HIP(hipGetLastError()); // (also the launch of the kernel that filled part)
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_default_opts(pmh_svm_opts *o)
{
  PMH_ARG(o);
  memset(o, 0, sizeof(*o));
  o->loss_type = PMH_SVM_LOSS_L1;
  o->C         = 1.0;
  o->bias      = 1;
  PMH_CHK(pmh_qps_default_opts(&o->qps));
  PMH_CHK(pmh_mpgp_default_opts(&o->mpgp));
  return pmh_smalxe_default_opts(&o->smalxe);
}

extern "C" int pmh_svm_destroy(pmh_svm s)
{
  if (!s) return PMH_SUCCESS;
  if (s->mpgp) pmh_mpgp_destroy(s->mpgp);
  if (s->sx) pmh_smalxe_destroy(s->sx);
  if (s->pf) pmh_qppf_destroy(s->pf);
  if (s->H) pmh_op_destroy(s->H);
  double *v[] = {s->alpha, s->rhs, s->lb, s->ub, s->row, s->w, s->part, s->scal, s->dots, s->Cv, s->Cinv, s->Dm};
  for (double *p : v)
    if (p) pmh_free(s->ctx, p);
  if (s->ws_cnt) pmh_free(s->ctx, s->ws_cnt);
  delete s;
  return PMH_SUCCESS;
}

// the solvers hold the operator and the projector: whoever changes or replaces either drops them first
static void svm_drop_solver(pmh_svm s)
{
  if (s->mpgp) pmh_mpgp_destroy(s->mpgp), s->mpgp = nullptr;
  if (s->sx) pmh_smalxe_destroy(s->sx), s->sx = nullptr;
}
// The solver over the handle's operator, vectors and projector: SMALXE (bias) or MPGP.  Both size their steps and penalties by the operator's largest
// eigenvalue, estimated at creation: whoever changes the operator's terms (pmh_svm_set_penalties, L2) builds the solver anew
static int svm_build_solver(pmh_svm s)
{
  svm_drop_solver(s);
  if (s->o.bias) {
    pmh_smalxe_opts so = s->o.smalxe;
    so.rtol = s->o.qps.rtol, so.atol = s->o.qps.atol, so.divtol = s->o.qps.divtol;
    if (s->o.qps.max_it_set) so.max_it = s->o.qps.max_it;
    return pmh_smalxe_create(s->ctx, s->H, s->rhs, s->alpha, s->lb, s->ub, s->pf, &so, &s->sx);
  }
  pmh_mpgp_opts mo = s->o.mpgp;
  mo.rtol = s->o.qps.rtol, mo.atol = s->o.qps.atol, mo.divtol = s->o.qps.divtol, mo.max_it = s->o.qps.max_it;
  return pmh_mpgp_create(s->ctx, s->H, s->rhs, s->alpha, s->lb, s->ub, &mo, &s->mpgp);
}

// the samples the problem is posed over, all ranks: the subset's, or all
static long long svm_n_posed(pmh_svm s) { return s->n_sub > 0 ? s->n_sub : s->n_global; }
// the equality's row y / sqrt(n) and its projector; under a subset the masked labels over sqrt(n_S): zero on the held-out rows
static int svm_refresh_row(pmh_svm s)
{
  if (!s->o.bias) return PMH_SUCCESS;
  if (s->pf) pmh_qppf_destroy(s->pf), s->pf = nullptr;
  if (s->n > 0) hipLaunchKernelGGL(k_svm_fill_row, dim3(pmh_vec_grid(s->n)), dim3(PMH_BLOCK), 0, s->ctx->stream, s->n, static_cast<SvmDualBase *>(s->H)->yk(), 1.0 / sqrt((double)svm_n_posed(s)), s->row);
  PMH_HIP(hipGetLastError());
  return pmh_qppf_create_onerow(s->ctx, s->row, s->n, &s->pf);
}
// Dm_i = m_i cinv_i (cinv == nullptr: m_i c)
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_mask_diag(int n, const double *__restrict__ m, const double *__restrict__ cinv, double c, double *__restrict__ Dm)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) Dm[i] = m[i] != 0.0 ? (cinv ? cinv[i] : c) : 0.0;
}
// L2: the operator's term beside H from the handle's state: the shift 1 / C, the diagonal 1 / C_i (penalties) or, under a subset, the diagonal m_i / C_i
static int svm_refresh_l2(pmh_svm s)
{
  if (s->o.loss_type != PMH_SVM_LOSS_L2) return PMH_SUCCESS;
  if (s->n_sub > 0) {
    if (!s->Dm) PMH_CHK(pmh_malloc(s->ctx, sizeof(double) * (size_t)(s->n ? s->n : 1), (void **)&s->Dm));
    if (s->n > 0) hipLaunchKernelGGL(k_svm_mask_diag, dim3(pmh_vec_grid(s->n)), dim3(PMH_BLOCK), 0, s->ctx->stream, s->n, (const double *)static_cast<SvmDualBase *>(s->H)->msk, (const double *)s->Cinv, 1.0 / s->o.C, s->Dm);
    PMH_HIP(hipGetLastError());
    PMH_CHK(pmh_op_svm_dual_set_terms(s->H, 0.0, 0.0));
    return pmh_op_svm_dual_set_diag(s->H, s->Dm);
  }
  if (s->Cinv) {
    PMH_CHK(pmh_op_svm_dual_set_terms(s->H, 0.0, 0.0));
    return pmh_op_svm_dual_set_diag(s->H, s->Cinv);
  }
  PMH_CHK(pmh_op_svm_dual_set_diag(s->H, nullptr));
  return pmh_op_svm_dual_set_terms(s->H, 1.0 / s->o.C, 0.0);
}

// X_dev (dense rows: doubles, or floats where f32) or Xcsr
static int svm_create(pmh_ctx ctx, int n_local, int d, const void *X_dev, int f32, pmh_csr Xcsr, const double *y_dev, const pmh_svm_opts *opts, pmh_svm *out)
{
  if (opts->loss_type != PMH_SVM_LOSS_L1 && opts->loss_type != PMH_SVM_LOSS_L2) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_create: unknown loss type %d (PMH_SVM_LOSS_L1 | PMH_SVM_LOSS_L2)", opts->loss_type);
  if (!(opts->C > 0.0)) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_create: C = %g, must be positive", opts->C);
  pmh_svm s = new pmh_svm_s();
  s->ctx = ctx, s->n = n_local, s->d = d, s->X = X_dev, s->f32 = f32, s->Xcsr = Xcsr, s->y = y_dev, s->o = *opts;
  memset(&s->st, 0, sizeof(s->st));
  const int    n  = n_local;
  const size_t nb = sizeof(double) * (size_t)(n ? n : 1);
  int          rc = PMH_SUCCESS;
  do {
    if ((rc = Xcsr ? pmh_op_create_svm_dual_csr(ctx, Xcsr, y_dev, &s->H) : (f32 ? pmh_op_create_svm_dual_f32(ctx, n, d, (const float *)X_dev, y_dev, &s->H) : pmh_op_create_svm_dual(ctx, n, d, (const double *)X_dev, y_dev, &s->H)))) break;
    if ((rc = svm_refresh_l2(s))) break;
    if ((rc = pmh_malloc(ctx, nb, (void **)&s->alpha)) || (rc = pmh_malloc(ctx, nb, (void **)&s->rhs)) || (rc = pmh_malloc(ctx, nb, (void **)&s->lb))) break;
    if ((rc = pmh_malloc(ctx, sizeof(double) * (size_t)d, (void **)&s->w)) || (rc = pmh_malloc(ctx, sizeof(double) * 4 * PMH_MAX_VEC_BLOCKS, (void **)&s->part)) || (rc = pmh_malloc(ctx, sizeof(double) * 8, (void **)&s->scal))) break;
    if ((rc = pmh_memset(ctx, s->alpha, 0, nb)) || (rc = pmh_memset(ctx, s->lb, 0, nb)) || (rc = pmh_vec_set(ctx, n, s->rhs, 1.0))) break;
    if (opts->loss_type == PMH_SVM_LOSS_L1) {
      if ((rc = pmh_malloc(ctx, nb, (void **)&s->ub)) || (rc = pmh_vec_set(ctx, n, s->ub, opts->C))) break;
    }
    // the number of samples over all ranks (the row of the equality is y / sqrt(n))
    double ng = (double)n;
    if ((rc = pmh_comm_sum_host(ctx, &ng, 1))) break;
    s->n_global = (long long)ng;
    if (opts->bias) {
      if (s->n_global < 1) {
        rc = pmh_set_error(PMH_ERR_ARG, "pmh_svm_create: no samples");
        break;
      }
      if ((rc = pmh_malloc(ctx, nb, (void **)&s->row)) || (rc = svm_refresh_row(s))) break;
    }
    if ((rc = svm_build_solver(s))) break;
  } while (0);
  if (rc) {
    pmh_svm_destroy(s);
    return rc;
  }
  *out = s;
  return PMH_SUCCESS;
}

static int svm_create_dense(pmh_ctx ctx, int n_local, int d, const void *X_dev, int f32, const double *y_dev, const pmh_svm_opts *opts, pmh_svm *out)
{
  PMH_ARG(ctx && out && opts && n_local >= 0 && d >= 1 && d <= 64 * SVM_KMAX && X_dev && y_dev);
  return svm_create(ctx, n_local, d, X_dev, f32, nullptr, y_dev, opts, out);
}
extern "C" int pmh_svm_create(pmh_ctx ctx, int n_local, int d, const double *X_dev, const double *y_dev, const pmh_svm_opts *opts, pmh_svm *out) { return svm_create_dense(ctx, n_local, d, X_dev, 0, y_dev, opts, out); }
extern "C" int pmh_svm_create_f32(pmh_ctx ctx, int n_local, int d, const float *X_dev, const double *y_dev, const pmh_svm_opts *opts, pmh_svm *out) { return svm_create_dense(ctx, n_local, d, X_dev, 1, y_dev, opts, out); }

extern "C" int pmh_svm_create_csr(pmh_ctx ctx, pmh_csr X, const double *y_dev, const pmh_svm_opts *opts, pmh_svm *out)
{
  PMH_ARG(ctx && out && opts && X && y_dev && X->ctx == ctx);
  if (X->ncols < 1) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_create_csr: the sample matrix has no columns");
  return svm_create(ctx, X->nrows, X->ncols, nullptr, 0, X, y_dev, opts, out);
}

// scal[0..3] = the sums over all workgroups and ranks of the four rows a bias / predict kernel left in part[4][nb] (n == 0: no kernel ran, zeros)
static int svm_sum_part(pmh_svm s, int n, int nb)
{
  if (n > 0) PMH_CHK(pmh_svm_sum_rows(s->ctx, nb, 4, s->part, s->scal));
  else PMH_CHK(pmh_memset(s->ctx, s->scal, 0, sizeof(double) * 4));
  return pmh_comm_allreduce_sum(s->ctx, s->scal, 4);
}

// w, b and the counts from the current alpha
static int svm_model(pmh_svm s)
{
  pmh_ctx       ctx = s->ctx;
  SvmDualBase  *H   = static_cast<SvmDualBase *>(s->H);
  const double *w   = nullptr;
  PMH_CHK(H->form_w(s->alpha, &w));
  PMH_CHK(pmh_vec_copy(ctx, s->d, w, s->w));
  s->h_w.resize((size_t)s->d);
  const int    nb    = SVM_NB(s->n);
  const double astol = s->sx ? s->o.smalxe.inner.astol : s->o.mpgp.astol, ubound = s->o.loss_type == PMH_SVM_LOSS_L1 ? s->o.C : 0.0;
  const double *ubv  = s->o.loss_type == PMH_SVM_LOSS_L1 ? s->Cv : nullptr; // per-sample penalties: free means a_i < C_i - astol
  if (s->n > 0 && s->Xcsr) {
    if (!s->dots) PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)s->n, (void **)&s->dots));
    PMH_CHK(pmh_svm_csr_op_row_dots(H, s->w, s->dots));
    hipLaunchKernelGGL((ubv ? k_svm_bias_dots<1> : k_svm_bias_dots<0>), dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, s->n, (const double *)s->dots, s->y, (const double *)s->alpha, astol, ubound, ubv, s->part);
  } else if (s->n > 0) {
    H->npass++;
    svm_const<2>(ubv != nullptr, [&](auto U) {
      svm_const<2>(s->f32, [&](auto F) {
        using T = svm_sample_t<decltype(F)>;
        hipLaunchKernelGGL((k_svm_bias<decltype(U)::value, T>), dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, s->n, s->d, (const T *)s->X, s->y, (const double *)s->w, (const double *)s->alpha, astol, ubound, ubv, s->part);
      });
    });
  }
  PMH_CHK(svm_sum_part(s, s->n, nb));
  // the equality's multiplier: SMALXE keeps B'mu = mu row (the Lagrangian is 1/2 a'Ha - 1'a + mu (row'a)), so mu = row'(B'mu) / (row'row) and, with
  // row = y / sqrt(n), stationarity in a free sample reads y_i - x_i . w = mu / sqrt(n): b = mu / sqrt(n)
  if (s->sx) {
    double *Btmu = nullptr;
    PMH_CHK(pmh_smalxe_get_penalized(s->sx, nullptr, nullptr, &Btmu));
    PMH_CHK(pmh_onerow_dot(s->pf, Btmu, 1.0 / s->pf->row_aat, s->scal + 4));
  } else PMH_CHK(pmh_memset(ctx, s->scal + 4, 0, sizeof(double)));
  double h[5];
  PMH_CHK(pmh_memcpy_d2h(ctx, h, s->scal, sizeof(h)));
  PMH_CHK(pmh_memcpy_d2h(ctx, s->h_w.data(), s->w, sizeof(double) * (size_t)s->d));
  s->st.yTalpha = h[1], s->st.n_free_sv = (long long)h[2], s->st.n_sv = (long long)h[3];
  s->st.b_multiplier = h[4] / sqrt((double)(svm_n_posed(s) > 0 ? svm_n_posed(s) : 1)); // (the row is y / sqrt(n), over the subset: n_S)
  s->st.b_free       = h[2] > 0.0 ? h[0] / h[2] : NAN;
  if (!s->o.bias) s->b = 0.0;
  else s->b = h[2] > 0.0 ? s->st.b_free : s->st.b_multiplier;
  s->st.b = s->b;
  return PMH_SUCCESS;
}

// The start vector of a warm training from the handle's last dual: a0_i = m_i ? min(max(scale alpha_i, 0), ub_i) : 0, in this order of operations (m: the subset
// mask, nullptr: all ones; ub: the upper bounds, nullptr: none), and how many entries the mask zeroed that were not zero (cnt[0]) and how many were clipped at
// ub (cnt[1]).  alpha and a0 may be the same array
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_warm_start(int n, const double *alpha, const double *__restrict__ m, const double *__restrict__ ub, double scale, double *a0, int *__restrict__ cnt)
{
  int nm = 0, nc = 0;
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    const double ai = alpha[i];
    double       v  = 0.0;
    if (!m || m[i] != 0.0) {
      v = fmax(scale * ai, 0.0);
      if (ub && v > ub[i]) v = ub[i], nc++;
    } else if (ai != 0.0) nm++;
    a0[i] = v;
  }
  if (nm) atomicAdd(cnt, nm);
  if (nc) atomicAdd(cnt + 1, nc);
}

// the one place the start vector is formed: pmh_svm_warm_start_vector (a0: the caller's) and pmh_svm_train_warm (a0 = alpha, in place)
static int svm_warm_start(pmh_svm s, const char *who, double scale, double *a0)
{
  if (!(scale > 0.0) || !std::isfinite(scale)) return pmh_set_error(PMH_ERR_ARG, "%s: alpha_scale = %g, must be positive and finite", who, scale);
  if (!s->has_dual) return pmh_set_error(PMH_ERR_STATE, "%s: the handle holds no dual of its current labels (call pmh_svm_train first; pmh_svm_set_labels drops the dual)", who);
  pmh_ctx ctx = s->ctx;
  if (!s->ws_cnt) PMH_CHK(pmh_malloc(ctx, sizeof(int) * 2, (void **)&s->ws_cnt));
  PMH_CHK(pmh_memset(ctx, s->ws_cnt, 0, sizeof(int) * 2));
  if (s->n > 0) {
    hipLaunchKernelGGL(k_svm_warm_start, dim3(pmh_vec_grid(s->n)), dim3(PMH_BLOCK), 0, ctx->stream, s->n, (const double *)s->alpha, (const double *)static_cast<SvmDualBase *>(s->H)->msk, (const double *)s->ub, scale, a0, s->ws_cnt);
    PMH_HIP(hipGetLastError());
  }
  int h[2];
  PMH_CHK(pmh_memcpy_d2h(ctx, h, s->ws_cnt, sizeof(h)));
  double c[2] = {(double)h[0], (double)h[1]};
  PMH_CHK(pmh_comm_sum_host(ctx, c, 2));
  s->ws_masked = (long long)c[0], s->ws_clipped = (long long)c[1];
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_warm_start_vector(pmh_svm s, double alpha_scale, double *a0_dev)
{
  PMH_ARG(s && a0_dev);
  return svm_warm_start(s, "pmh_svm_warm_start_vector", alpha_scale, a0_dev);
}

extern "C" int pmh_svm_get_warm_start_counts(pmh_svm s, long long *masked, long long *clipped)
{
  PMH_ARG(s);
  if (masked) *masked = s->ws_masked;
  if (clipped) *clipped = s->ws_clipped;
  return PMH_SUCCESS;
}

// warm: alpha starts as the start vector of its own last value, SMALXE from the last training's multiplier; else both from zero
static int svm_train(pmh_svm s, const char *who, int warm, double alpha_scale)
{
  if (!s->sx && !s->mpgp) return pmh_set_error(PMH_ERR_STATE, "%s: the handle has no solver (an earlier pmh_svm_set_labels / pmh_svm_set_penalties failed)", who);
  const size_t nb = sizeof(double) * (size_t)(s->n ? s->n : 1);
  if (warm) PMH_CHK(svm_warm_start(s, who, alpha_scale, s->alpha)); // (a refusal changes nothing)
  s->calibrated = 0;
  if (!warm) PMH_CHK(pmh_memset(s->ctx, s->alpha, 0, nb));
  s->has_dual = 0; // (until the solve has returned: alpha is an iterate meanwhile)
  long long p0 = 0, p1 = 0;
  PMH_CHK(pmh_op_svm_dual_passes(s->H, &p0));
  if (s->sx) {
    PMH_CHK(pmh_smalxe_reset(s->sx));
    if (warm) {
      // B'mu = mu row with b = mu / sqrt(n_S) (svm_model): the last bias over the CURRENT row m o y / sqrt(n_S), which a new subset has rebuilt -- written into
      // the solver's own B'mu
      double *Btmu = nullptr;
      PMH_CHK(pmh_smalxe_get_penalized(s->sx, nullptr, nullptr, &Btmu));
      if (s->n > 0) hipLaunchKernelGGL(k_svm_fill_row, dim3(pmh_vec_grid(s->n)), dim3(PMH_BLOCK), 0, s->ctx->stream, s->n, (const double *)s->row, s->b_mult * sqrt((double)svm_n_posed(s)), Btmu);
      PMH_HIP(hipGetLastError());
      PMH_CHK(pmh_smalxe_set_initial_multiplier(s->sx, Btmu));
    }
    PMH_CHK(pmh_smalxe_solve(s->sx));
    pmh_smalxe_stats st;
    PMH_CHK(pmh_smalxe_get_stats(s->sx, &st));
    s->st.reason = st.reason, s->st.outer_iterations = st.iteration, s->st.inner_iterations = st.inner_iter_accu;
    s->st.nmv = st.inner.nmv, s->st.ncg = st.inner.ncg, s->st.nexp = st.inner.nexp, s->st.nprop = st.inner.nprop;
    s->st.rho = st.rho, s->st.normBu = st.normBu, s->st.rnorm = st.rnorm;
  } else {
    PMH_CHK(pmh_mpgp_solve(s->mpgp));
    pmh_mpgp_stats st;
    PMH_CHK(pmh_mpgp_get_stats(s->mpgp, &st));
    s->st.reason = st.reason, s->st.outer_iterations = 0, s->st.inner_iterations = st.iteration;
    s->st.nmv = st.nmv, s->st.ncg = st.ncg, s->st.nexp = st.nexp, s->st.nprop = st.nprop;
    s->st.rho = 0.0, s->st.normBu = 0.0, s->st.rnorm = st.rnorm;
  }
  PMH_CHK(pmh_op_svm_dual_passes(s->H, &p1));
  s->st.passes_X = p1 - p0; // the solve's passes over X (the model's two are not counted)
  s->has_dual    = 1;
  PMH_CHK(svm_model(s));
  s->b_mult  = s->st.b_multiplier;
  s->trained = 1;
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_train(pmh_svm s)
{
  PMH_ARG(s);
  return svm_train(s, "pmh_svm_train", 0, 1.0);
}

extern "C" int pmh_svm_train_warm(pmh_svm s, double alpha_scale)
{
  PMH_ARG(s);
  return svm_train(s, "pmh_svm_train_warm", 1, alpha_scale);
}

extern "C" int pmh_svm_get_model(pmh_svm s, double *w_host, double *b)
{
  PMH_ARG(s);
  if (!s->trained) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_get_model: call pmh_svm_train first");
  if (w_host) memcpy(w_host, s->h_w.data(), sizeof(double) * (size_t)s->d);
  if (b) *b = s->b;
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_get_dual(pmh_svm s, double *alpha_dev)
{
  PMH_ARG(s && alpha_dev);
  return pmh_vec_copy(s->ctx, s->n, s->alpha, alpha_dev);
}

extern "C" int pmh_svm_get_stats(pmh_svm s, pmh_svm_stats *st)
{
  PMH_ARG(s && st);
  *st = s->st;
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_get_solver(pmh_svm s, pmh_op *H, pmh_qppf *pf, pmh_mpgp *mpgp, pmh_smalxe *smalxe)
{
  PMH_ARG(s);
  if (H) *H = s->H;
  if (pf) *pf = s->pf;
  if (mpgp) *mpgp = s->mpgp;
  if (smalxe) *smalxe = s->sx;
  return PMH_SUCCESS;
}

// ---- per-class and per-sample penalties ---------------------------------------------------------------------------------------------------------------------
// how many weights are not positive and finite, or give a C_i = c_{y_i} weight_i that is not (a count: any order gives the same integer)
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_weights_bad(int n, const double *__restrict__ y, const double *__restrict__ weight, double cpos, double cneg, int *__restrict__ bad)
{
  int b = 0;
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    const double wi = weight[i], ci = (y[i] > 0.0 ? cpos : cneg) * wi;
    b += (wi > 0.0 && isfinite(wi) && ci > 0.0 && isfinite(ci)) ? 0 : 1;
  }
  if (b) atomicAdd(bad, b);
}
// Cv_i = (y_i > 0 ? cpos : cneg) weight_i (weight == nullptr: 1); ub / Cinv where given: ub_i = Cv_i, Cinv_i = 1 / Cv_i
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_fill_penalties(int n, const double *__restrict__ y, const double *__restrict__ weight, double cpos, double cneg, double *__restrict__ Cv,
                                                                  double *__restrict__ ub, double *__restrict__ Cinv)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    const double ci = (y[i] > 0.0 ? cpos : cneg) * (weight ? weight[i] : 1.0);
    Cv[i] = ci;
    if (ub) ub[i] = ci;
    if (Cinv) Cinv[i] = 1.0 / ci;
  }
}

extern "C" int pmh_svm_set_penalties(pmh_svm s, double C_pos, double C_neg, const double *weight_dev)
{
  PMH_ARG(s);
  if (!(C_pos > 0.0) || !std::isfinite(C_pos)) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_set_penalties: C_pos = %g, must be positive and finite", C_pos);
  if (!(C_neg > 0.0) || !std::isfinite(C_neg)) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_set_penalties: C_neg = %g, must be positive and finite", C_neg);
  pmh_ctx      ctx = s->ctx;
  const int    n   = s->n;
  const size_t nb  = sizeof(double) * (size_t)(n ? n : 1);
  const bool   L2  = s->o.loss_type == PMH_SVM_LOSS_L2;
  if (weight_dev) {
    // every rank decides alike: the counts are summed over the communicator before anything is changed
    int  bad   = 0;
    int *d_bad = nullptr;
    PMH_CHK(pmh_malloc(ctx, sizeof(int), (void **)&d_bad));
    int rc = pmh_memset(ctx, d_bad, 0, sizeof(int));
    if (!rc && n > 0) {
      hipLaunchKernelGGL(k_svm_weights_bad, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, s->y, weight_dev, C_pos, C_neg, d_bad);
      if (hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "pmh_svm_set_penalties: the launch that checks the weights failed");
    }
    if (!rc) rc = pmh_memcpy_d2h(ctx, &bad, d_bad, sizeof(int));
    pmh_free(ctx, d_bad);
    PMH_CHK(rc);
    double nbad = (double)bad;
    PMH_CHK(pmh_comm_sum_host(ctx, &nbad, 1));
    if (nbad != 0.0)
      return pmh_set_error(PMH_ERR_ARG, "pmh_svm_set_penalties: %lld of the sample weights are not positive and finite (or give a penalty C_i that is not); a zero weight does not leave a sample out: pmh_svm_set_subset does",
                           (long long)nbad);
  }
  if (!s->Cv) PMH_CHK(pmh_malloc(ctx, nb, (void **)&s->Cv));
  if (L2 && !s->Cinv) PMH_CHK(pmh_malloc(ctx, nb, (void **)&s->Cinv));
  s->trained = s->calibrated = 0;
  if (n > 0) {
    hipLaunchKernelGGL(k_svm_fill_penalties, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, s->y, weight_dev, C_pos, C_neg, s->Cv, L2 ? nullptr : s->ub, L2 ? s->Cinv : nullptr);
    PMH_HIP(hipGetLastError());
  }
  PMH_CHK(svm_refresh_l2(s)); // the diagonal 1 / C_i in place of the scalar 1 / C (under a subset m_i / C_i)
  return svm_build_solver(s);
}

extern "C" int pmh_svm_get_penalties(pmh_svm s, double *c_dev)
{
  PMH_ARG(s && c_dev);
  if (s->Cv) return pmh_vec_copy(s->ctx, s->n, s->Cv, c_dev);
  return pmh_vec_set(s->ctx, s->n, c_dev, s->o.C);
}

// New labels on the created handle: everything svm_create derived from y is redone by the calls svm_create makes (svm_refresh_l2, svm_refresh_row,
// svm_build_solver) after the operator's labels and the penalties, which go back to the scalar C: a training afterwards gives what a fresh handle on (X, y_dev)
// gives, bit for bit
extern "C" int pmh_svm_set_labels(pmh_svm s, const double *y_dev)
{
  PMH_ARG(s && y_dev);
  pmh_ctx   ctx = s->ctx;
  const int n   = s->n;
  s->trained = s->calibrated = 0;
  s->has_dual = 0; // alpha belongs to the old labels: no warm start from it
  svm_drop_solver(s);
  PMH_CHK(pmh_op_svm_dual_set_labels(s->H, y_dev));
  s->y = y_dev;
  if (s->o.loss_type != PMH_SVM_LOSS_L2) PMH_CHK(pmh_vec_set(ctx, n, s->ub, s->o.C));
  if (s->Cv) pmh_free(ctx, s->Cv), s->Cv = nullptr;
  if (s->Cinv) pmh_free(ctx, s->Cinv), s->Cinv = nullptr;
  PMH_CHK(svm_refresh_l2(s)); // (a subset stays: the operator rebuilt its masked labels, the diagonal is m_i / C again)
  PMH_CHK(svm_refresh_row(s));
  return svm_build_solver(s);
}

// ---- sample subsets ----------------------------------------------------------------------------------------------------------------------------------------
// Train on the subset S of the handle's samples, X staying where it is: the operator becomes H_S = M (H + D) M (pmh_op_svm_dual_set_subset), rhs = m, the
// equality's row the masked labels over sqrt(n_S), L2 the diagonal m_i / C_i; L1 keeps its bounds.  From alpha = 0 every iterate, gradient and direction of
// the solvers is then zero on the held-out rows, so the multiplier, the free support vectors and n_sv are those of S.  The solver is built anew as by
// pmh_svm_set_penalties: the eigenvalue estimate must be H_S's.  A refused mask leaves the handle as it was
extern "C" int pmh_svm_set_subset(pmh_svm s, const double *m_dev)
{
  PMH_ARG(s);
  pmh_ctx      ctx = s->ctx;
  SvmDualBase *H   = static_cast<SvmDualBase *>(s->H);
  PMH_CHK(pmh_op_svm_dual_set_subset(s->H, m_dev)); // (checks the mask before anything changes; the solvers only hold the operator)
  s->trained = s->calibrated = 0;
  svm_drop_solver(s);
  s->n_sub = 0;
  if (m_dev) {
    double ns = (double)H->n_sub; // all-reduced as n_global is
    PMH_CHK(pmh_comm_sum_host(ctx, &ns, 1));
    s->n_sub = (long long)ns;
    PMH_CHK(pmh_vec_copy(ctx, s->n, H->msk, s->rhs));
  } else PMH_CHK(pmh_vec_set(ctx, s->n, s->rhs, 1.0));
  PMH_CHK(svm_refresh_l2(s));
  PMH_CHK(svm_refresh_row(s));
  return svm_build_solver(s);
}

extern "C" int pmh_svm_get_subset(pmh_svm s, double *m_dev, long long *n_in)
{
  PMH_ARG(s);
  SvmDualBase *H = static_cast<SvmDualBase *>(s->H);
  if (n_in) *n_in = svm_n_posed(s);
  if (!m_dev) return PMH_SUCCESS;
  return H->msk ? pmh_vec_copy(s->ctx, s->n, H->msk, m_dev) : pmh_vec_set(s->ctx, s->n, m_dev, 1.0);
}

void pmh_svm_own_samples(pmh_svm s, const void **X, int *f32, pmh_csr *Xcsr, const double **msk)
{
  if (X) *X = s->X;
  if (f32) *f32 = s->f32;
  if (Xcsr) *Xcsr = s->Xcsr;
  if (msk) *msk = static_cast<SvmDualBase *>(s->H)->msk;
}

// X (dense rows, n x d: doubles, or floats where f32 -- the test samples' type, whatever the handle was trained on) or Xt (CSR)
// own: the handle's own samples (X or, CSR, the operator's tables: Xt == nullptr); sel: which of them the counts are taken over
static int svm_predict(pmh_svm s, int n, const void *X, int f32, pmh_csr Xt, double *scores, double *labels, const double *ytrue, long long *counts, bool own = false, svm_sel sel = svm_sel())
{
  PMH_ARG(s && n >= 0 && (X || Xt || n == 0 || own));
  if (!s->trained) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_predict: call pmh_svm_train first");
  if (!own) PMH_CHK(pmh_svm_check_test_samples("pmh_svm_predict", s->d, Xt));
  const int nb = SVM_NB(n);
  if (n > 0 && (Xt || (own && s->Xcsr))) {
    double *dots = scores; // the dot products land where the scores go; without scores in a buffer of this call
    if (!dots) PMH_CHK(pmh_malloc(s->ctx, sizeof(double) * (size_t)n, (void **)&dots));
    int rc = Xt ? pmh_svm_csr_row_dots(Xt, s->w, dots) : pmh_svm_csr_op_row_dots(static_cast<SvmDualBase *>(s->H), s->w, dots);
    if (!rc) {
      hipLaunchKernelGGL(k_svm_predict_dots, dim3(nb), dim3(PMH_BLOCK), 0, s->ctx->stream, n, (const double *)dots, s->b, scores, labels, ytrue, s->part, sel);
      if (hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "pmh_svm_predict_csr: the launch failed");
    }
    if (!scores) pmh_free(s->ctx, dots);
    PMH_CHK(rc);
  } else if (n > 0) {
    svm_const<2>(f32, [&](auto F) {
      using T = svm_sample_t<decltype(F)>;
      if (s->d == 64) hipLaunchKernelGGL(k_svm_predict64<T>, dim3(nb), dim3(PMH_BLOCK), 0, s->ctx->stream, n, (const T *)X, (const double *)s->w, s->b, scores, labels, ytrue, s->part, sel);
      else hipLaunchKernelGGL(k_svm_predict<T>, dim3(nb), dim3(PMH_BLOCK), 0, s->ctx->stream, n, s->d, (const T *)X, (const double *)s->w, s->b, scores, labels, ytrue, s->part, sel);
    });
    PMH_HIP(hipGetLastError());
  }
  if (!counts) return PMH_SUCCESS;
  PMH_CHK(svm_sum_part(s, n, nb));
  double h[4];
  PMH_CHK(pmh_memcpy_d2h(s->ctx, h, s->scal, sizeof(h)));
  for (int k = 0; k < 4; k++) counts[k] = (long long)h[k];
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_predict(pmh_svm s, int n, const double *X_dev, double *scores_dev, double *labels_dev) { return svm_predict(s, n, X_dev, 0, nullptr, scores_dev, labels_dev, nullptr, nullptr); }
extern "C" int pmh_svm_predict_f32(pmh_svm s, int n, const float *X_dev, double *scores_dev, double *labels_dev) { return svm_predict(s, n, X_dev, 1, nullptr, scores_dev, labels_dev, nullptr, nullptr); }

extern "C" int pmh_svm_predict_csr(pmh_svm s, pmh_csr Xt, double *scores_dev, double *labels_dev)
{
  PMH_ARG(s && Xt);
  return svm_predict(s, Xt->nrows, nullptr, 0, Xt, scores_dev, labels_dev, nullptr, nullptr);
}

extern "C" int pmh_svm_test_csr(pmh_svm s, pmh_csr Xt, const double *y_dev, long long counts[4])
{
  PMH_ARG(s && Xt && y_dev && counts);
  return svm_predict(s, Xt->nrows, nullptr, 0, Xt, nullptr, nullptr, y_dev, counts);
}

extern "C" int pmh_svm_test(pmh_svm s, int n, const double *X_dev, const double *y_dev, long long counts[4])
{
  PMH_ARG(y_dev && counts);
  return svm_predict(s, n, X_dev, 0, nullptr, nullptr, nullptr, y_dev, counts);
}
extern "C" int pmh_svm_test_f32(pmh_svm s, int n, const float *X_dev, const double *y_dev, long long counts[4])
{
  PMH_ARG(y_dev && counts);
  return svm_predict(s, n, X_dev, 1, nullptr, nullptr, nullptr, y_dev, counts);
}

// the handle's own samples, nothing uploaded: the predict sweep over the X the handle was created on (CSR: the row sweep with the operator's tables)
extern "C" int pmh_svm_predict_own(pmh_svm s, double *scores_dev, double *labels_dev)
{
  PMH_ARG(s);
  return svm_predict(s, s->n, s->X, s->f32, nullptr, scores_dev, labels_dev, nullptr, nullptr, true);
}

extern "C" int pmh_svm_test_own(pmh_svm s, int which, long long counts[4])
{
  PMH_ARG(s && counts);
  if (which != PMH_SVM_OWN_HELD_OUT && which != PMH_SVM_OWN_SUBSET && which != PMH_SVM_OWN_ALL) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_test_own: which = %d (PMH_SVM_OWN_HELD_OUT | PMH_SVM_OWN_SUBSET | PMH_SVM_OWN_ALL)", which);
  SvmDualBase *H = static_cast<SvmDualBase *>(s->H);
  if (which == PMH_SVM_OWN_HELD_OUT && !H->msk) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_test_own: no subset is set (pmh_svm_set_subset), so no sample is held out");
  svm_sel sel;
  if (which != PMH_SVM_OWN_ALL && H->msk) sel.m = H->msk, sel.want = which == PMH_SVM_OWN_SUBSET ? 1.0 : 0.0;
  return svm_predict(s, s->n, s->X, s->f32, nullptr, nullptr, nullptr, s->y, counts, true, sel);
}

// ---- probabilities (Platt scaling, svm_proba.hip) ---------------------------------------------------------------------------------------------------------------
// the scores of the calibration samples by the predict path, then the fit on them
static int svm_calibrate(pmh_svm s, int n, const void *X, int f32, pmh_csr Xt, const double *y)
{
  PMH_ARG(s && n >= 0 && (X || Xt || n == 0) && (y || n == 0));
  if (!s->trained) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_calibrate: call pmh_svm_train first");
  double *scores = nullptr;
  PMH_CHK(pmh_malloc(s->ctx, sizeof(double) * (size_t)(n ? n : 1), (void **)&scores));
  double              A = 0.0, B = 0.0;
  pmh_svm_platt_stats st;
  int                 rc = svm_predict(s, n, X, f32, Xt, scores, nullptr, nullptr, nullptr);
  if (!rc) rc = pmh_svm_platt_fit(s->ctx, n, scores, y, &A, &B, &st);
  pmh_free(s->ctx, scores);
  PMH_CHK(rc);
  s->cal_A = A, s->cal_B = B, s->cal_st = st, s->calibrated = 1;
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_calibrate(pmh_svm s, int n, const double *X_dev, const double *y_dev) { return svm_calibrate(s, n, X_dev, 0, nullptr, y_dev); }
extern "C" int pmh_svm_calibrate_f32(pmh_svm s, int n, const float *X_dev, const double *y_dev) { return svm_calibrate(s, n, X_dev, 1, nullptr, y_dev); }

extern "C" int pmh_svm_calibrate_csr(pmh_svm s, pmh_csr Xt, const double *y_dev)
{
  PMH_ARG(s && Xt);
  return svm_calibrate(s, Xt->nrows, nullptr, 0, Xt, y_dev);
}

extern "C" int pmh_svm_set_calibration(pmh_svm s, double A, double B)
{
  PMH_ARG(s);
  if (!std::isfinite(A) || !std::isfinite(B)) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_set_calibration: A = %g, B = %g, both must be finite", A, B);
  if (!s->trained) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_set_calibration: call pmh_svm_train first (a calibration belongs to a model)");
  memset(&s->cal_st, 0, sizeof(s->cal_st));
  s->cal_A = A, s->cal_B = B, s->calibrated = 1;
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_get_calibration(pmh_svm s, double *A, double *B, pmh_svm_platt_stats *st)
{
  PMH_ARG(s);
  if (!s->calibrated) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_get_calibration: call pmh_svm_calibrate or pmh_svm_set_calibration first");
  if (A) *A = s->cal_A;
  if (B) *B = s->cal_B;
  if (st) *st = s->cal_st;
  return PMH_SUCCESS;
}

// X (dense rows, n x d: doubles, or floats where f32) or Xt (CSR): one pass over the samples
static int svm_predict_proba(pmh_svm s, int n, const void *X, int f32, pmh_csr Xt, double *proba)
{
  PMH_ARG(s && n >= 0 && (X || Xt || n == 0) && (proba || n == 0));
  if (!s->trained) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_predict_proba: call pmh_svm_train first");
  if (!s->calibrated) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_predict_proba: call pmh_svm_calibrate or pmh_svm_set_calibration first");
  PMH_CHK(pmh_svm_check_test_samples("pmh_svm_predict", s->d, Xt));
  if (n == 0) return PMH_SUCCESS;
  pmh_ctx   ctx = s->ctx;
  const int nb  = SVM_NB(n);
  if (Xt) {
    PMH_CHK(pmh_svm_csr_row_dots(Xt, s->w, proba));
    hipLaunchKernelGGL(k_svm_proba_dots, dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, n, s->b, s->cal_A, s->cal_B, proba);
  } else
    svm_const<2>(f32, [&](auto F) {
      using T = svm_sample_t<decltype(F)>;
      if (s->d == 64) hipLaunchKernelGGL(k_svm_proba64<T>, dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, n, (const T *)X, (const double *)s->w, s->b, s->cal_A, s->cal_B, proba);
      else hipLaunchKernelGGL(k_svm_proba<T>, dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, n, s->d, (const T *)X, (const double *)s->w, s->b, s->cal_A, s->cal_B, proba);
    });
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

extern "C" int pmh_svm_predict_proba(pmh_svm s, int n, const double *X_dev, double *proba_dev) { return svm_predict_proba(s, n, X_dev, 0, nullptr, proba_dev); }
extern "C" int pmh_svm_predict_proba_f32(pmh_svm s, int n, const float *X_dev, double *proba_dev) { return svm_predict_proba(s, n, X_dev, 1, nullptr, proba_dev); }

extern "C" int pmh_svm_predict_proba_csr(pmh_svm s, pmh_csr Xt, double *proba_dev)
{
  PMH_ARG(s && Xt);
  return svm_predict_proba(s, Xt->nrows, nullptr, 0, Xt, proba_dev);
}
