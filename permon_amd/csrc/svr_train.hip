// SVR front end: linear epsilon-insensitive support vector regression over the dual operators of svr.hip, the route of svm_train.hip:
//   dual in u = [p; q]:  min 1/2 u'H^u - c^'u,  c^ = [t - eps; -t - eps],  L1: 0 <= u <= [C_i; C_i] (D = 0),  L2: 0 <= u (D = diag(1 / C_i))
//   bias: additionally sum (p_i - q_i) = 0, posed as ([1; -1] / sqrt(2 n))'u = 0 -- a one-row projector under SMALXE whose penalty term the operator absorbs
// No bias: MPGP on the box alone.  Model: w = X'(p - q) by the operator's pass 1; b by one pass over X (k_svr_bias: the sums of svr_bias_row); prediction and
// the regression metrics by one pass over the test samples (k_svr_score / k_svr_score64 on the sweeps of svm_rows.h).  Samples in CSR: x_i . w by the
// entry-balanced row sweep of svm_csr.hip, then one kernel over the n dot products (k_svr_bias_dots, k_svr_score_dots).  Dense samples in float32: the same
// kernels with the sample type as template argument.  Every sum leaves a workgroup through svr_store and is finished by one workgroup in a fixed order.
#include <cmath>

#include "svr_internal.h"
#include "svm_rows.h"

struct pmh_svr_s {
  pmh_ctx       ctx;
  int           n, d; // samples of this rank, features
  long long     n_global;
  const void   *X; // dense rows: doubles, or floats where f32
  int           f32 = 0;
  pmh_csr       Xcsr = nullptr; // the samples in CSR (then X == nullptr), borrowed
  const double *t;
  pmh_svr_opts  o;
  pmh_op        H    = nullptr;
  pmh_qppf      pf   = nullptr;
  pmh_mpgp      mpgp = nullptr;
  pmh_smalxe    sx   = nullptr;
  double       *u = nullptr, *rhs = nullptr, *lb = nullptr, *ub = nullptr, *row = nullptr; // 2 n each (ub: L1 only; row: bias only)
  double       *w = nullptr, *part = nullptr, *scal = nullptr, *dots = nullptr;
  double       *Cv = nullptr, *Cinv = nullptr; // pmh_svr_set_penalties: C_i and, L2, 1 / C_i (n doubles); nullptr: opts.C everywhere
  std::vector<double> h_w;
  double        b = 0.0;
  int           trained = 0;
  pmh_svr_stats st;
};

#define SVR_NSUM 7 // the most sums a kernel here leaves per workgroup (k_svr_score); the bias kernels leave 4

// K sums of a thread reduced over the workgroup one after the other -> part[K][gridDim.x]; MINROW: that row is a minimum (max |r| travels as -|r|)
template <int K, int MINROW = -1> static __device__ __forceinline__ void svr_store(const double (&s)[K], double *red, double *__restrict__ part)
{
#pragma unroll
  for (int k = 0; k < K; k++) {
    const double r = k == MINROW ? pmh_block_reduce<PMH_RED_MIN>(s[k], red) : pmh_block_reduce<PMH_RED_SUM>(s[k], red);
    if (threadIdx.x == 0) part[(size_t)k * gridDim.x + blockIdx.x] = r;
  }
}
// out[k] = sum (k == minrow: min) over b of part[k][b]: one workgroup, fixed order
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_finish(int nb, int K, int minrow, const double *__restrict__ part, double *__restrict__ out)
{
  __shared__ double red[PMH_BLOCK / 64];
  for (int k = 0; k < K; k++) {
    const bool mn = k == minrow;
    double     v  = mn ? INFINITY : 0.0;
    for (int b = threadIdx.x; b < nb; b += PMH_BLOCK) v = mn ? fmin(v, part[(size_t)k * nb + b]) : v + part[(size_t)k * nb + b];
    v = mn ? pmh_block_reduce<PMH_RED_MIN>(v, red) : pmh_block_reduce<PMH_RED_SUM>(v, red);
    if (threadIdx.x == 0) out[k] = v;
  }
}

// ---- the bias -------------------------------------------------------------------------------------------------------------------------------------------------
struct svr_bias_args {
  const double *t, *p, *q, *ubv, *dv; // ubv: the upper bound of sample i (per-sample penalties, L1) or nullptr: ub; dv: D_i (L2) or nullptr: dsc
  double        eps, astol, ub, dsc;  // ub <= 0: no upper bound (L2); dsc: the scalar D (L1: 0)
};
// sample i with dot = x_i . w in s[0]: the sum over the free entries of t_i - eps - D_i p_i - dot (a free p_i) and t_i + eps + D_i q_i - dot (a free q_i), each
// evaluated left to right; s[1]: sum (p_i - q_i); s[2]: free entries; s[3]: entries above astol.  free: astol < u_k and (ub > 0: u_k < ub - astol)
static __device__ __forceinline__ void svr_bias_row(const svr_bias_args &a, long long i, double dot, double (&s)[4])
{
  const double pi = a.p[i], qi = a.q[i], ti = a.t[i], ub = a.ubv ? a.ubv[i] : a.ub, D = a.dv ? a.dv[i] : a.dsc;
  s[1] += pi - qi;
  if (pi > a.astol) {
    s[3] += 1.0;
    if (!(ub > 0.0) || pi < ub - a.astol) s[2] += 1.0, s[0] += ((ti - a.eps) - D * pi) - dot;
  }
  if (qi > a.astol) {
    s[3] += 1.0;
    if (!(ub > 0.0) || qi < ub - a.astol) s[2] += 1.0, s[0] += ((ti + a.eps) + D * qi) - dot;
  }
}
// One pass over X for the bias -> part[4][gridDim.x]
template <class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_bias(int n, int d, const T *__restrict__ X, const double *__restrict__ w, svr_bias_args a, double *__restrict__ part)
{
  __shared__ double red[PMH_BLOCK / 64];
  double            s[4] = {0.0, 0.0, 0.0, 0.0};
  svm_sweep_rows(n, d, X, w, [&](long long i, double dot) { svr_bias_row(a, i, dot, s); });
  svr_store<4>(s, red, part);
}
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_bias_dots(int n, const double *__restrict__ dots, svr_bias_args a, double *__restrict__ part)
{
  __shared__ double red[PMH_BLOCK / 64];
  double            s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) svr_bias_row(a, i, dots[i], s);
  svr_store<4>(s, red, part);
}

// ---- prediction and the metrics ---------------------------------------------------------------------------------------------------------------------------------
// sample i with the score f = x_i . w + b: f -> scores (where given) and, with targets, r = f - t_i in the seven sums: sum r, sum r^2, sum |r|, -max |r|, sum t,
// sum t^2, the count of |r| <= eps.  No __restrict__ on scores: the CSR form reads the dot products from the array the scores go to
static __device__ __forceinline__ void svr_score_row(long long i, double f, double *scores, const double *__restrict__ t, double eps, double (&s)[SVR_NSUM])
{
  if (scores) scores[i] = f;
  if (t) {
    const double ti = t[i], r = f - ti, ar = fabs(r);
    s[0] += r, s[1] += r * r, s[2] += ar, s[3] = fmin(s[3], -ar), s[4] += ti, s[5] += ti * ti, s[6] += ar <= eps ? 1.0 : 0.0;
  }
}
#define SVR_SUMS_INIT {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0} // (-max |r| starts at -0: no sample, max 0)
template <class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_score(int n, int d, const T *__restrict__ X, const double *__restrict__ w, double b, double *scores, const double *__restrict__ t, double eps,
                                                         double *__restrict__ part)
{
  __shared__ double red[PMH_BLOCK / 64];
  double            s[SVR_NSUM] = SVR_SUMS_INIT;
  svm_sweep_rows(n, d, X, w, [&](long long i, double dot) { svr_score_row(i, dot + b, scores, t, eps, s); });
  if (t) svr_store<SVR_NSUM, 3>(s, red, part); // (uniform: a kernel argument)
}
// d == 64: the row layout of k_svr_x64, four row groups in flight
template <class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_score64(int n, const T *__restrict__ X, const double *__restrict__ w, double b, double *scores, const double *__restrict__ t, double eps,
                                                           double *__restrict__ part)
{
  __shared__ double red[PMH_BLOCK / 64];
  double            s[SVR_NSUM] = SVR_SUMS_INIT;
  svm_sweep_rows64<4>(n, X, w, [&](long long i, double dot) { svr_score_row(i, dot + b, scores, t, eps, s); });
  if (t) svr_store<SVR_NSUM, 3>(s, red, part);
}
// (dots and scores may be the same array)
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_score_dots(int n, const double *dots, double b, double *scores, const double *__restrict__ t, double eps, double *__restrict__ part)
{
  __shared__ double red[PMH_BLOCK / 64];
  double            s[SVR_NSUM] = SVR_SUMS_INIT;
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) svr_score_row(i, dots[i] + b, scores, t, eps, s);
  if (t) svr_store<SVR_NSUM, 3>(s, red, part);
}

// ---- the vectors of the QP ------------------------------------------------------------------------------------------------------------------------------------
// rhs = [t - eps; -t - eps]
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_fill_rhs(int n, const double *__restrict__ t, double eps, double *__restrict__ rhs)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) rhs[i] = t[i] - eps, rhs[n + i] = -t[i] - eps;
}
// row = c [1; -1]
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_fill_row(int n, double c, double *__restrict__ row)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) row[i] = c, row[n + i] = -c;
}
// how many targets are not finite (a count: any order gives the same integer)
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_targets_bad(int n, const double *__restrict__ t, int *__restrict__ bad)
{
  int b = 0;
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) b += isfinite(t[i]) ? 0 : 1;
  if (b) atomicAdd(bad, b);
}
// how many weights are not positive and finite, or give a C_i = C weight_i that is not
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_weights_bad(int n, const double *__restrict__ weight, double C, int *__restrict__ bad)
{
  int b = 0;
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    const double wi = weight[i], ci = C * wi;
    b += (wi > 0.0 && isfinite(wi) && ci > 0.0 && isfinite(ci)) ? 0 : 1;
  }
  if (b) atomicAdd(bad, b);
}
// Cv_i = C weight_i (weight == nullptr: 1); ub where given: both halves C_i; Cinv where given: 1 / C_i
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_fill_penalties(int n, const double *__restrict__ weight, double C, double *__restrict__ Cv, double *__restrict__ ub, double *__restrict__ Cinv)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    const double ci = C * (weight ? weight[i] : 1.0);
    Cv[i] = ci;
    if (ub) ub[i] = ci, ub[n + i] = ci;
    if (Cinv) Cinv[i] = 1.0 / ci;
  }
}
// the count an int-counting kernel leaves (launch: what runs it on d_bad), summed over the ranks so that every rank decides alike
template <class L> static int svr_count_bad(pmh_ctx ctx, const char *who, L launch, long long *nbad)
{
  int  bad   = 0;
  int *d_bad = nullptr;
  PMH_CHK(pmh_malloc(ctx, sizeof(int), (void **)&d_bad));
  int rc = pmh_memset(ctx, d_bad, 0, sizeof(int));
  if (!rc) {
    launch(d_bad);
    if (hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "%s: the launch that checks the values failed", who);
  }
  if (!rc) rc = pmh_memcpy_d2h(ctx, &bad, d_bad, sizeof(int));
  pmh_free(ctx, d_bad);
  PMH_CHK(rc);
  double c = (double)bad;
  PMH_CHK(pmh_comm_sum_host(ctx, &c, 1));
  *nbad = (long long)c;
  return PMH_SUCCESS;
}

extern "C" int pmh_svr_default_opts(pmh_svr_opts *o)
{
  PMH_ARG(o);
  memset(o, 0, sizeof(*o));
  o->loss_type = PMH_SVM_LOSS_L1;
  o->C         = 1.0;
  o->epsilon   = 0.1;
  o->bias      = 1;
  PMH_CHK(pmh_qps_default_opts(&o->qps));
  PMH_CHK(pmh_mpgp_default_opts(&o->mpgp));
  return pmh_smalxe_default_opts(&o->smalxe);
}

extern "C" int pmh_svr_destroy(pmh_svr s)
{
  if (!s) return PMH_SUCCESS;
  if (s->mpgp) pmh_mpgp_destroy(s->mpgp);
  if (s->sx) pmh_smalxe_destroy(s->sx);
  if (s->pf) pmh_qppf_destroy(s->pf);
  if (s->H) pmh_op_destroy(s->H);
  double *v[] = {s->u, s->rhs, s->lb, s->ub, s->row, s->w, s->part, s->scal, s->dots, s->Cv, s->Cinv};
  for (double *p : v)
    if (p) pmh_free(s->ctx, p);
  delete s;
  return PMH_SUCCESS;
}

// The solver over the handle's operator, vectors and projector: SMALXE (bias) or MPGP, built as svm_train.hip builds them.  Both size their steps by the
// operator's largest eigenvalue, estimated at creation: whoever changes the operator's terms builds the solver anew
static int svr_build_solver(pmh_svr s)
{
  if (s->mpgp) pmh_mpgp_destroy(s->mpgp), s->mpgp = nullptr;
  if (s->sx) pmh_smalxe_destroy(s->sx), s->sx = nullptr;
  if (s->o.bias) {
    pmh_smalxe_opts so = s->o.smalxe;
    so.rtol = s->o.qps.rtol, so.atol = s->o.qps.atol, so.divtol = s->o.qps.divtol;
    if (s->o.qps.max_it_set) so.max_it = s->o.qps.max_it;
    return pmh_smalxe_create(s->ctx, s->H, s->rhs, s->u, s->lb, s->ub, s->pf, &so, &s->sx);
  }
  pmh_mpgp_opts mo = s->o.mpgp;
  mo.rtol = s->o.qps.rtol, mo.atol = s->o.qps.atol, mo.divtol = s->o.qps.divtol, mo.max_it = s->o.qps.max_it;
  return pmh_mpgp_create(s->ctx, s->H, s->rhs, s->u, s->lb, s->ub, &mo, &s->mpgp);
}
// L2: the operator's D: the shift 1 / C or the diagonal 1 / C_i
static int svr_refresh_l2(pmh_svr s)
{
  if (s->o.loss_type != PMH_SVM_LOSS_L2) return PMH_SUCCESS;
  if (s->Cinv) {
    PMH_CHK(pmh_op_svr_dual_set_terms(s->H, 0.0, 0.0));
    return pmh_op_svr_dual_set_diag(s->H, s->Cinv);
  }
  PMH_CHK(pmh_op_svr_dual_set_diag(s->H, nullptr));
  return pmh_op_svr_dual_set_terms(s->H, 1.0 / s->o.C, 0.0);
}
static int svr_fill_rhs(pmh_svr s)
{
  if (s->n > 0) hipLaunchKernelGGL(k_svr_fill_rhs, dim3(pmh_vec_grid(s->n)), dim3(PMH_BLOCK), 0, s->ctx->stream, s->n, s->t, s->o.epsilon, s->rhs);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}
static int svr_check_epsilon(const char *who, double eps)
{
  if (!(eps >= 0.0) || !std::isfinite(eps)) return pmh_set_error(PMH_ERR_ARG, "%s: epsilon = %g, must be non-negative and finite", who, eps);
  return PMH_SUCCESS;
}

// X_dev (dense rows: doubles, or floats where f32) or Xcsr
static int svr_create(pmh_ctx ctx, int n, int d, const void *X_dev, int f32, pmh_csr Xcsr, const double *t_dev, const pmh_svr_opts *opts, pmh_svr *out)
{
  if (opts->loss_type != PMH_SVM_LOSS_L1 && opts->loss_type != PMH_SVM_LOSS_L2) return pmh_set_error(PMH_ERR_ARG, "pmh_svr_create: unknown loss type %d (PMH_SVM_LOSS_L1 | PMH_SVM_LOSS_L2)", opts->loss_type);
  if (!(opts->C > 0.0) || !std::isfinite(opts->C)) return pmh_set_error(PMH_ERR_ARG, "pmh_svr_create: C = %g, must be positive and finite", opts->C);
  PMH_CHK(svr_check_epsilon("pmh_svr_create", opts->epsilon));
  long long nbad = 0;
  PMH_CHK(svr_count_bad(ctx, "pmh_svr_create", [&](int *d_bad) {
    if (n > 0) hipLaunchKernelGGL(k_svr_targets_bad, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, t_dev, d_bad);
  }, &nbad));
  if (nbad) return pmh_set_error(PMH_ERR_ARG, "pmh_svr_create: %lld of the targets are not finite", nbad);
  pmh_svr s = new pmh_svr_s();
  s->ctx = ctx, s->n = n, s->d = d, s->X = X_dev, s->f32 = f32, s->Xcsr = Xcsr, s->t = t_dev, s->o = *opts;
  memset(&s->st, 0, sizeof(s->st));
  const size_t nb2 = sizeof(double) * 2 * (size_t)(n ? n : 1);
  int          rc  = PMH_SUCCESS;
  do {
    if ((rc = Xcsr ? pmh_op_create_svr_dual_csr(ctx, Xcsr, &s->H) : (f32 ? pmh_op_create_svr_dual_f32(ctx, n, d, (const float *)X_dev, &s->H) : pmh_op_create_svr_dual(ctx, n, d, (const double *)X_dev, &s->H)))) break;
    if ((rc = svr_refresh_l2(s))) break;
    if ((rc = pmh_malloc(ctx, nb2, (void **)&s->u)) || (rc = pmh_malloc(ctx, nb2, (void **)&s->rhs)) || (rc = pmh_malloc(ctx, nb2, (void **)&s->lb))) break;
    if ((rc = pmh_malloc(ctx, sizeof(double) * (size_t)d, (void **)&s->w)) || (rc = pmh_malloc(ctx, sizeof(double) * SVR_NSUM * PMH_MAX_VEC_BLOCKS, (void **)&s->part)) || (rc = pmh_malloc(ctx, sizeof(double) * 8, (void **)&s->scal))) break;
    if ((rc = pmh_memset(ctx, s->u, 0, nb2)) || (rc = pmh_memset(ctx, s->lb, 0, nb2)) || (rc = svr_fill_rhs(s))) break;
    if (opts->loss_type == PMH_SVM_LOSS_L1) {
      if ((rc = pmh_malloc(ctx, nb2, (void **)&s->ub)) || (rc = pmh_vec_set(ctx, 2 * n, s->ub, opts->C))) break;
    }
    double ng = (double)n; // the number of samples over all ranks (the row of the equality is [1; -1] / sqrt(2 n))
    if ((rc = pmh_comm_sum_host(ctx, &ng, 1))) break;
    s->n_global = (long long)ng;
    if (opts->bias) {
      if (s->n_global < 1) {
        rc = pmh_set_error(PMH_ERR_ARG, "pmh_svr_create: no samples");
        break;
      }
      if ((rc = pmh_malloc(ctx, nb2, (void **)&s->row))) break;
      if (n > 0) hipLaunchKernelGGL(k_svr_fill_row, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, 1.0 / sqrt(2.0 * (double)s->n_global), s->row);
      if (hipGetLastError() != hipSuccess) {
        rc = pmh_set_error(PMH_ERR_HIP, "pmh_svr_create: the launch that fills the equality's row failed");
        break;
      }
      if ((rc = pmh_qppf_create_onerow(ctx, s->row, 2 * n, &s->pf))) break;
    }
    if ((rc = svr_build_solver(s))) break;
  } while (0);
  if (rc) {
    pmh_svr_destroy(s);
    return rc;
  }
  *out = s;
  return PMH_SUCCESS;
}

static int svr_create_dense(pmh_ctx ctx, int n_local, int d, const void *X_dev, int f32, const double *t_dev, const pmh_svr_opts *opts, pmh_svr *out)
{
  PMH_ARG(ctx && out && opts && n_local >= 0 && d >= 1 && d <= 64 * SVM_KMAX && X_dev && t_dev);
  return svr_create(ctx, n_local, d, X_dev, f32, nullptr, t_dev, opts, out);
}
extern "C" int pmh_svr_create(pmh_ctx ctx, int n_local, int d, const double *X_dev, const double *t_dev, const pmh_svr_opts *opts, pmh_svr *out) { return svr_create_dense(ctx, n_local, d, X_dev, 0, t_dev, opts, out); }
extern "C" int pmh_svr_create_f32(pmh_ctx ctx, int n_local, int d, const float *X_dev, const double *t_dev, const pmh_svr_opts *opts, pmh_svr *out) { return svr_create_dense(ctx, n_local, d, X_dev, 1, t_dev, opts, out); }
extern "C" int pmh_svr_create_csr(pmh_ctx ctx, pmh_csr X, const double *t_dev, const pmh_svr_opts *opts, pmh_svr *out)
{
  PMH_ARG(ctx && out && opts && X && t_dev && X->ctx == ctx);
  if (X->ncols < 1) return pmh_set_error(PMH_ERR_ARG, "pmh_svr_create_csr: the sample matrix has no columns");
  return svr_create(ctx, X->nrows, X->ncols, nullptr, 0, X, t_dev, opts, out);
}

extern "C" int pmh_svr_set_penalties(pmh_svr s, double C, const double *weight_dev)
{
  PMH_ARG(s);
  if (!(C > 0.0) || !std::isfinite(C)) return pmh_set_error(PMH_ERR_ARG, "pmh_svr_set_penalties: C = %g, must be positive and finite", C);
  pmh_ctx      ctx = s->ctx;
  const int    n   = s->n;
  const size_t nb  = sizeof(double) * (size_t)(n ? n : 1);
  const bool   L2  = s->o.loss_type == PMH_SVM_LOSS_L2;
  if (weight_dev) {
    long long nbad = 0;
    PMH_CHK(svr_count_bad(ctx, "pmh_svr_set_penalties", [&](int *d_bad) {
      if (n > 0) hipLaunchKernelGGL(k_svr_weights_bad, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, weight_dev, C, d_bad);
    }, &nbad));
    if (nbad) return pmh_set_error(PMH_ERR_ARG, "pmh_svr_set_penalties: %lld of the sample weights are not positive and finite (or give a penalty C_i that is not); a zero weight does not leave a sample out", nbad);
  }
  if (!s->Cv) PMH_CHK(pmh_malloc(ctx, nb, (void **)&s->Cv));
  if (L2 && !s->Cinv) PMH_CHK(pmh_malloc(ctx, nb, (void **)&s->Cinv));
  s->trained = 0;
  if (n > 0) {
    hipLaunchKernelGGL(k_svr_fill_penalties, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, weight_dev, C, s->Cv, L2 ? nullptr : s->ub, L2 ? s->Cinv : nullptr);
    PMH_HIP(hipGetLastError());
  }
  PMH_CHK(svr_refresh_l2(s));
  return svr_build_solver(s);
}

extern "C" int pmh_svr_set_epsilon(pmh_svr s, double epsilon)
{
  PMH_ARG(s);
  PMH_CHK(svr_check_epsilon("pmh_svr_set_epsilon", epsilon));
  s->o.epsilon = epsilon;
  s->trained   = 0;
  PMH_CHK(svr_fill_rhs(s));
  // MPGP takes |c^| for its stopping test at its first solve: asked to take it again.  SMALXE sizes eta by |c^| when it is created: built anew
  if (s->mpgp) return pmh_mpgp_set_tolerances(s->mpgp, s->o.qps.rtol, s->o.qps.atol, s->o.qps.divtol, s->o.qps.max_it);
  return svr_build_solver(s);
}

// scal[0 .. K) = the K rows a kernel left in part[K][nb], finished and joined over the ranks (n == 0: no kernel ran: zeros); minrow as in k_svr_finish
static int svr_sum_part(pmh_svr s, int n, int nb, int K, int minrow)
{
  if (n > 0) {
    hipLaunchKernelGGL(k_svr_finish, dim3(1), dim3(PMH_BLOCK), 0, s->ctx->stream, nb, K, minrow, (const double *)s->part, s->scal);
    PMH_HIP(hipGetLastError()); // (also the launch of the kernel that filled part)
  } else PMH_CHK(pmh_memset(s->ctx, s->scal, 0, sizeof(double) * K));
  if (!pmh_comm_on(s->ctx)) return PMH_SUCCESS;
  int ops[SVR_NSUM];
  for (int k = 0; k < K; k++) ops[k] = k == minrow ? PMH_RED_MIN : PMH_RED_SUM;
  return pmh_comm_allreduce_scalars(s->ctx, s->scal, K, ops);
}

// w, b and the counts from the current u
static int svr_model(pmh_svr s)
{
  pmh_ctx       ctx = s->ctx;
  SvrDualBase  *H   = static_cast<SvrDualBase *>(s->H);
  const double *w   = nullptr;
  const int     n   = s->n;
  PMH_CHK(H->form_w(s->u, &w));
  PMH_CHK(pmh_vec_copy(ctx, s->d, w, s->w));
  s->h_w.resize((size_t)s->d);
  const int     nb = SVM_NB(n);
  const bool    L1 = s->o.loss_type == PMH_SVM_LOSS_L1;
  svr_bias_args a{s->t, s->u, s->u + n, L1 ? s->Cv : nullptr, L1 ? nullptr : s->Cinv, s->o.epsilon, s->sx ? s->o.smalxe.inner.astol : s->o.mpgp.astol, L1 ? s->o.C : 0.0, L1 ? 0.0 : 1.0 / s->o.C};
  if (n > 0 && s->Xcsr) {
    if (!s->dots) PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)n, (void **)&s->dots));
    PMH_CHK(H->row_dots(s->w, s->dots));
    hipLaunchKernelGGL(k_svr_bias_dots, dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, n, (const double *)s->dots, a, s->part);
  } else if (n > 0) {
    H->npass++;
    svm_const<2>(s->f32, [&](auto F) {
      using T = svm_sample_t<decltype(F)>;
      hipLaunchKernelGGL(k_svr_bias<T>, dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, n, s->d, (const T *)s->X, (const double *)s->w, a, s->part);
    });
  }
  PMH_CHK(svr_sum_part(s, n, nb, 4, -1));
  // the equality's multiplier: SMALXE keeps B'mu = mu row, so mu = row'(B'mu) / (row'row); with row = [1; -1] / sqrt(2 n) stationarity in a free p_i reads
  // x_i . w + D_i p_i - (t_i - eps) + mu / sqrt(2 n) = 0: b = mu / sqrt(2 n)
  if (s->sx) {
    double *Btmu = nullptr;
    PMH_CHK(pmh_smalxe_get_penalized(s->sx, nullptr, nullptr, &Btmu));
    PMH_CHK(pmh_onerow_dot(s->pf, Btmu, 1.0 / s->pf->row_aat, s->scal + 4));
  } else PMH_CHK(pmh_memset(ctx, s->scal + 4, 0, sizeof(double)));
  double h[5];
  PMH_CHK(pmh_memcpy_d2h(ctx, h, s->scal, sizeof(h)));
  PMH_CHK(pmh_memcpy_d2h(ctx, s->h_w.data(), s->w, sizeof(double) * (size_t)s->d));
  s->st.sum_beta = h[1], s->st.n_free_sv = (long long)h[2], s->st.n_sv = (long long)h[3];
  s->st.b_multiplier = h[4] / sqrt(2.0 * (double)(s->n_global > 0 ? s->n_global : 1));
  s->st.b_free       = h[2] > 0.0 ? h[0] / h[2] : NAN;
  if (!s->o.bias) s->b = 0.0;
  else s->b = h[2] > 0.0 ? s->st.b_free : s->st.b_multiplier;
  s->st.b = s->b;
  return PMH_SUCCESS;
}

extern "C" int pmh_svr_train(pmh_svr s)
{
  PMH_ARG(s);
  if (!s->sx && !s->mpgp) return pmh_set_error(PMH_ERR_STATE, "pmh_svr_train: the handle has no solver (an earlier pmh_svr_set_penalties / pmh_svr_set_epsilon failed)");
  s->trained = 0;
  PMH_CHK(pmh_memset(s->ctx, s->u, 0, sizeof(double) * 2 * (size_t)(s->n ? s->n : 1)));
  long long p0 = 0, p1 = 0;
  PMH_CHK(pmh_op_svr_dual_passes(s->H, &p0));
  if (s->sx) {
    PMH_CHK(pmh_smalxe_reset(s->sx));
    PMH_CHK(pmh_smalxe_solve(s->sx));
    pmh_smalxe_stats st;
    PMH_CHK(pmh_smalxe_get_stats(s->sx, &st));
    s->st.reason = st.reason, s->st.outer_iterations = st.iteration, s->st.inner_iterations = st.inner_iter_accu;
    s->st.nmv = st.inner.nmv, s->st.ncg = st.inner.ncg, s->st.nexp = st.inner.nexp, s->st.nprop = st.inner.nprop;
    s->st.rho = st.rho, s->st.normBu = st.normBu, s->st.rnorm = st.rnorm;
  } else {
    PMH_CHK(pmh_mpgp_reset_statistics(s->mpgp)); // (the solver may be kept over trainings: the counters are this solve's)
    PMH_CHK(pmh_mpgp_solve(s->mpgp));
    pmh_mpgp_stats st;
    PMH_CHK(pmh_mpgp_get_stats(s->mpgp, &st));
    s->st.reason = st.reason, s->st.outer_iterations = 0, s->st.inner_iterations = st.iteration;
    s->st.nmv = st.nmv, s->st.ncg = st.ncg, s->st.nexp = st.nexp, s->st.nprop = st.nprop;
    s->st.rho = 0.0, s->st.normBu = 0.0, s->st.rnorm = st.rnorm;
  }
  PMH_CHK(pmh_op_svr_dual_passes(s->H, &p1));
  s->st.passes_X = p1 - p0; // the solve's passes over X (the model's two are not counted)
  PMH_CHK(svr_model(s));
  s->trained = 1;
  return PMH_SUCCESS;
}

extern "C" int pmh_svr_get_model(pmh_svr s, double *w_host, double *b)
{
  PMH_ARG(s);
  if (!s->trained) return pmh_set_error(PMH_ERR_STATE, "pmh_svr_get_model: call pmh_svr_train first");
  if (w_host) memcpy(w_host, s->h_w.data(), sizeof(double) * (size_t)s->d);
  if (b) *b = s->b;
  return PMH_SUCCESS;
}

extern "C" int pmh_svr_get_dual(pmh_svr s, double *u_dev)
{
  PMH_ARG(s && u_dev);
  return pmh_vec_copy(s->ctx, 2 * s->n, s->u, u_dev);
}

extern "C" int pmh_svr_get_stats(pmh_svr s, pmh_svr_stats *st)
{
  PMH_ARG(s && st);
  *st = s->st;
  return PMH_SUCCESS;
}

extern "C" int pmh_svr_get_solver(pmh_svr s, pmh_op *H, pmh_qppf *pf, pmh_mpgp *mpgp, pmh_smalxe *smalxe)
{
  PMH_ARG(s);
  if (H) *H = s->H;
  if (pf) *pf = s->pf;
  if (mpgp) *mpgp = s->mpgp;
  if (smalxe) *smalxe = s->sx;
  return PMH_SUCCESS;
}

// X (dense rows, n x d: doubles, or floats where f32 -- the test samples' type, whatever the handle was trained on) or Xt (CSR); t != nullptr: the metrics
static int svr_score(pmh_svr s, const char *who, int n, const void *X, int f32, pmh_csr Xt, double *scores, const double *t, pmh_svr_metrics *m)
{
  PMH_ARG(s && n >= 0 && (X || Xt || n == 0));
  if (!s->trained) return pmh_set_error(PMH_ERR_STATE, "%s: call pmh_svr_train first", who);
  PMH_CHK(pmh_svm_check_test_samples(who, s->d, Xt));
  pmh_ctx      ctx = s->ctx;
  const int    nb  = SVM_NB(n);
  const double eps = s->o.epsilon;
  if (n > 0 && Xt) {
    double *dots = scores; // the dot products land where the scores go; without scores in a buffer of this call
    if (!dots) PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)n, (void **)&dots));
    int rc = pmh_svm_csr_row_dots(Xt, s->w, dots);
    if (!rc) {
      hipLaunchKernelGGL(k_svr_score_dots, dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, n, (const double *)dots, s->b, scores, t, eps, s->part);
      if (hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "%s_csr: the launch failed", who);
    }
    if (!scores) pmh_free(ctx, dots); // (waits for the stream)
    PMH_CHK(rc);
  } else if (n > 0) {
    svm_const<2>(f32, [&](auto F) {
      using T = svm_sample_t<decltype(F)>;
      if (s->d == 64) hipLaunchKernelGGL(k_svr_score64<T>, dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, n, (const T *)X, (const double *)s->w, s->b, scores, t, eps, s->part);
      else hipLaunchKernelGGL(k_svr_score<T>, dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, n, s->d, (const T *)X, (const double *)s->w, s->b, scores, t, eps, s->part);
    });
    PMH_HIP(hipGetLastError());
  }
  if (!m) return PMH_SUCCESS;
  PMH_CHK(svr_sum_part(s, n, nb, SVR_NSUM, 3));
  double h[SVR_NSUM], ng = (double)n;
  PMH_CHK(pmh_memcpy_d2h(ctx, h, s->scal, sizeof(h)));
  PMH_CHK(pmh_comm_sum_host(ctx, &ng, 1));
  m->n = (long long)ng, m->sum_r = h[0], m->sum_r2 = h[1], m->sum_abs_r = h[2], m->max_abs = -h[3] + 0.0, m->sum_t = h[4], m->sum_t2 = h[5], m->n_in_tube = (long long)h[6];
  const double sst = h[5] - h[4] * h[4] / ng;
  m->mse = ng > 0.0 ? h[1] / ng : NAN, m->mae = ng > 0.0 ? h[2] / ng : NAN, m->r2 = (ng > 0.0 && sst > 0.0) ? 1.0 - h[1] / sst : NAN;
  return PMH_SUCCESS;
}

extern "C" int pmh_svr_predict(pmh_svr s, int n, const double *X_dev, double *f_dev) { return svr_score(s, "pmh_svr_predict", n, X_dev, 0, nullptr, f_dev, nullptr, nullptr); }
extern "C" int pmh_svr_predict_f32(pmh_svr s, int n, const float *X_dev, double *f_dev) { return svr_score(s, "pmh_svr_predict", n, X_dev, 1, nullptr, f_dev, nullptr, nullptr); }
extern "C" int pmh_svr_predict_csr(pmh_svr s, pmh_csr Xt, double *f_dev)
{
  PMH_ARG(s && Xt);
  return svr_score(s, "pmh_svr_predict", Xt->nrows, nullptr, 0, Xt, f_dev, nullptr, nullptr);
}
extern "C" int pmh_svr_test(pmh_svr s, int n, const double *X_dev, const double *t_dev, pmh_svr_metrics *m)
{
  PMH_ARG(t_dev && m);
  return svr_score(s, "pmh_svr_test", n, X_dev, 0, nullptr, nullptr, t_dev, m);
}
extern "C" int pmh_svr_test_f32(pmh_svr s, int n, const float *X_dev, const double *t_dev, pmh_svr_metrics *m)
{
  PMH_ARG(t_dev && m);
  return svr_score(s, "pmh_svr_test", n, X_dev, 1, nullptr, nullptr, t_dev, m);
}
extern "C" int pmh_svr_test_csr(pmh_svr s, pmh_csr Xt, const double *t_dev, pmh_svr_metrics *m)
{
  PMH_ARG(s && Xt && t_dev && m);
  return svr_score(s, "pmh_svr_test", Xt->nrows, nullptr, 0, Xt, nullptr, t_dev, m);
}
