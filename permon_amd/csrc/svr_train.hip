// SVR front end: linear epsilon-insensitive support vector regression over the dual operators of svr.hip, on the training core of svm_front.h (sv_front: the
// solver, the statistics, the model's tail and the buffers are those of svm_train.hip):
//   dual in u = [p; q]:  min 1/2 u'H^u - c^'u,  c^ = [t - eps; -t - eps],  L1: 0 <= u <= [C_i; C_i] (D = 0),  L2: 0 <= u (D = diag(1 / C_i))
//   bias: additionally sum (p_i - q_i) = 0, posed as ([1; -1] / sqrt(2 n))'u = 0 -- a one-row projector under SMALXE whose penalty term the operator absorbs
// No bias: MPGP on the box alone.  Model: w = X'(p - q) by the operator's pass 1; b by one pass over X (svr_bias_f); prediction and the regression metrics by
// one pass over the test samples (svr_score_f), both on the kernel shells of svm_front.h, picked by sv_sweep: dense rows in fp64 or float32, d == 64, or CSR
// (x_i . w by the entry-balanced row sweep of svm_csr.hip, then one thread per dot product).  Every sum leaves a workgroup through svm_store and is finished by
// one workgroup in a fixed order.  Here: epsilon, the doubled right-hand side, the [1; -1] row, the metrics.
// A sample subset S (pmh_svr_set_subset): the operator's H^_S (svr.hip), c^_S = [m o (t - eps); m o (-t - eps)], the row [m; -m] / sqrt(2 n_S); L2: the operator
// restricts D to S itself (it masks its operand and writes +0 on the held-out rows), L1 keeps its bounds.  From u = 0 every iterate, gradient and direction of the
// solvers is then exactly zero on the held-out rows in both halves, so the trained u, the multiplier, w, b and the counts are those of S alone.
#include "svm_front.h"

struct pmh_svr_s : sv_front { // (nu = 2 n: u = [p; q])
  const double *t = nullptr;
  double        C = 0.0, epsilon = 0.0;
  pmh_svr_stats st;
};

#define SVR_NSUM 7 // the most sums a kernel here leaves per workgroup (svr_score_f); the bias leaves 4

// ---- the bias -------------------------------------------------------------------------------------------------------------------------------------------------
// sample i with dot = x_i . w in s[0]: the sum over the free entries of t_i - eps - D_i p_i - dot (a free p_i) and t_i + eps + D_i q_i - dot (a free q_i), each
// evaluated left to right; s[1]: sum (p_i - q_i); s[2]: free entries; s[3]: entries above astol.  free: astol < u_k and (ub > 0: u_k < ub - astol)
// Under a subset the pass still visits every row, and relies on this: a held-out row has p_i = q_i = 0 after a training (above), so it adds +0 to s[1], is
// counted in neither s[2] nor s[3], and its dot product -- whatever the row of X holds -- reaches no sum
struct svr_bias_f {
  const double *t, *p, *q, *ubv, *dv; // ubv: the upper bound of sample i (per-sample penalties, L1) or nullptr: ub; dv: D_i (L2) or nullptr: dsc
  double        eps, astol, ub, dsc;  // ub <= 0: no upper bound (L2); dsc: the scalar D (L1: 0)
  double       *part;                 // -> part[4][gridDim.x]
  double        s[4] = {0.0, 0.0, 0.0, 0.0};
  __device__ __forceinline__ void row(long long i, double dot)
  {
    const double pi = p[i], qi = q[i], ti = t[i], ubi = ubv ? ubv[i] : ub, D = dv ? dv[i] : dsc;
    s[1] += pi - qi;
    if (pi > astol) {
      s[3] += 1.0;
      if (!(ubi > 0.0) || pi < ubi - astol) s[2] += 1.0, s[0] += ((ti - eps) - D * pi) - dot;
    }
    if (qi > astol) {
      s[3] += 1.0;
      if (!(ubi > 0.0) || qi < ubi - astol) s[2] += 1.0, s[0] += ((ti + eps) + D * qi) - dot;
    }
  }
  __device__ __forceinline__ void done(double *red) { svm_store<4>(s, red, part); }
};

// ---- prediction and the metrics ---------------------------------------------------------------------------------------------------------------------------------
// sample i with the score f = x_i . w + b: f -> scores (where given) and, with targets, r = f - t_i in the seven sums: sum r, sum r^2, sum |r|, -max |r|, sum t,
// sum t^2, the count of |r| <= eps.  No __restrict__ on scores: the CSR form reads the dot products from the array the scores go to
// sel (pmh_svr_test_own): the sums are taken over the selected samples only; every sample is still scored
static __device__ __forceinline__ void svr_score_row(long long i, double f, double *scores, const double *__restrict__ t, double eps, svm_sel sel, double (&s)[SVR_NSUM])
{
  if (scores) scores[i] = f;
  if (t && (!sel.m || sel.m[i] == sel.want)) {
    const double ti = t[i], r = f - ti, ar = fabs(r);
    s[0] += r, s[1] += r * r, s[2] += ar, s[3] = fmin(s[3], -ar), s[4] += ti, s[5] += ti * ti, s[6] += ar <= eps ? 1.0 : 0.0;
  }
}
struct svr_score_f {
  double        b;
  double       *scores;
  const double *t;
  double        eps;
  svm_sel       sel;
  double       *part;                                              // -> part[SVR_NSUM][gridDim.x]
  double        s[SVR_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; // (-max |r| starts at -0: no sample, max 0)
  __device__ __forceinline__ void row(long long i, double dot) { svr_score_row(i, dot + b, scores, t, eps, sel, s); }
  __device__ __forceinline__ void done(double *red)
  {
    if (t) svm_store<SVR_NSUM, 3>(s, red, part); // (uniform: a kernel argument)
  }
};

// ---- the vectors of the QP ------------------------------------------------------------------------------------------------------------------------------------
// rhs = [t - eps; -t - eps]; m given (a subset): +0 in both halves of a held-out sample
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_fill_rhs(int n, const double *__restrict__ t, double eps, const double *__restrict__ m, double *__restrict__ rhs)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    const bool in = !m || m[i] != 0.0;
    rhs[i] = in ? t[i] - eps : 0.0, rhs[n + i] = in ? -t[i] - eps : 0.0;
  }
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
  sv_free(s);
  delete s;
  return PMH_SUCCESS;
}

// L2: the operator's D: the shift 1 / C or the diagonal 1 / C_i
static int svr_refresh_l2(pmh_svr s)
{
  if (s->loss_type != PMH_SVM_LOSS_L2) return PMH_SUCCESS;
  if (s->Cinv) {
    PMH_CHK(pmh_op_svr_dual_set_terms(s->H, 0.0, 0.0));
    return pmh_op_svr_dual_set_diag(s->H, s->Cinv);
  }
  PMH_CHK(pmh_op_svr_dual_set_diag(s->H, nullptr));
  return pmh_op_svr_dual_set_terms(s->H, 1.0 / s->C, 0.0);
}
static int svr_fill_rhs(pmh_svr s)
{
  if (s->n > 0) hipLaunchKernelGGL(k_svr_fill_rhs, dim3(pmh_vec_grid(s->n)), dim3(PMH_BLOCK), 0, s->ctx->stream, s->n, s->t, s->epsilon, (const double *)static_cast<SvmDualBase *>(s->H)->msk, s->rhs);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}
// the equality's row [1; -1] / sqrt(2 n) and its projector; under a subset [m; -m] / sqrt(2 n_S) (the operator's masked labels: sv_refresh_row)
static int svr_refresh_row(pmh_svr s) { return sv_refresh_row(s, 1.0 / sqrt(2.0 * (double)sv_n_posed(s))); }
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
  PMH_CHK(sv_count_bad(ctx, "pmh_svr_create", "values", [&](int *cnt) {
    if (n > 0) hipLaunchKernelGGL(k_svr_targets_bad, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, t_dev, cnt);
  }, &nbad));
  if (nbad) return pmh_set_error(PMH_ERR_ARG, "pmh_svr_create: %lld of the targets are not finite", nbad);
  pmh_svr s = new pmh_svr_s();
  s->ctx = ctx, s->n = n, s->nu = 2 * n, s->d = d, s->X = X_dev, s->f32 = f32, s->Xcsr = Xcsr, s->t = t_dev, s->C = opts->C, s->epsilon = opts->epsilon;
  sv_take_opts(s, *opts);
  memset(&s->st, 0, sizeof(s->st));
  const size_t nb2 = sizeof(double) * 2 * (size_t)(n ? n : 1);
  int          rc  = PMH_SUCCESS;
  do {
    if ((rc = Xcsr ? pmh_op_create_svr_dual_csr(ctx, Xcsr, &s->H) : (f32 ? pmh_op_create_svr_dual_f32(ctx, n, d, (const float *)X_dev, &s->H) : pmh_op_create_svr_dual(ctx, n, d, (const double *)X_dev, &s->H)))) break;
    if ((rc = svr_refresh_l2(s))) break;
    if ((rc = sv_alloc_common(s, SVR_NSUM, opts->C)) || (rc = svr_fill_rhs(s))) break;
    if ((rc = sv_count_samples(s, "pmh_svr_create"))) break; // (the row of the equality is [1; -1] / sqrt(2 n))
    if (opts->bias && ((rc = pmh_malloc(ctx, nb2, (void **)&s->row)) || (rc = svr_refresh_row(s)))) break;
    if ((rc = sv_build_solver(s))) break;
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
  const bool   L2  = s->loss_type == PMH_SVM_LOSS_L2;
  if (weight_dev) {
    long long nbad = 0;
    PMH_CHK(sv_count_bad(ctx, "pmh_svr_set_penalties", "values", [&](int *cnt) {
      if (n > 0) hipLaunchKernelGGL(k_svr_weights_bad, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, weight_dev, C, cnt);
    }, &nbad));
    if (nbad) return pmh_set_error(PMH_ERR_ARG, "pmh_svr_set_penalties: %lld of the sample weights are not positive and finite (or give a penalty C_i that is not); a zero weight does not leave a sample out", nbad);
  }
  PMH_CHK(sv_alloc_penalties(s));
  s->trained = 0;
  if (n > 0) {
    hipLaunchKernelGGL(k_svr_fill_penalties, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, weight_dev, C, s->Cv, L2 ? nullptr : s->ub, L2 ? s->Cinv : nullptr);
    PMH_HIP(hipGetLastError());
  }
  PMH_CHK(svr_refresh_l2(s));
  return sv_build_solver(s);
}

extern "C" int pmh_svr_set_epsilon(pmh_svr s, double epsilon)
{
  PMH_ARG(s);
  PMH_CHK(svr_check_epsilon("pmh_svr_set_epsilon", epsilon));
  s->epsilon = epsilon;
  s->trained = 0;
  PMH_CHK(svr_fill_rhs(s));
  // MPGP takes |c^| for its stopping test at its first solve: asked to take it again.  SMALXE sizes eta by |c^| when it is created: built anew
  if (s->mpgp) return pmh_mpgp_set_tolerances(s->mpgp, s->o_qps.rtol, s->o_qps.atol, s->o_qps.divtol, s->o_qps.max_it);
  return sv_build_solver(s);
}

// w, b and the counts from the current u.  Stationarity in a free p_i reads x_i . w + D_i p_i - (t_i - eps) + mu / sqrt(2 n) = 0: b = mu / sqrt(2 n)
static int svr_model(pmh_svr s)
{
  const bool L1 = s->loss_type == PMH_SVM_LOSS_L1;
  double     h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  svr_bias_f a{s->t, s->u, s->u + s->n, L1 ? s->Cv : nullptr, L1 ? nullptr : s->Cinv, s->epsilon, s->astol(), L1 ? s->C : 0.0, L1 ? 0.0 : 1.0 / s->C, s->part};
  const int  rc = sv_model(s, "pmh_svr_train", a, sqrt(2.0 * (double)(sv_n_posed(s) > 0 ? sv_n_posed(s) : 1)), &s->st, h);
  s->st.sum_beta = h[1];
  return rc;
}

extern "C" int pmh_svr_train(pmh_svr s)
{
  PMH_ARG(s);
  if (!s->sx && !s->mpgp) return pmh_set_error(PMH_ERR_STATE, "pmh_svr_train: the handle has no solver (an earlier pmh_svr_set_penalties / pmh_svr_set_epsilon failed)");
  s->trained = 0;
  PMH_CHK(pmh_memset(s->ctx, s->u, 0, sizeof(double) * (size_t)(s->nu ? s->nu : 1)));
  if (s->mpgp) PMH_CHK(pmh_mpgp_reset_statistics(s->mpgp)); // (the solver may be kept over trainings: the counters are this solve's)
  PMH_CHK(sv_solve(s, &s->st));
  PMH_CHK(svr_model(s));
  s->trained = 1;
  return PMH_SUCCESS;
}

extern "C" int pmh_svr_get_model(pmh_svr s, double *w_host, double *b)
{
  PMH_ARG(s);
  return sv_get_model(s, "pmh_svr", w_host, b);
}

extern "C" int pmh_svr_get_dual(pmh_svr s, double *u_dev)
{
  PMH_ARG(s && u_dev);
  return pmh_vec_copy(s->ctx, s->nu, s->u, u_dev);
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
  return sv_get_solver(s, H, pf, mpgp, smalxe);
}

// own: the handle's own samples (X or, CSR, the operator's tables: Xt == nullptr); sel: which of them the sums are taken over, n_sel of this rank
// mp: mapped samples (then X, f32 and Xt are not looked at)
static int svr_score(pmh_svr s, const char *who, int n, const void *X, int f32, pmh_csr Xt, double *scores, const double *t, pmh_svr_metrics *m, bool own = false, svm_sel sel = svm_sel(), long long n_sel = -1,
                     const sv_mapped *mp = nullptr)
{
  PMH_ARG(s && n >= 0 && (X || Xt || n == 0 || own || mp));
  if (!s->trained) return pmh_set_error(PMH_ERR_STATE, "%s: call pmh_svr_train first", who);
  if (mp) PMH_CHK(sv_check_mapped(who, *mp, n, s->d));
  else if (!own) PMH_CHK(pmh_svm_check_test_samples(who, s->d, Xt));
  pmh_ctx ctx = s->ctx;
  // (CSR: the dot products land where the scores go; without scores in a buffer of the call)
  PMH_CHK(sv_sweep<true>(ctx, who, n, s->d, X, f32, Xt, own && s->Xcsr ? static_cast<SvmDualBase *>(s->H) : nullptr, s->w, scores, svr_score_f{s->b, scores, t, s->epsilon, sel, s->part}, mp));
  if (!m) return PMH_SUCCESS;
  PMH_CHK(pmh_svm_finish_part(ctx, n, SVM_NB(n), SVR_NSUM, 3, s->part, s->scal));
  double h[SVR_NSUM], ng = (double)(n_sel >= 0 ? n_sel : n);
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
// mapped samples (rff_score.hip): the features' dot products with w come ready, as the CSR samples' do
extern "C" int pmh_svr_predict_rff(pmh_svr s, pmh_rff map, int n, const void *X_dev, int x_type, double *f_dev)
{
  const sv_mapped mp{map, X_dev, x_type};
  return svr_score(s, "pmh_svr_predict", n, nullptr, 0, nullptr, f_dev, nullptr, nullptr, false, svm_sel(), -1, &mp);
}
extern "C" int pmh_svr_test_rff(pmh_svr s, pmh_rff map, int n, const void *X_dev, int x_type, const double *t_dev, pmh_svr_metrics *m)
{
  PMH_ARG(t_dev && m);
  const sv_mapped mp{map, X_dev, x_type};
  return svr_score(s, "pmh_svr_test", n, nullptr, 0, nullptr, nullptr, t_dev, m, false, svm_sel(), -1, &mp);
}

// ---- sample subsets, the handle's own rows ------------------------------------------------------------------------------------------------------------------------
// Train on the subset S of the handle's samples, X staying where it is (the header of this file).  The solver is built anew as by pmh_svr_set_penalties: the
// eigenvalue estimate must be H^_S's.  A refused mask leaves the handle exactly as it was: the operator checks it before anything changes
extern "C" int pmh_svr_set_subset(pmh_svr s, const double *m_dev)
{
  PMH_ARG(s);
  PMH_CHK(pmh_op_svr_dual_set_subset(s->H, m_dev));
  s->trained = 0;
  sv_drop_solver(s);
  PMH_CHK(sv_count_subset(s));
  PMH_CHK(svr_fill_rhs(s));
  PMH_CHK(svr_refresh_row(s));
  return sv_build_solver(s);
}

extern "C" int pmh_svr_get_subset(pmh_svr s, double *m_dev, long long *n_in)
{
  PMH_ARG(s);
  return sv_get_subset(s, m_dev, n_in);
}

// the handle's own samples, nothing uploaded: the predict sweep over the X the handle was created on (CSR: the row sweep with the operator's tables)
extern "C" int pmh_svr_predict_own(pmh_svr s, double *f_dev)
{
  PMH_ARG(s && f_dev);
  return svr_score(s, "pmh_svr_predict_own", s->n, s->X, s->f32, nullptr, f_dev, nullptr, nullptr, true);
}

extern "C" int pmh_svr_test_own(pmh_svr s, int which, pmh_svr_metrics *m)
{
  PMH_ARG(s && m);
  svm_sel sel;
  PMH_CHK(sv_own_selector(s, "pmh_svr_test_own", "pmh_svr_set_subset", which, &sel));
  const long long in = static_cast<SvmDualBase *>(s->H)->n_sub; // (of this rank; read only where a mask is set)
  return svr_score(s, "pmh_svr_test_own", s->n, s->X, s->f32, nullptr, nullptr, s->t, m, true, sel, !sel.m ? s->n : (sel.want != 0.0 ? in : s->n - in));
}
