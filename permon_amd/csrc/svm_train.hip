// SVM front end (PermonSVM's role: train, model, predict) over the dual operators of svm.hip (dense rows) and svm_csr.hip (samples in CSR):
//   L1: min 1/2 a'Ha - 1'a,          0 <= a <= C   (primal 1/2 |w|^2 + C sum xi)
//   L2: min 1/2 a'(H + I/C)a - 1'a,  0 <= a        (primal 1/2 |w|^2 + C/2 sum xi^2)
//   penalties (pmh_svm_set_penalties): C_i = (y_i > 0 ? C_pos : C_neg) weight_i per sample: L1 the upper bounds, L2 the diagonal 1 / C_i of the operator
//   bias: additionally y'a = 0, posed as (y / sqrt(n))'a = 0 -- a one-row projector (onerow.hip) under SMALXE, whose penalty term the operator absorbs (qppf.hip)
// H = diag(y) X X' diag(y).  No bias: MPGP on the box alone.  Model: w = X'(y o a) by the operator's pass-1 kernels; b by one pass over X (svm_bias_f);
// prediction by one pass over the test samples.  The kernels are the three shells of svm_front.h (k_svm_rows: any d the operator accepts; k_svm_rows64 for
// d = 64: the sweeps of the operator's own pass 2, svm_rows.h; k_svm_dots for samples in CSR: x_i . w by the entry-balanced sweep of svm_csr.hip, then one
// thread per dot product) around a row functor, picked by sv_sweep.  What a row's dot product is used for is the functor: svm_bias_f, svm_classify_f and
// svm_sigmoid_f here; their sums leave every kernel through svm_store.
// Probabilities (pmh_svm_calibrate, pmh_svm_predict_proba): A, B of the Platt fit (svm_proba.hip) on the handle; 1 / (1 + exp(A (x_i . w + b) + B)) is one more
// functor on the same sweeps, so a probability costs the one pass over X that a score costs.
// Dense samples in float32 (pmh_svm_create_f32; test samples: pmh_svm_predict_f32, _test_f32, _predict_proba_f32, _calibrate_f32): the same kernels with the
// sample type as template argument, picked where they are launched; alpha, w, b, the solvers and the model are fp64 either way.
// The training core (solver, statistics, the model's tail, the buffers) is sv_front's, shared with svr_train.hip (svm_front.h); here: labels, subsets, warm
// starts, calibration.
#include "svm_front.h"

struct pmh_svm_s : sv_front { // (u is alpha)
  const double *y = nullptr;
  double        C = 0.0;
  // pmh_svm_set_subset (the mask and n_sub: sv_front): Dm: L2, the operator's diagonal m_i / C_i under a subset (n doubles)
  double       *Dm = nullptr;
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


// sample i with dot = x_i . w in the sums of the bias: s[0] over the free support vectors of y_i - x_i . w, s[1] = y'a, s[2] the number of free support vectors,
// s[3] of support vectors; free: astol < a_i and (ubound > 0: a_i < ubound - astol).  UBV: the upper bound of sample i is ubv[i] (per-sample penalties, L1),
// not the scalar
template <int UBV> struct svm_bias_f {
  const double *__restrict__ y, *__restrict__ alpha, *__restrict__ ubv;
  double        astol, ubound;
  double       *part; // -> part[4][gridDim.x]
  double        s[4] = {0.0, 0.0, 0.0, 0.0};
  __device__ __forceinline__ void row(long long i, double dot)
  {
    const double ub = UBV ? ubv[i] : ubound, ai = alpha[i], yi = y[i];
    s[1] += yi * ai;
    if (ai > astol) {
      s[3] += 1.0;
      if (!(ub > 0.0) || ai < ub - astol) s[2] += 1.0, s[0] += yi - dot;
    }
  }
  __device__ __forceinline__ void done(double *red) { svm_store<4>(s, red, part); }
};

struct svm_counts {
  double tp = 0.0, fp = 0.0, tn = 0.0, fn = 0.0;
};
// sample i with the score s = x_i . w + b: label_i = +-1 (s >= 0: +1) and, with the true labels, the confusion counts.  scores / labels / ytrue may each be
// nullptr; no __restrict__ on scores: the CSR form reads the dot products from the array the scores go to.  The counts go in and out by value: through
// references the choice (pos ? tp : fp) is one between addresses, and the compiler then keeps the counts in memory (40 bytes of scratch per lane, or 8 KiB of LDS)
// The selector of pmh_svm_test_own (svm_sel, svm_front.h): with sel.m given, a sample is counted only where m_i == sel.want
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
// scores, labels and per workgroup the confusion counts -> part[4][gridDim.x]
struct svm_classify_f {
  double        b;
  double       *scores, *labels;
  const double *ytrue;
  svm_sel       sel;
  double       *part;
  svm_counts    c;
  __device__ __forceinline__ void row(long long i, double dot) { c = svm_classify_row(i, dot + b, scores, labels, ytrue, c, sel); }
  __device__ __forceinline__ void done(double *red)
  {
    const double s[4] = {c.tp, c.fp, c.tn, c.fn};
    if (ytrue) svm_store<4>(s, red, part); // (uniform: a kernel argument)
  }
};
// proba[i] = 1 / (1 + exp(A (x_i . w + b) + B)), the dot product summed as the scores sum it (CSR: in place, the dot products lie where the probabilities go)
struct svm_sigmoid_f {
  double  b, A, B;
  double *proba;
  __device__ __forceinline__ void row(long long i, double dot) { proba[i] = svm_sigmoid(A * (dot + b) + B); }
  __device__ __forceinline__ void done(double *) {}
};

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
  sv_free(s);
  if (s->Dm) pmh_free(s->ctx, s->Dm);
  if (s->ws_cnt) pmh_free(s->ctx, s->ws_cnt);
  delete s;
  return PMH_SUCCESS;
}

static long long svm_n_posed(pmh_svm s) { return sv_n_posed(s); }
// the equality's row y / sqrt(n) and its projector; under a subset the masked labels over sqrt(n_S): zero on the held-out rows
static int svm_refresh_row(pmh_svm s) { return sv_refresh_row(s, 1.0 / sqrt((double)svm_n_posed(s))); }
// Dm_i = m_i cinv_i (cinv == nullptr: m_i c)
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_mask_diag(int n, const double *__restrict__ m, const double *__restrict__ cinv, double c, double *__restrict__ Dm)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) Dm[i] = m[i] != 0.0 ? (cinv ? cinv[i] : c) : 0.0;
}
// L2: the operator's term beside H from the handle's state: the shift 1 / C, the diagonal 1 / C_i (penalties) or, under a subset, the diagonal m_i / C_i
static int svm_refresh_l2(pmh_svm s)
{
  if (s->loss_type != PMH_SVM_LOSS_L2) return PMH_SUCCESS;
  if (s->n_sub > 0) {
    if (!s->Dm) PMH_CHK(pmh_malloc(s->ctx, sizeof(double) * (size_t)(s->n ? s->n : 1), (void **)&s->Dm));
    if (s->n > 0) hipLaunchKernelGGL(k_svm_mask_diag, dim3(pmh_vec_grid(s->n)), dim3(PMH_BLOCK), 0, s->ctx->stream, s->n, (const double *)static_cast<SvmDualBase *>(s->H)->msk, (const double *)s->Cinv, 1.0 / s->C, s->Dm);
    PMH_HIP(hipGetLastError());
    PMH_CHK(pmh_op_svm_dual_set_terms(s->H, 0.0, 0.0));
    return pmh_op_svm_dual_set_diag(s->H, s->Dm);
  }
  if (s->Cinv) {
    PMH_CHK(pmh_op_svm_dual_set_terms(s->H, 0.0, 0.0));
    return pmh_op_svm_dual_set_diag(s->H, s->Cinv);
  }
  PMH_CHK(pmh_op_svm_dual_set_diag(s->H, nullptr));
  return pmh_op_svm_dual_set_terms(s->H, 1.0 / s->C, 0.0);
}

// X_dev (dense rows: doubles, or floats where f32) or Xcsr
static int svm_create(pmh_ctx ctx, int n_local, int d, const void *X_dev, int f32, pmh_csr Xcsr, const double *y_dev, const pmh_svm_opts *opts, pmh_svm *out)
{
  if (opts->loss_type != PMH_SVM_LOSS_L1 && opts->loss_type != PMH_SVM_LOSS_L2) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_create: unknown loss type %d (PMH_SVM_LOSS_L1 | PMH_SVM_LOSS_L2)", opts->loss_type);
  if (!(opts->C > 0.0)) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_create: C = %g, must be positive", opts->C);
  pmh_svm s = new pmh_svm_s();
  s->ctx = ctx, s->n = s->nu = n_local, s->d = d, s->X = X_dev, s->f32 = f32, s->Xcsr = Xcsr, s->y = y_dev, s->C = opts->C;
  sv_take_opts(s, *opts);
  memset(&s->st, 0, sizeof(s->st));
  const int    n  = n_local;
  const size_t nb = sizeof(double) * (size_t)(n ? n : 1);
  int          rc = PMH_SUCCESS;
  do {
    if ((rc = Xcsr ? pmh_op_create_svm_dual_csr(ctx, Xcsr, y_dev, &s->H) : (f32 ? pmh_op_create_svm_dual_f32(ctx, n, d, (const float *)X_dev, y_dev, &s->H) : pmh_op_create_svm_dual(ctx, n, d, (const double *)X_dev, y_dev, &s->H)))) break;
    if ((rc = svm_refresh_l2(s))) break;
    if ((rc = sv_alloc_common(s, 4, opts->C)) || (rc = pmh_vec_set(ctx, n, s->rhs, 1.0))) break;
    if ((rc = sv_count_samples(s, "pmh_svm_create"))) break; // (the row of the equality is y / sqrt(n))
    if (opts->bias && ((rc = pmh_malloc(ctx, nb, (void **)&s->row)) || (rc = svm_refresh_row(s)))) break;
    if ((rc = sv_build_solver(s))) break;
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

// w, b and the counts from the current alpha.  The equality's row is y / sqrt(n), over the subset: n_S
static int svm_model(pmh_svm s)
{
  const bool   L1  = s->loss_type == PMH_SVM_LOSS_L1;
  const double *ubv = L1 ? s->Cv : nullptr; // per-sample penalties: free means a_i < C_i - astol
  const double scale = sqrt((double)(svm_n_posed(s) > 0 ? svm_n_posed(s) : 1));
  double       h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  int          rc   = PMH_SUCCESS;
  svm_const<2>(ubv != nullptr, [&](auto U) { rc = sv_model(s, "pmh_svm_train", svm_bias_f<decltype(U)::value>{s->y, s->u, ubv, s->astol(), L1 ? s->C : 0.0, s->part}, scale, &s->st, h); });
  s->st.yTalpha = h[1];
  return rc;
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
    hipLaunchKernelGGL(k_svm_warm_start, dim3(pmh_vec_grid(s->n)), dim3(PMH_BLOCK), 0, ctx->stream, s->n, (const double *)s->u, (const double *)static_cast<SvmDualBase *>(s->H)->msk, (const double *)s->ub, scale, a0, s->ws_cnt);
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
  if (warm) PMH_CHK(svm_warm_start(s, who, alpha_scale, s->u)); // (a refusal changes nothing)
  s->calibrated = 0;
  if (!warm) PMH_CHK(pmh_memset(s->ctx, s->u, 0, nb));
  s->has_dual = 0; // (until the solve has returned: alpha is an iterate meanwhile)
  if (s->sx && warm) {
    // B'mu = mu row with b = mu / sqrt(n_S) (svm_model): the last bias over the CURRENT row m o y / sqrt(n_S), which a new subset has rebuilt -- written into
    // the solver's own B'mu
    double *Btmu = nullptr;
    PMH_CHK(pmh_smalxe_get_penalized(s->sx, nullptr, nullptr, &Btmu));
    PMH_CHK(sv_fill_row(s->ctx, s->n, s->row, s->b_mult * sqrt((double)svm_n_posed(s)), Btmu));
    PMH_HIP(hipGetLastError());
    PMH_CHK(pmh_smalxe_set_initial_multiplier(s->sx, Btmu));
  }
  PMH_CHK(sv_solve(s, &s->st)); // (MPGP's counters are not reset: a solver kept over trainings goes on counting)
  s->has_dual = 1;
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
  return sv_get_model(s, "pmh_svm", w_host, b);
}

extern "C" int pmh_svm_get_dual(pmh_svm s, double *alpha_dev)
{
  PMH_ARG(s && alpha_dev);
  return pmh_vec_copy(s->ctx, s->nu, s->u, alpha_dev);
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
  return sv_get_solver(s, H, pf, mpgp, smalxe);
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
  const bool   L2  = s->loss_type == PMH_SVM_LOSS_L2;
  if (weight_dev) {
    long long nbad = 0; // (every rank decides alike, before anything is changed)
    PMH_CHK(sv_count_bad(ctx, "pmh_svm_set_penalties", "weights", [&](int *cnt) {
      if (n > 0) hipLaunchKernelGGL(k_svm_weights_bad, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, s->y, weight_dev, C_pos, C_neg, cnt);
    }, &nbad));
    if (nbad)
      return pmh_set_error(PMH_ERR_ARG, "pmh_svm_set_penalties: %lld of the sample weights are not positive and finite (or give a penalty C_i that is not); a zero weight does not leave a sample out: pmh_svm_set_subset does", nbad);
  }
  PMH_CHK(sv_alloc_penalties(s));
  s->trained = s->calibrated = 0;
  if (n > 0) {
    hipLaunchKernelGGL(k_svm_fill_penalties, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, s->y, weight_dev, C_pos, C_neg, s->Cv, L2 ? nullptr : s->ub, L2 ? s->Cinv : nullptr);
    PMH_HIP(hipGetLastError());
  }
  PMH_CHK(svm_refresh_l2(s)); // the diagonal 1 / C_i in place of the scalar 1 / C (under a subset m_i / C_i)
  return sv_build_solver(s);
}

extern "C" int pmh_svm_get_penalties(pmh_svm s, double *c_dev)
{
  PMH_ARG(s && c_dev);
  if (s->Cv) return pmh_vec_copy(s->ctx, s->n, s->Cv, c_dev);
  return pmh_vec_set(s->ctx, s->n, c_dev, s->C);
}

// New labels on the created handle: everything svm_create derived from y is redone by the calls svm_create makes (svm_refresh_l2, svm_refresh_row,
// sv_build_solver) after the operator's labels and the penalties, which go back to the scalar C: a training afterwards gives what a fresh handle on (X, y_dev)
// gives, bit for bit
extern "C" int pmh_svm_set_labels(pmh_svm s, const double *y_dev)
{
  PMH_ARG(s && y_dev);
  pmh_ctx   ctx = s->ctx;
  const int n   = s->n;
  s->trained = s->calibrated = 0;
  s->has_dual = 0; // alpha belongs to the old labels: no warm start from it
  sv_drop_solver(s);
  PMH_CHK(pmh_op_svm_dual_set_labels(s->H, y_dev));
  s->y = y_dev;
  if (s->loss_type != PMH_SVM_LOSS_L2) PMH_CHK(pmh_vec_set(ctx, n, s->ub, s->C));
  if (s->Cv) pmh_free(ctx, s->Cv), s->Cv = nullptr;
  if (s->Cinv) pmh_free(ctx, s->Cinv), s->Cinv = nullptr;
  PMH_CHK(svm_refresh_l2(s)); // (a subset stays: the operator rebuilt its masked labels, the diagonal is m_i / C again)
  PMH_CHK(svm_refresh_row(s));
  return sv_build_solver(s);
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
  sv_drop_solver(s);
  PMH_CHK(sv_count_subset(s));
  if (m_dev) PMH_CHK(pmh_vec_copy(ctx, s->n, H->msk, s->rhs));
  else PMH_CHK(pmh_vec_set(ctx, s->n, s->rhs, 1.0));
  PMH_CHK(svm_refresh_l2(s));
  PMH_CHK(svm_refresh_row(s));
  return sv_build_solver(s);
}

extern "C" int pmh_svm_get_subset(pmh_svm s, double *m_dev, long long *n_in)
{
  PMH_ARG(s);
  return sv_get_subset(s, m_dev, n_in);
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
// mp: mapped samples (then X, f32 and Xt are not looked at)
static int svm_predict(pmh_svm s, int n, const void *X, int f32, pmh_csr Xt, double *scores, double *labels, const double *ytrue, long long *counts, bool own = false, svm_sel sel = svm_sel(),
                       const sv_mapped *mp = nullptr)
{
  PMH_ARG(s && n >= 0 && (X || Xt || n == 0 || own || mp));
  if (!s->trained) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_predict: call pmh_svm_train first");
  if (mp) PMH_CHK(sv_check_mapped("pmh_svm_predict", *mp, n, s->d));
  else if (!own) PMH_CHK(pmh_svm_check_test_samples("pmh_svm_predict", s->d, Xt));
  // (CSR: the dot products land where the scores go; without scores in a buffer of the call)
  PMH_CHK(sv_sweep<true>(s->ctx, "pmh_svm_predict", n, s->d, X, f32, Xt, own && s->Xcsr ? static_cast<SvmDualBase *>(s->H) : nullptr, s->w, scores, svm_classify_f{s->b, scores, labels, ytrue, sel, s->part}, mp));
  if (!counts) return PMH_SUCCESS;
  PMH_CHK(pmh_svm_finish_part(s->ctx, n, SVM_NB(n), 4, -1, s->part, s->scal));
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
  svm_sel sel;
  PMH_CHK(sv_own_selector(s, "pmh_svm_test_own", "pmh_svm_set_subset", which, &sel));
  return svm_predict(s, s->n, s->X, s->f32, nullptr, nullptr, nullptr, s->y, counts, true, sel);
}

// ---- probabilities (Platt scaling, svm_proba.hip) ---------------------------------------------------------------------------------------------------------------
// the scores of the calibration samples by the predict path, then the fit on them
static int svm_calibrate(pmh_svm s, int n, const void *X, int f32, pmh_csr Xt, const double *y, const sv_mapped *mp = nullptr)
{
  PMH_ARG(s && n >= 0 && (X || Xt || n == 0 || mp) && (y || n == 0));
  if (!s->trained) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_calibrate: call pmh_svm_train first");
  double *scores = nullptr;
  PMH_CHK(pmh_malloc(s->ctx, sizeof(double) * (size_t)(n ? n : 1), (void **)&scores));
  double              A = 0.0, B = 0.0;
  pmh_svm_platt_stats st;
  int                 rc = svm_predict(s, n, X, f32, Xt, scores, nullptr, nullptr, nullptr, false, svm_sel(), mp);
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
static int svm_predict_proba(pmh_svm s, int n, const void *X, int f32, pmh_csr Xt, double *proba, const sv_mapped *mp = nullptr)
{
  PMH_ARG(s && n >= 0 && (X || Xt || n == 0 || mp) && (proba || n == 0));
  if (!s->trained) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_predict_proba: call pmh_svm_train first");
  if (!s->calibrated) return pmh_set_error(PMH_ERR_STATE, "pmh_svm_predict_proba: call pmh_svm_calibrate or pmh_svm_set_calibration first");
  if (mp) PMH_CHK(sv_check_mapped("pmh_svm_predict_proba", *mp, n, s->d));
  else PMH_CHK(pmh_svm_check_test_samples("pmh_svm_predict", s->d, Xt));
  return sv_sweep<true>(s->ctx, "pmh_svm_predict_proba", n, s->d, X, f32, Xt, nullptr, s->w, proba, svm_sigmoid_f{s->b, s->cal_A, s->cal_B, proba}, mp);
}

extern "C" int pmh_svm_predict_proba(pmh_svm s, int n, const double *X_dev, double *proba_dev) { return svm_predict_proba(s, n, X_dev, 0, nullptr, proba_dev); }
extern "C" int pmh_svm_predict_proba_f32(pmh_svm s, int n, const float *X_dev, double *proba_dev) { return svm_predict_proba(s, n, X_dev, 1, nullptr, proba_dev); }

extern "C" int pmh_svm_predict_proba_csr(pmh_svm s, pmh_csr Xt, double *proba_dev)
{
  PMH_ARG(s && Xt);
  return svm_predict_proba(s, Xt->nrows, nullptr, 0, Xt, proba_dev);
}

// ---- mapped samples (rff_score.hip): the features' dot products with w come ready, as the CSR samples' do, and every functor applies through k_svm_dots ------------
extern "C" int pmh_svm_predict_rff(pmh_svm s, pmh_rff map, int n, const void *X_dev, int x_type, double *scores_dev, double *labels_dev)
{
  const sv_mapped mp{map, X_dev, x_type};
  return svm_predict(s, n, nullptr, 0, nullptr, scores_dev, labels_dev, nullptr, nullptr, false, svm_sel(), &mp);
}
extern "C" int pmh_svm_test_rff(pmh_svm s, pmh_rff map, int n, const void *X_dev, int x_type, const double *y_dev, long long counts[4])
{
  PMH_ARG(y_dev && counts);
  const sv_mapped mp{map, X_dev, x_type};
  return svm_predict(s, n, nullptr, 0, nullptr, nullptr, nullptr, y_dev, counts, false, svm_sel(), &mp);
}
extern "C" int pmh_svm_calibrate_rff(pmh_svm s, pmh_rff map, int n, const void *X_dev, int x_type, const double *y_dev)
{
  const sv_mapped mp{map, X_dev, x_type};
  return svm_calibrate(s, n, nullptr, 0, nullptr, y_dev, &mp);
}
extern "C" int pmh_svm_predict_proba_rff(pmh_svm s, pmh_rff map, int n, const void *X_dev, int x_type, double *proba_dev)
{
  const sv_mapped mp{map, X_dev, x_type};
  return svm_predict_proba(s, n, nullptr, 0, nullptr, proba_dev, &mp);
}
