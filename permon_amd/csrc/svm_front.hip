// The training core of the SVM and SVR front ends and the finishing kernel of their sums (svm_front.h).
#include <cstring>
#include <type_traits>

#include "svm_front.h"

// the two statistics structs are one layout: sv_solve and sv_model_tail fill either
static_assert(sizeof(pmh_svm_stats) == sizeof(pmh_svr_stats) && offsetof(pmh_svm_stats, yTalpha) == offsetof(pmh_svr_stats, sum_beta) && offsetof(pmh_svm_stats, b) == offsetof(pmh_svr_stats, b) &&
                offsetof(pmh_svm_stats, rnorm) == offsetof(pmh_svr_stats, rnorm) && offsetof(pmh_svm_stats, passes_X) == offsetof(pmh_svr_stats, passes_X),
              "pmh_svm_stats and pmh_svr_stats differ in more than the name of yTalpha / sum_beta");

// out[k] = sum (k == minrow: min) over b of part[k][b]: one workgroup, fixed order
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_finish(int nb, int K, int minrow, const double *__restrict__ part, double *__restrict__ out)
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

int pmh_svm_sum_rows(pmh_ctx ctx, int nb, int K, const double *part, double *out, int minrow)
{
  hipLaunchKernelGGL(k_svm_finish, dim3(1), dim3(PMH_BLOCK), 0, ctx->stream, nb, K, minrow, part, out);
  PMH_HIP(hipGetLastError()); // (also the launch of the kernel that filled part)
  return PMH_SUCCESS;
}

int pmh_svm_finish_part(pmh_ctx ctx, int n, int nb, int K, int minrow, const double *part, double *scal)
{
  if (n > 0) PMH_CHK(pmh_svm_sum_rows(ctx, nb, K, part, scal, minrow));
  else PMH_CHK(pmh_memset(ctx, scal, 0, sizeof(double) * (size_t)K));
  if (!pmh_comm_on(ctx)) return PMH_SUCCESS;
  if (minrow < 0) return pmh_comm_allreduce_sum(ctx, scal, (size_t)K);
  std::vector<int> ops((size_t)K, PMH_RED_SUM);
  ops[(size_t)minrow] = PMH_RED_MIN;
  return pmh_comm_allreduce_scalars(ctx, scal, K, ops.data());
}

void sv_drop_solver(sv_front *f)
{
  if (f->mpgp) pmh_mpgp_destroy(f->mpgp), f->mpgp = nullptr;
  if (f->sx) pmh_smalxe_destroy(f->sx), f->sx = nullptr;
}

int sv_build_solver(sv_front *f)
{
  sv_drop_solver(f);
  const pmh_qps_opts &q = f->o_qps;
  if (f->bias) {
    pmh_smalxe_opts so = f->o_smalxe;
    so.rtol = q.rtol, so.atol = q.atol, so.divtol = q.divtol;
    if (q.max_it_set) so.max_it = q.max_it;
    return pmh_smalxe_create(f->ctx, f->H, f->rhs, f->u, f->lb, f->ub, f->pf, &so, &f->sx);
  }
  pmh_mpgp_opts mo = f->o_mpgp;
  mo.rtol = q.rtol, mo.atol = q.atol, mo.divtol = q.divtol, mo.max_it = q.max_it;
  return pmh_mpgp_create(f->ctx, f->H, f->rhs, f->u, f->lb, f->ub, &mo, &f->mpgp);
}

template <class ST> int sv_solve(sv_front *f, ST *s)
{
  SvmDualBase    *H  = static_cast<SvmDualBase *>(f->H);
  const long long p0 = H->npass;
  if (f->sx) {
    PMH_CHK(pmh_smalxe_reset(f->sx));
    PMH_CHK(pmh_smalxe_solve(f->sx));
    pmh_smalxe_stats st;
    PMH_CHK(pmh_smalxe_get_stats(f->sx, &st));
    s->reason = st.reason, s->outer_iterations = st.iteration, s->inner_iterations = st.inner_iter_accu;
    s->nmv = st.inner.nmv, s->ncg = st.inner.ncg, s->nexp = st.inner.nexp, s->nprop = st.inner.nprop;
    s->rho = st.rho, s->normBu = st.normBu, s->rnorm = st.rnorm;
  } else {
    PMH_CHK(pmh_mpgp_solve(f->mpgp));
    pmh_mpgp_stats st;
    PMH_CHK(pmh_mpgp_get_stats(f->mpgp, &st));
    s->reason = st.reason, s->outer_iterations = 0, s->inner_iterations = st.iteration;
    s->nmv = st.nmv, s->ncg = st.ncg, s->nexp = st.nexp, s->nprop = st.nprop;
    s->rho = 0.0, s->normBu = 0.0, s->rnorm = st.rnorm;
  }
  s->passes_X = H->npass - p0; // the solve's passes over X (the model's two are not counted)
  return PMH_SUCCESS;
}
template int sv_solve(sv_front *, pmh_svm_stats *);
template int sv_solve(sv_front *, pmh_svr_stats *);

// The equality's multiplier: SMALXE keeps B'mu = mu row (the Lagrangian is 1/2 u'Hu - c'u + mu (row'u)), so mu = row'(B'mu) / (row'row); with the row the labels
// over row_scale, stationarity in a free entry reads (its residual) = mu / row_scale: b = mu / row_scale
template <class ST> int sv_model_tail(sv_front *f, double row_scale, ST *st, double (&h)[5])
{
  if (f->sx) {
    double *Btmu = nullptr;
    PMH_CHK(pmh_smalxe_get_penalized(f->sx, nullptr, nullptr, &Btmu));
    PMH_CHK(pmh_onerow_dot(f->pf, Btmu, 1.0 / f->pf->row_aat, f->scal + 4));
  } else PMH_CHK(pmh_memset(f->ctx, f->scal + 4, 0, sizeof(double)));
  PMH_CHK(pmh_memcpy_d2h(f->ctx, h, f->scal, sizeof(h)));
  f->h_w.resize((size_t)f->d);
  PMH_CHK(pmh_memcpy_d2h(f->ctx, f->h_w.data(), f->w, sizeof(double) * (size_t)f->d));
  st->n_free_sv = (long long)h[2], st->n_sv = (long long)h[3];
  st->b_multiplier = h[4] / row_scale;
  st->b_free       = h[2] > 0.0 ? h[0] / h[2] : NAN;
  if (!f->bias) f->b = 0.0;
  else f->b = h[2] > 0.0 ? st->b_free : st->b_multiplier;
  st->b = f->b;
  return PMH_SUCCESS;
}
template int sv_model_tail(sv_front *, double, pmh_svm_stats *, double (&)[5]);
template int sv_model_tail(sv_front *, double, pmh_svr_stats *, double (&)[5]);

int sv_alloc_common(sv_front *f, int part_rows, double C)
{
  pmh_ctx      ctx = f->ctx;
  const size_t nb  = sizeof(double) * (size_t)(f->nu ? f->nu : 1);
  PMH_CHK(pmh_malloc(ctx, nb, (void **)&f->u));
  PMH_CHK(pmh_malloc(ctx, nb, (void **)&f->rhs));
  PMH_CHK(pmh_malloc(ctx, nb, (void **)&f->lb));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)f->d, (void **)&f->w));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)part_rows * PMH_MAX_VEC_BLOCKS, (void **)&f->part));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * 8, (void **)&f->scal));
  PMH_CHK(pmh_memset(ctx, f->u, 0, nb));
  PMH_CHK(pmh_memset(ctx, f->lb, 0, nb));
  if (f->loss_type != PMH_SVM_LOSS_L1) return PMH_SUCCESS;
  PMH_CHK(pmh_malloc(ctx, nb, (void **)&f->ub));
  return pmh_vec_set(ctx, f->nu, f->ub, C);
}

int sv_count_samples(sv_front *f, const char *who)
{
  double ng = (double)f->n;
  PMH_CHK(pmh_comm_sum_host(f->ctx, &ng, 1));
  f->n_global = (long long)ng;
  if (f->bias && f->n_global < 1) return pmh_set_error(PMH_ERR_ARG, "%s: no samples", who);
  return PMH_SUCCESS;
}

int sv_count_subset(sv_front *f)
{
  SvmDualBase *H = static_cast<SvmDualBase *>(f->H);
  double       ns = H->msk ? (double)H->n_sub : 0.0;
  PMH_CHK(pmh_comm_sum_host(f->ctx, &ns, 1));
  f->n_sub = (long long)ns;
  return PMH_SUCCESS;
}

__global__ __launch_bounds__(PMH_BLOCK) void k_svm_fill_row(int n, const double *__restrict__ y, double c, double *__restrict__ row)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) row[i] = c * y[i];
}
int sv_fill_row(pmh_ctx ctx, int n, const double *y, double c, double *row)
{
  if (n > 0) hipLaunchKernelGGL(k_svm_fill_row, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, y, c, row);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}
int sv_refresh_row(sv_front *f, double c)
{
  if (!f->bias) return PMH_SUCCESS;
  if (f->pf) pmh_qppf_destroy(f->pf), f->pf = nullptr;
  PMH_CHK(sv_fill_row(f->ctx, f->nu, static_cast<SvmDualBase *>(f->H)->yk(), c, f->row));
  return pmh_qppf_create_onerow(f->ctx, f->row, f->nu, &f->pf);
}

int sv_get_subset(sv_front *f, double *m_dev, long long *n_in)
{
  SvmDualBase *H = static_cast<SvmDualBase *>(f->H);
  if (n_in) *n_in = sv_n_posed(f);
  if (!m_dev) return PMH_SUCCESS;
  return H->msk ? pmh_vec_copy(f->ctx, f->n, H->msk, m_dev) : pmh_vec_set(f->ctx, f->n, m_dev, 1.0);
}

int sv_own_selector(sv_front *f, const char *who, const char *set_subset, int which, svm_sel *sel)
{
  if (which != PMH_SVM_OWN_HELD_OUT && which != PMH_SVM_OWN_SUBSET && which != PMH_SVM_OWN_ALL) return pmh_set_error(PMH_ERR_ARG, "%s: which = %d (PMH_SVM_OWN_HELD_OUT | PMH_SVM_OWN_SUBSET | PMH_SVM_OWN_ALL)", who, which);
  SvmDualBase *H = static_cast<SvmDualBase *>(f->H);
  if (which == PMH_SVM_OWN_HELD_OUT && !H->msk) return pmh_set_error(PMH_ERR_STATE, "%s: no subset is set (%s), so no sample is held out", who, set_subset);
  *sel = svm_sel();
  if (which != PMH_SVM_OWN_ALL && H->msk) sel->m = H->msk, sel->want = which == PMH_SVM_OWN_SUBSET ? 1.0 : 0.0;
  return PMH_SUCCESS;
}

int sv_alloc_penalties(sv_front *f)
{
  const size_t nb = sizeof(double) * (size_t)(f->n ? f->n : 1);
  if (!f->Cv) PMH_CHK(pmh_malloc(f->ctx, nb, (void **)&f->Cv));
  if (f->loss_type == PMH_SVM_LOSS_L2 && !f->Cinv) PMH_CHK(pmh_malloc(f->ctx, nb, (void **)&f->Cinv));
  return PMH_SUCCESS;
}

void sv_free(sv_front *f)
{
  sv_drop_solver(f);
  if (f->pf) pmh_qppf_destroy(f->pf);
  if (f->H) pmh_op_destroy(f->H);
  double *v[] = {f->u, f->rhs, f->lb, f->ub, f->row, f->w, f->part, f->scal, f->dots, f->Cv, f->Cinv};
  for (double *p : v)
    if (p) pmh_free(f->ctx, p);
}

int sv_get_model(sv_front *f, const char *pre, double *w_host, double *b)
{
  if (!f->trained) return pmh_set_error(PMH_ERR_STATE, "%s_get_model: call %s_train first", pre, pre);
  if (w_host) memcpy(w_host, f->h_w.data(), sizeof(double) * (size_t)f->d);
  if (b) *b = f->b;
  return PMH_SUCCESS;
}

int sv_get_solver(sv_front *f, pmh_op *H, pmh_qppf *pf, pmh_mpgp *mpgp, pmh_smalxe *smalxe)
{
  if (H) *H = f->H;
  if (pf) *pf = f->pf;
  if (mpgp) *mpgp = f->mpgp;
  if (smalxe) *smalxe = f->sx;
  return PMH_SUCCESS;
}
