// SVM probabilities by Platt scaling: P(y = +1 | x) = 1 / (1 + exp(A s(x) + B)) with A, B fitted to the scores s_i and labels of a calibration set by the
// regularised maximum-likelihood Newton iteration of
//   H.-T. Lin, C.-J. Lin, R. C. Weng: A note on Platt's probabilistic outputs for support vector machines.  Machine Learning 68 (2007) 267-276
// (LIBSVM's sigmoid_train).  With z_i = A f_i + B, p_i = 1 / (1 + e^{z_i}) and the targets t_i (t_+ for the positive class, t_- for the other):
//   F = sum_i F_i,  F_i = t_i z_i + log(1 + e^{-z_i}),   dF/dA = g1 = sum f_i (t_i - p_i),   dF/dB = g2 = sum (t_i - p_i),
//   h11 = sum f_i^2 p_i (1 - p_i),  h22 = sum p_i (1 - p_i),  h21 = sum f_i p_i (1 - p_i).
// k_svm_platt_sums forms all six in one pass over the scores for one point (A, B): the point a line search accepts then has its gradient and Hessian already.
// The order of every sum is fixed: per-thread sums over i = tid, tid + grid, .., pmh_block_reduce one sum after the other -> part[6][grid] (svm_store), then
// k_svm_finish (svm_front.hip) over the workgroups; the grid is a function of n alone.  No float atomics: two fits give the same bits.  Six doubles cross to
// the host per evaluated point, where the Newton step and the backtracking run.  The kernels that apply the model (svm_train.hip, svm_multi.hip) take the
// sigmoid in the same two branches (svm_sigmoid, svm_rows.h).
#include <cmath>

#include "svm_front.h"

// The constants of Lin, Lin and Weng's algorithm (their Appendix 3 / sigmoid_train): not tunables
static const int    PLATT_MAX_IT   = 100;   // Newton iterations at most
static const double PLATT_MIN_STEP = 1e-10; // the line search gives up below this step
static const double PLATT_SIGMA    = 1e-12; // added to h11 and h22: the Hessian stays positive definite
static const double PLATT_EPS      = 1e-5;  // stop when |g1| and |g2| are below
static const double PLATT_ARMIJO   = 1e-4;  // sufficient decrease: F_new < F + PLATT_ARMIJO step (g . d)

// One pass over the scores f_i = scores[i stride] for the point (A, B): F, g1, g2, h11, h22, h21 -> part[6][gridDim.x].  The target of sample i is tpos where
// y[i] == pos, else tneg.  The objective and the sigmoid in the two-branch form that cannot overflow
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_platt_sums(int n, const double *__restrict__ scores, int stride, const double *__restrict__ y, double pos, double tpos, double tneg, double A, double B,
                                                              double *__restrict__ part)
{
  __shared__ double red[PMH_BLOCK / 64];
  double            s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    const double f = scores[(size_t)i * stride], t = y[i] == pos ? tpos : tneg, z = A * f + B;
    double       p, Fi;
    if (z >= 0.0) {
      const double e = exp(-z);
      p = e / (1.0 + e), Fi = t * z + log1p(e);
    } else {
      const double e = exp(z);
      p = 1.0 / (1.0 + e), Fi = (t - 1.0) * z + log1p(e);
    }
    const double q = p * (1.0 - p), r = t - p;
    s[0] += Fi, s[1] += f * r, s[2] += r, s[3] += f * f * q, s[4] += q, s[5] += f * q;
  }
  svm_store<6>(s, red, part);
}

// the class counts: y[i] == pos, the rest, and (binary) the labels that are neither pos nor -pos, which count in neither class -> part[3][gridDim.x]
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_platt_count(int n, const double *__restrict__ y, double pos, int binary, double *__restrict__ part)
{
  __shared__ double red[PMH_BLOCK / 64];
  double            c[3] = {0.0, 0.0, 0.0}; // y[i] == pos, the rest, neither
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    const double yi = y[i];
    if (yi == pos) c[0] += 1.0;
    else if (!binary || yi == -pos) c[1] += 1.0;
    else c[2] += 1.0;
  }
  svm_store<3>(c, red, part);
}

namespace {
struct platt_fit {
  pmh_ctx       ctx;
  int           n, stride, nb;
  const double *scores, *y;
  double        pos, tpos = 0.0, tneg = 0.0;
  double       *part = nullptr, *scal = nullptr; // part[6][nb], the six sums on the device
  int           evaluations = 0;
  // h[0..5] = the sums over all workgroups and ranks
  int           finish(int K, double *h)
  {
    PMH_CHK(pmh_svm_finish_part(ctx, n, nb, K, -1, part, scal));
    return pmh_memcpy_d2h(ctx, h, scal, sizeof(double) * (size_t)K);
  }
  int count(int binary, double *h)
  {
    if (n > 0) hipLaunchKernelGGL(k_svm_platt_count, dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, n, y, pos, binary, part);
    return finish(3, h);
  }
  int eval(double A, double B, double *h)
  {
    evaluations++;
    if (n > 0) hipLaunchKernelGGL(k_svm_platt_sums, dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, n, scores, stride, y, pos, tpos, tneg, A, B, part);
    return finish(6, h);
  }
};
} // namespace

static int platt_run(platt_fit &f, int binary, double *A_out, double *B_out, pmh_svm_platt_stats *st)
{
  double c[3];
  PMH_CHK(f.count(binary, c));
  if (c[0] + c[1] + c[2] < 1.0) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_platt_fit: no scores (n = 0)");
  if (c[2] != 0.0) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_platt_fit: %lld of the %lld labels are not +-1", (long long)c[2], (long long)(c[0] + c[1] + c[2]));
  const double n_pos = c[0], n_neg = c[1];
  f.tpos = (n_pos + 1.0) / (n_pos + 2.0), f.tneg = 1.0 / (n_neg + 2.0);
  double A = 0.0, B = log((n_neg + 1.0) / (n_pos + 1.0));
  double h[6], hn[6]; // F, g1, g2, h11, h22, h21
  PMH_CHK(f.eval(A, B, h));
  int it = 0, reason = PMH_PLATT_MAX_IT;
  for (; it < PLATT_MAX_IT; it++) {
    const double g1 = h[1], g2 = h[2], h11 = h[3] + PLATT_SIGMA, h22 = h[4] + PLATT_SIGMA, h21 = h[5];
    if (fabs(g1) < PLATT_EPS && fabs(g2) < PLATT_EPS) {
      reason = PMH_PLATT_CONVERGED;
      break;
    }
    // the Newton direction of the 2 x 2 system
    const double det = h11 * h22 - h21 * h21, dA = -(h22 * g1 - h21 * g2) / det, dB = -(-h21 * g1 + h11 * g2) / det, gd = g1 * dA + g2 * dB;
    double       step = 1.0;
    while (step >= PLATT_MIN_STEP) {
      const double An = A + step * dA, Bn = B + step * dB;
      PMH_CHK(f.eval(An, Bn, hn));
      if (hn[0] < h[0] + PLATT_ARMIJO * step * gd) { // (false for a point that is not finite: it is never accepted)
        A = An, B = Bn;
        for (int k = 0; k < 6; k++) h[k] = hn[k];
        break;
      }
      step /= 2.0;
    }
    if (step < PLATT_MIN_STEP) {
      reason = PMH_PLATT_LINE_SEARCH;
      break;
    }
  }
  *A_out = A, *B_out = B;
  if (st) {
    st->reason = reason, st->iterations = it, st->evaluations = f.evaluations;
    st->n_pos = (long long)n_pos, st->n_neg = (long long)n_neg;
    st->fval = h[0], st->g1 = h[1], st->g2 = h[2];
  }
  return PMH_SUCCESS;
}

int pmh_svm_platt_fit_strided(pmh_ctx ctx, int n, const double *scores, int stride, const double *y, double pos, int binary, double *A, double *B, pmh_svm_platt_stats *st)
{
  PMH_ARG(ctx && A && B && stride >= 1);
  if (n < 0 || (n < 1 && !pmh_comm_on(ctx))) return pmh_set_error(PMH_ERR_ARG, "pmh_svm_platt_fit: n = %d scores, at least one is needed", n);
  PMH_ARG(n == 0 || (scores && y));
  platt_fit f;
  f.ctx = ctx, f.n = n, f.stride = stride, f.nb = pmh_vec_grid(n), f.scores = scores, f.y = y, f.pos = pos;
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (6 * (size_t)f.nb + 8), (void **)&f.part));
  f.scal = f.part + 6 * (size_t)f.nb;
  int rc = platt_run(f, binary, A, B, st);
  if (!rc && hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "pmh_svm_platt_fit: a launch failed");
  pmh_free(ctx, f.part);
  return rc;
}

extern "C" int pmh_svm_platt_fit(pmh_ctx ctx, int n, const double *scores_dev, const double *y_dev, double *A, double *B, pmh_svm_platt_stats *st)
{
  return pmh_svm_platt_fit_strided(ctx, n, scores_dev, 1, y_dev, 1.0, 1, A, B, st);
}
