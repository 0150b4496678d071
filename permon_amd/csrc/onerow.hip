// One-row equality constraint as a projector (the reference's MATONEROW role, src/mat/impls/onerow/onerow.c: MatMult = one dot product, MatMultTranspose = one
// scaled copy): G = a' with a a dense device vector.  No CSR, no host factorisation: G G' = a'a is one reduction at creation.
//   G v = a'v,  G's = s a,  Q v = a (a'v) / (a'a),  P = I - Q,  (G G')^{-1} = 1 / (a'a).
// Every apply is one dot product (a and v read once; per-workgroup partial sums finished in a fixed order by one workgroup: reproducible run to run) and / or one
// scaled copy (a read, the result written): algorithmic bytes 16 n (G v), 16 n (G's), 24 n (Q v, P v with the second read of a counted once; 32 n of traffic
// where a does not stay in the last-level cache between the two launches).  Under a communicator the dot is joined by pmh_comm_allreduce_sum (one scalar).
#include "pmh_internal.h"
#include "reduce.h"

// per-workgroup partial sums of a'v: grid-stride, one entry per thread per trip, block tree of reduce.h
__global__ __launch_bounds__(PMH_BLOCK) void k_onerow_dot(int n, const double *__restrict__ a, const double *__restrict__ v, double *__restrict__ part)
{
  __shared__ double red[PMH_BLOCK / 64];
  double            s = 0.0;
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) s += __builtin_nontemporal_load(&a[i]) * __builtin_nontemporal_load(&v[i]);
  s = pmh_block_reduce<PMH_RED_SUM>(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// out[0] = coef * sum_b part[b]: one workgroup, thread t takes b = t, t + 256, ..., then the block tree
__global__ __launch_bounds__(PMH_BLOCK) void k_onerow_finish(int nb, const double *__restrict__ part, double coef, double *__restrict__ out)
{
  __shared__ double red[PMH_BLOCK / 64];
  double            s = 0.0;
  for (int b = threadIdx.x; b < nb; b += PMH_BLOCK) s += part[b];
  s = pmh_block_reduce<PMH_RED_SUM>(s, red);
  if (threadIdx.x == 0) out[0] = coef * s;
}
// y = (coef s) a   or   y = v - (coef s) a
__global__ __launch_bounds__(PMH_BLOCK) void k_onerow_scaled_row(int n, const double *__restrict__ a, const double *__restrict__ s, double coef, const double *__restrict__ v, double *__restrict__ y)
{
  const double t = coef * s[0];
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    const double q = t * __builtin_nontemporal_load(&a[i]);
    y[i]           = v ? v[i] - q : q;
  }
}

int pmh_onerow_dot(pmh_qppf pf, const double *v, double coef, double *out)
{
  pmh_ctx   ctx = pf->ctx;
  const int nb  = pf->n > 0 ? pmh_vec_grid(pf->n) : 0;
  // (several ranks: the local sums are joined first, the coefficient applied after -- every rank then holds the same bits)
  const bool dist = pmh_comm_on(ctx);
  if (nb) hipLaunchKernelGGL(k_onerow_dot, dim3(nb), dim3(PMH_BLOCK), 0, ctx->stream, pf->n, pf->row, v, pf->or_part);
  hipLaunchKernelGGL(k_onerow_finish, dim3(1), dim3(PMH_BLOCK), 0, ctx->stream, nb, (const double *)pf->or_part, dist ? 1.0 : coef, out);
  PMH_HIP(hipGetLastError());
  if (dist) {
    PMH_CHK(pmh_comm_allreduce_sum(ctx, out, 1));
    if (coef != 1.0) PMH_CHK(pmh_vec_scale(ctx, 1, out, coef));
  }
  return PMH_SUCCESS;
}

int pmh_onerow_scaled_row(pmh_qppf pf, const double *s, double coef, const double *v, double *y)
{
  if (pf->n <= 0) return PMH_SUCCESS;
  hipLaunchKernelGGL(k_onerow_scaled_row, dim3(pmh_vec_grid(pf->n)), dim3(PMH_BLOCK), 0, pf->ctx->stream, pf->n, pf->row, s, coef, v, y);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

// a_dev: n_local doubles on the device, borrowed (the caller keeps it alive and unchanged).  The rows count as orthonormal (Q = G'G, as pmh_qppf_create's
// orthonormal = 1) when |a'a - 1| <= n eps, the forward bound of the n-term sum for a row normalised in floating point; otherwise Q divides by a'a
extern "C" int pmh_qppf_create_onerow(pmh_ctx ctx, const double *a_dev, int n, pmh_qppf *out)
{
  PMH_ARG(ctx && out && n >= 0 && (a_dev || n == 0));
  pmh_qppf pf       = new pmh_qppf_s();
  pf->ctx           = ctx;
  pf->G             = nullptr;
  pf->m             = 1;
  pf->n             = n;
  pf->orthonormal   = 0;
  pf->implicit_orth = 0;
  pf->d_inv = pf->d_Tt = pf->d_S = pf->tmp_m = nullptr;
  pf->ggt_mfma_ms = pf->host_inverse_ms = 0.0;
  pf->onerow = 1, pf->row = a_dev;
  PMH_CHK(pmh_malloc(ctx, sizeof(double), (void **)&pf->G_left));
  PMH_CHK(pmh_malloc(ctx, sizeof(double), (void **)&pf->Gt_right));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * PMH_MAX_VEC_BLOCKS, (void **)&pf->or_part));
  PMH_CHK(pmh_malloc(ctx, sizeof(double), (void **)&pf->or_s));
  PMH_CHK(pmh_onerow_dot(pf, a_dev, 1.0, pf->or_s));
  PMH_CHK(pmh_memcpy_d2h(ctx, &pf->row_aat, pf->or_s, sizeof(double)));
  if (!(pf->row_aat > 0.0) || std::isinf(pf->row_aat)) {
    const double aat = pf->row_aat;
    pmh_qppf_destroy(pf);
    return pmh_set_error(PMH_ERR_ARG, "pmh_qppf_create_onerow: a'a = %g, the row must be non-zero and finite (G must have full row rank)", aat);
  }
  // (the global length decides the bound; a rank knows its own: the local one is the smaller, hence the stricter)
  pf->orthonormal = fabs(pf->row_aat - 1.0) <= (double)(n > 0 ? n : 1) * 2.220446049250313e-16 ? 1 : 0;
  *out = pf;
  return PMH_SUCCESS;
}
