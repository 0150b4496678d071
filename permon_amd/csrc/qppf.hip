// QPPF projector factory on gfx950: Q = G'(GG')^{-1}G, P = I - Q (src/qppf/interface/qppf.c) and the two
// shell operators of the QP transform chain built on it: A + rho*G'G (src/qp/utils/matpenalized.c) and
// P*A*P / P*A (QPTEnforceEqByProjector, src/qp/interface/qptransform.c:215-316).
//
// G (m x n, m = 6 * #subdomains rigid-body rows, each dense over one subdomain's interface) is an explicit
// CSR in HBM; G v uses the long-row path of the SpMV (one workgroup per row), G' w the short-row stream
// path on the transposed CSR.  The coarse problem (GG')^{-1} is small and dense: GG' is assembled and
// inverted on the host once (the reference's QPPFSetUpGGt_Private / -qppf_explicit_inv path, qppf.c:213-333)
// and applied as a dense GEMV, redundantly on every GPU (mirrors -qppf_redundancy, qppf.c:182,305).
//
// Shared pieces.  The projector kernels k_gt_fused / k_gt_fused1 / k_gt_dual1 / k_gt_fused1d are built from gt_row_sum (a row of G' left to right, 16 loads in
// flight, one or two coarse vectors), gt_chunk_sum (a long row's chunk sums in order) and gt_epilogue (mode 0 / mode 1), all in this file.  The MPGP vector phase
// folded into k_gt_fused1d is pmh_p1_terms / pmh_split_terms (box_inline.h) and write_partials (reduce.h), the same functions k_p1_dots and k_split_setp
// (mpgp.hip) are made of: that is why its block partials are theirs (tests/test_gpu_projector_paths.py).  Which product of the penalised operator applies is
// PenalizedOp::form() (PMH_PEN_* of pmh_internal.h); mult, mult_epi and mult_same_input switch on it.
#include <chrono>

#include "pmh_internal.h"
#include "reduce.h"
#include "box_inline.h"
#include "dualchain.h"
#include "svm_internal.h"


// y = M x, M dense m x m row-major; one 64-lane wavefront per row
__global__ __launch_bounds__(PMH_BLOCK) void k_dense_gemv(int m, const double *__restrict__ M, const double *__restrict__ x, double *__restrict__ y)
{
  const int row = blockIdx.x * (PMH_BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= m) return;
  double s = 0.0;
  for (int j = lane; j < m; j += 64) s += M[(size_t)row * m + j] * x[j];
  s = pmh_wave_sum(s);
  if (lane == 0) y[row] = s;
}

// ---- GG' assembly on the matrix cores (the one GEMM-shaped item of the path, SURVEY 2.3 K20: the reference builds the
// 6x6 blocks of GG' with BLASgemm("N","T"), extension.c:961) -----------------------------------------------------------
// G is densified TRANSPOSED (Gt: n x Mp row-major, Mp = m rounded up to 16) so that the MFMA operand loads are
// contiguous: for v_mfma_f64_16x16x4_f64 lane l holds A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15]; with C = G G'
// both come from row (k0 + (l>>4)) of Gt, columns i0 + (l&15) and j0 + (l&15).  C/D: col = l&15, row = (l>>4) + 4*reg.
// Every workgroup owns one 16x16 output tile and one K chunk; its 4 wavefronts split the chunk, partial tiles are summed
// in wave order through LDS, and the per-chunk partials are added in chunk order by k_ggt_reduce (deterministic).
typedef double v4f64 __attribute__((ext_vector_type(4)));
#define GGT_KCHUNK 8192

__global__ __launch_bounds__(PMH_BLOCK) void k_densify_gt(int m, int Mp, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val, double *__restrict__ Gt)
{
  const int row = blockIdx.x;
  if (row >= m) return;
  for (int k = rowptr[row] + (int)threadIdx.x; k < rowptr[row + 1]; k += PMH_BLOCK) Gt[(size_t)col[k] * Mp + row] = val[k];
}

__global__ __launch_bounds__(PMH_BLOCK) void k_ggt_mfma(int n, int Mp, const double *__restrict__ Gt, double *__restrict__ part)
{
  __shared__ double lds[PMH_BLOCK / 64][256];
  const int         nt = Mp / 16, ti = blockIdx.x / nt, tj = blockIdx.x % nt, chunk = blockIdx.y;
  const int         lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int         k_lo = chunk * GGT_KCHUNK + wave * (GGT_KCHUNK / 4);
  const int         k_hi = min(n, k_lo + GGT_KCHUNK / 4);
  v4f64             acc  = {0.0, 0.0, 0.0, 0.0};
  const int         kk = lane >> 4, ij = lane & 15;
  for (int k = k_lo; k < k_hi; k += 4) {
    const int  kr = k + kk;
    const bool ok = kr < k_hi;
    const double a = ok ? Gt[(size_t)kr * Mp + ti * 16 + ij] : 0.0;
    const double b = ok ? Gt[(size_t)kr * Mp + tj * 16 + ij] : 0.0;
    acc            = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; r++) lds[wave][((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[r];
  __syncthreads();
  const int t = threadIdx.x; // 256 threads = 256 tile entries
  double    v = lds[0][t];
#pragma unroll
  for (int w = 1; w < PMH_BLOCK / 64; w++) v += lds[w][t];
  part[((size_t)chunk * nt * nt + blockIdx.x) * 256 + t] = v;
}

__global__ __launch_bounds__(PMH_BLOCK) void k_ggt_reduce(int nchunks, int Mp, const double *__restrict__ part, double *__restrict__ GGt)
{
  const int nt = Mp / 16, tile = blockIdx.x, ti = tile / nt, tj = tile % nt, t = threadIdx.x;
  double    v = 0.0;
  for (int c = 0; c < nchunks; c++) v += part[((size_t)c * nt * nt + tile) * 256 + t];
  GGt[(size_t)(ti * 16 + t / 16) * Mp + tj * 16 + (t % 16)] = v;
}

// device GG' (m x m, row-major, returned on the host)
static int device_ggt(pmh_ctx ctx, pmh_csr G, std::vector<double> &ggt, double *mfma_ms)
{
  const int m = G->nrows, n = G->ncols, Mp = ((m + 15) / 16) * 16, nt = Mp / 16;
  const int nchunks = (n + GGT_KCHUNK - 1) / GGT_KCHUNK;
  double   *Gt = nullptr, *part = nullptr, *dggt = nullptr;
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)n * Mp, (void **)&Gt));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)nchunks * nt * nt * 256, (void **)&part));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)Mp * Mp, (void **)&dggt));
  PMH_CHK(pmh_memset(ctx, Gt, 0, sizeof(double) * (size_t)n * Mp));
  hipLaunchKernelGGL(k_densify_gt, dim3(m), dim3(PMH_BLOCK), 0, ctx->stream, m, Mp, (const int *)G->d_rowptr, (const int *)G->d_col, (const double *)G->d_val, Gt);
  PMH_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  hipLaunchKernelGGL(k_ggt_mfma, dim3(nt * nt, nchunks), dim3(PMH_BLOCK), 0, ctx->stream, n, Mp, (const double *)Gt, part);
  hipLaunchKernelGGL(k_ggt_reduce, dim3(nt * nt), dim3(PMH_BLOCK), 0, ctx->stream, nchunks, Mp, (const double *)part, dggt);
  PMH_HIP(hipEventRecord(ctx->ev1, ctx->stream));
  PMH_HIP(hipGetLastError());
  PMH_HIP(hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  PMH_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  if (mfma_ms) *mfma_ms = ms;
  std::vector<double> full((size_t)Mp * Mp);
  PMH_CHK(pmh_memcpy_d2h(ctx, full.data(), dggt, sizeof(double) * full.size()));
  ggt.assign((size_t)m * m, 0.0);
  for (int i = 0; i < m; i++)
    for (int j = 0; j < m; j++) ggt[(size_t)i * m + j] = full[(size_t)i * Mp + j];
  pmh_free(ctx, Gt);
  pmh_free(ctx, part);
  pmh_free(ctx, dggt);
  return PMH_SUCCESS;
}

static int host_cholesky_inverse(int m, std::vector<double> &a)
{
  // in-place lower Cholesky, then inverse via forward/back substitution against the identity
  for (int j = 0; j < m; j++) {
    double d = a[(size_t)j * m + j];
    for (int k = 0; k < j; k++) d -= a[(size_t)j * m + k] * a[(size_t)j * m + k];
    if (!(d > 0.0)) return 1;
    d                    = sqrt(d);
    a[(size_t)j * m + j] = d;
    for (int i = j + 1; i < m; i++) {
      double s = a[(size_t)i * m + j];
      for (int k = 0; k < j; k++) s -= a[(size_t)i * m + k] * a[(size_t)j * m + k];
      a[(size_t)i * m + j] = s / d;
    }
  }
  std::vector<double> inv((size_t)m * m, 0.0), col(m);
  for (int c = 0; c < m; c++) {
    for (int i = 0; i < m; i++) {
      double s = (i == c) ? 1.0 : 0.0;
      for (int k = 0; k < i; k++) s -= a[(size_t)i * m + k] * col[k];
      col[i] = s / a[(size_t)i * m + i];
    }
    for (int i = m - 1; i >= 0; i--) {
      double s = col[i];
      for (int k = i + 1; k < m; k++) s -= a[(size_t)k * m + i] * col[k];
      col[i] = s / a[(size_t)i * m + i];
    }
    for (int i = 0; i < m; i++) inv[(size_t)i * m + c] = col[i];
  }
  a.swap(inv);
  return 0;
}

// a = L L' (lower Cholesky, in place); T = L^{-1} (lower triangular, row-major), S = T'T = a^{-1} (symmetrised by construction)
static int host_cholesky_T(int m, std::vector<double> &a, std::vector<double> &T, std::vector<double> &S)
{
  for (int j = 0; j < m; j++) {
    double d = a[(size_t)j * m + j];
    for (int k = 0; k < j; k++) d -= a[(size_t)j * m + k] * a[(size_t)j * m + k];
    if (!(d > 0.0)) return 1;
    d                    = sqrt(d);
    a[(size_t)j * m + j] = d;
    for (int i = j + 1; i < m; i++) {
      double s = a[(size_t)i * m + j];
      for (int k = 0; k < j; k++) s -= a[(size_t)i * m + k] * a[(size_t)j * m + k];
      a[(size_t)i * m + j] = s / d;
    }
  }
  T.assign((size_t)m * m, 0.0);
  for (int c = 0; c < m; c++) // column c of L^{-1} by forward substitution against e_c
    for (int i = c; i < m; i++) {
      double s = (i == c) ? 1.0 : 0.0;
      for (int k = c; k < i; k++) s -= a[(size_t)i * m + k] * T[(size_t)k * m + c];
      T[(size_t)i * m + c] = s / a[(size_t)i * m + i];
    }
  S.assign((size_t)m * m, 0.0);
  for (int i = 0; i < m; i++)
    for (int j = 0; j <= i; j++) {
      double s = 0.0;
      for (int k = i; k < m; k++) s += T[(size_t)k * m + i] * T[(size_t)k * m + j]; // (T'T)_ij = sum_k T_ki T_kj, k >= max(i, j) = i
      S[(size_t)i * m + j] = S[(size_t)j * m + i] = s;
    }
  return 0;
}

extern "C" int pmh_qppf_create(pmh_ctx ctx, pmh_csr G, int orthonormal, pmh_qppf *out)
{
  PMH_ARG(ctx && G && out);
  pmh_qppf pf    = new pmh_qppf_s();
  pf->ctx        = ctx;
  pf->G          = G;
  pf->m          = G->nrows;
  pf->n          = G->ncols;
  pf->orthonormal = orthonormal ? 1 : 0;
  pf->implicit_orth = 0;
  pf->d_Tt = pf->d_S = pf->tmp_m = nullptr;
  pf->d_inv      = nullptr;
  pf->ggt_mfma_ms = pf->host_inverse_ms = 0.0;
  const int m    = pf->m;
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)(m ? m : 1), (void **)&pf->G_left));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)(m ? m : 1), (void **)&pf->Gt_right));
  if (!pf->orthonormal && m > 0) {
    // GG' on the device with fp64 MFMA (QPPFSetUpGGt_Private qppf.c:213-278); the small dense factorisation stays on the host
    std::vector<double> ggt;
    PMH_CHK(device_ggt(ctx, G, ggt, &pf->ggt_mfma_ms));
    const auto t0 = std::chrono::steady_clock::now();
    const int  bad = host_cholesky_inverse(m, ggt);
    pf->host_inverse_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (bad) {
      pmh_free(ctx, pf->G_left);
      pmh_free(ctx, pf->Gt_right);
      delete pf;
      return pmh_set_error(PMH_ERR_ARG, "pmh_qppf_create: G G' is not positive definite (G must have full row rank)");
    }
    PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)m * m, (void **)&pf->d_inv));
    PMH_CHK(pmh_memcpy_h2d(ctx, pf->d_inv, ggt.data(), sizeof(double) * (size_t)m * m));
  }
  if (orthonormal == 2 && m > 0) {
    // implicit orthonormalisation (the reference's -qp_E_orth_form implicit, qptransform.c:647, permonmatorth.c:176-205: the orthonormalised
    // matrix is never formed): G stays as sparse as it came (an explicit T G0 fills every row of a subdomain's modes with the columns of all
    // subdomains before it: 3.4 x the non-zeros for configs[2]); GG' = L L' on the device / host as above, T = L^{-1}, S = T'T = (GG')^{-1}
    std::vector<double> ggt;
    PMH_CHK(device_ggt(ctx, G, ggt, &pf->ggt_mfma_ms));
    const auto          t0 = std::chrono::steady_clock::now();
    std::vector<double> T, S;
    const int           bad = host_cholesky_T(m, ggt, T, S);
    pf->host_inverse_ms     = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (bad) {
      pmh_free(ctx, pf->G_left);
      pmh_free(ctx, pf->Gt_right);
      delete pf;
      return pmh_set_error(PMH_ERR_ARG, "pmh_qppf_create: G G' is not positive definite (G must have full row rank)");
    }
    std::vector<double> Tt((size_t)m * m);
    for (int i = 0; i < m; i++)
      for (int j = 0; j < m; j++) Tt[(size_t)j * m + i] = T[(size_t)i * m + j];
    const size_t bytes = sizeof(double) * (size_t)m * m;
    PMH_CHK(pmh_malloc(ctx, bytes, (void **)&pf->d_Tt));
    PMH_CHK(pmh_malloc(ctx, bytes, (void **)&pf->d_S));
    PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)m, (void **)&pf->tmp_m));
    PMH_CHK(pmh_memcpy_h2d(ctx, pf->d_Tt, Tt.data(), bytes));
    PMH_CHK(pmh_memcpy_h2d(ctx, pf->d_S, S.data(), bytes)); // symmetric: its own transpose
    pf->h_T           = T;
    pf->implicit_orth = 1;
  }
  *out = pf;
  return PMH_SUCCESS;
}

// e = T e0: the right-hand side of the implicitly orthonormalised constraint (T G0) lambda = T e0 (host vectors of length m)
extern "C" int pmh_qppf_orth_rhs(pmh_qppf pf, const double *e0, double *e)
{
  PMH_ARG(pf && e0 && e);
  if (!pf->implicit_orth) return pmh_set_error(PMH_ERR_STATE, "pmh_qppf_orth_rhs: the projector was not created with implicit orthonormalisation");
  const int m = pf->m;
  for (int i = 0; i < m; i++) {
    double s = 0.0;
    for (int j = 0; j <= i; j++) s += pf->h_T[(size_t)i * m + j] * e0[j];
    e[i] = s;
  }
  return PMH_SUCCESS;
}

// set-up cost of the coarse problem (SURVEY 8d asks for them separately): the GG' assembly on the matrix cores
// (k_ggt_mfma + its fixed-order reduction; 2 Mp^2 n flops with Mp = m rounded up to 16) and the host Cholesky + inverse
extern "C" int pmh_qppf_setup_stats(pmh_qppf pf, double *ggt_mfma_ms, double *ggt_flops, double *host_inverse_ms)
{
  PMH_ARG(pf);
  const double Mp = (double)(((pf->m + 15) / 16) * 16);
  if (ggt_mfma_ms) *ggt_mfma_ms = pf->ggt_mfma_ms;
  if (ggt_flops) *ggt_flops = pf->orthonormal ? 0.0 : 2.0 * Mp * Mp * (double)pf->n;
  if (host_inverse_ms) *host_inverse_ms = pf->host_inverse_ms;
  return PMH_SUCCESS;
}

extern "C" int pmh_qppf_destroy(pmh_qppf pf)
{
  if (!pf) return PMH_SUCCESS;
  pmh_free(pf->ctx, pf->G_left);
  pmh_free(pf->ctx, pf->Gt_right);
  if (pf->d_inv) pmh_free(pf->ctx, pf->d_inv);
  if (pf->d_Tt) pmh_free(pf->ctx, pf->d_Tt), pmh_free(pf->ctx, pf->d_S), pmh_free(pf->ctx, pf->tmp_m);
  if (pf->or_part) pmh_free(pf->ctx, pf->or_part);
  if (pf->or_s) pmh_free(pf->ctx, pf->or_s);
  delete pf;
  return PMH_SUCCESS;
}

// one-row projector: (G G')^{-1} as the generic code applies it (orthonormal rows: the identity)
static inline double onerow_inv(pmh_qppf pf) { return pf->orthonormal ? 1.0 : 1.0 / pf->row_aat; }

extern "C" int pmh_qppf_apply_G(pmh_qppf pf, const double *v, double *Gv)
{
  PMH_ARG(pf);
  if (pf->m == 0) return PMH_SUCCESS;
  if (pf->onerow) return pmh_onerow_dot(pf, v, 1.0, Gv);
  if (pf->implicit_orth) return pmh_csr_mult_then_dense(pf->G, v, pf->d_Tt, pf->tmp_m, Gv); // (T G0) v
  return pmh_csr_mult(pf->G, v, Gv);
}

// G v and ||G v||^2 (-> scalar slot, device + pinned host) without waiting: one launch pair where the implicit form with m <= 64 allows it
int pmh_qppf_apply_G_norm2(pmh_qppf pf, const double *v, double *Gv, int slot)
{
  if (pf->m == 0) return PMH_SUCCESS;
  if (pf->implicit_orth && pf->m <= 64) return pmh_csr_mult_then_dense(pf->G, v, pf->d_Tt, pf->tmp_m, Gv, slot);
  PMH_CHK(pmh_qppf_apply_G(pf, v, Gv));
  return pmh_k_dot_partials(pf->ctx, pf->m, Gv, Gv, slot);
}

// G_left = what G' is applied to in Q v = G'(..): G v for orthonormal rows, S G0 v under implicit orthonormalisation
static int qppf_left(pmh_qppf pf, const double *v)
{
  if (pf->implicit_orth) return pmh_csr_mult_then_dense(pf->G, v, pf->d_S, pf->tmp_m, pf->G_left);
  return pmh_csr_mult(pf->G, v, pf->G_left);
}

// QPPFApplyCP qppf.c:610-645
extern "C" int pmh_qppf_apply_CP(pmh_qppf pf, const double *x, double *y)
{
  PMH_ARG(pf);
  if (pf->m == 0) return PMH_SUCCESS;
  if (pf->onerow && !pf->orthonormal) {
    PMH_CHK(pmh_vec_copy(pf->ctx, 1, x, y));
    return pmh_vec_scale(pf->ctx, 1, y, onerow_inv(pf));
  }
  if (!pf->d_inv) return pmh_vec_copy(pf->ctx, pf->m, x, y);
  hipLaunchKernelGGL(k_dense_gemv, dim3((pf->m + 3) / 4), dim3(PMH_BLOCK), 0, pf->ctx->stream, pf->m, pf->d_inv, x, y);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

// QPPFApplyQ qppf.c:454-503
extern "C" int pmh_qppf_apply_Q(pmh_qppf pf, const double *v, double *Qv)
{
  PMH_ARG(pf && (const void *)v != (const void *)Qv);
  if (pf->m == 0) return pmh_vec_set(pf->ctx, pf->n, Qv, 0.0);
  if (pf->onerow) {
    PMH_CHK(pmh_onerow_dot(pf, v, 1.0, pf->or_s));
    return pmh_onerow_scaled_row(pf, pf->or_s, onerow_inv(pf), nullptr, Qv);
  }
  PMH_CHK(qppf_left(pf, v));
  if (pf->d_inv) {
    PMH_CHK(pmh_qppf_apply_CP(pf, pf->G_left, pf->Gt_right));
    return pmh_csr_mult_transpose(pf->G, pf->Gt_right, Qv);
  }
  return pmh_csr_mult_transpose(pf->G, pf->G_left, Qv);
}

// QPPFApplyP qppf.c:563-575: Pv = v - Qv  (VecAYPX(Pv,-1,v))
extern "C" int pmh_qppf_apply_P(pmh_qppf pf, const double *v, double *Pv)
{
  if (pf && pf->onerow && pf->m) {
    PMH_ARG((const void *)v != (const void *)Pv);
    PMH_CHK(pmh_onerow_dot(pf, v, 1.0, pf->or_s));
    return pmh_onerow_scaled_row(pf, pf->or_s, onerow_inv(pf), v, Pv);
  }
  PMH_CHK(pmh_qppf_apply_Q(pf, v, Pv));
  return pmh_vec_aypx(pf->ctx, pf->n, Pv, -1.0, v);
}

// QPPFApplyGtG qppf.c:580-605
extern "C" int pmh_qppf_apply_GtG(pmh_qppf pf, const double *v, double *y)
{
  PMH_ARG(pf);
  if (pf->orthonormal) return pmh_qppf_apply_Q(pf, v, y);
  if (pf->m == 0) return pmh_vec_set(pf->ctx, pf->n, y, 0.0);
  if (pf->onerow) {
    PMH_CHK(pmh_onerow_dot(pf, v, 1.0, pf->or_s));
    return pmh_onerow_scaled_row(pf, pf->or_s, 1.0, nullptr, y);
  }
  PMH_CHK(pmh_csr_mult(pf->G, v, pf->G_left));
  return pmh_csr_mult_transpose(pf->G, pf->G_left, y);
}

// QPPFApplyHalfQ qppf.c:507-527: y = (GG')^{-1} G x  (length m)
extern "C" int pmh_qppf_apply_halfQ(pmh_qppf pf, const double *x, double *y)
{
  PMH_ARG(pf);
  if (pf->m == 0) return PMH_SUCCESS;
  if (pf->onerow) return pmh_onerow_dot(pf, x, onerow_inv(pf), y);
  if (pf->implicit_orth) return pmh_csr_mult_then_dense(pf->G, x, pf->d_Tt, pf->tmp_m, y); // (GG')^{-1} = I for G = T G0: y = T G0 x
  PMH_CHK(pmh_csr_mult(pf->G, x, pf->G_left));
  return pmh_qppf_apply_CP(pf, pf->G_left, y);
}

// QPPFApplyHalfQTranspose qppf.c:531-559: y = G'(GG')^{-1} x
extern "C" int pmh_qppf_apply_halfQ_transpose(pmh_qppf pf, const double *x, double *y)
{
  PMH_ARG(pf);
  if (pf->m == 0) return pmh_vec_set(pf->ctx, pf->n, y, 0.0);
  if (pf->onerow) return pmh_onerow_scaled_row(pf, x, onerow_inv(pf), nullptr, y);
  if (pf->implicit_orth) { // (T G0)' x = G0' (T' x); k_dense_gemv takes a row-major matrix: T' row-major = d_Tt
    hipLaunchKernelGGL(k_dense_gemv, dim3((pf->m + 3) / 4), dim3(PMH_BLOCK), 0, pf->ctx->stream, pf->m, (const double *)pf->d_Tt, x, pf->Gt_right);
    PMH_HIP(hipGetLastError());
    return pmh_csr_mult_transpose(pf->G, pf->Gt_right, y);
  }
  if (pf->d_inv) {
    PMH_CHK(pmh_qppf_apply_CP(pf, x, pf->Gt_right));
    return pmh_csr_mult_transpose(pf->G, pf->Gt_right, y);
  }
  return pmh_csr_mult_transpose(pf->G, x, y);
}

// ---- fused epilogues of the projector's G' product (orthonormal G) ----------------------------------------------------
// One launch instead of G' w + VecWAXPY, resp. G' w + VecAYPX + VecScale + VecAXPY: the replicated dual-space work of one
// A_rho = P F P + rho Q application drops from 15 to 10 launches (each ~5 us: what limits the 8-GPU share of configs[2]).
// The row sum is taken exactly as the stream SpMV takes it for these rows (8 lanes per row striding the row, shuffle tree 4-2-1),
// and the epilogue arithmetic is the unfused sequence term by term, so the result is bit-identical to the separate calls:
//   mode 0:  s = (G'w)_r;  y_r = s;  z_r = (-1) s + x_r                      (Q x, and P x = x - Q x: VecWAXPY)
//   mode 1:  s = (G'w)_r;  t = x_r + (-1) s;  y_r = y_r rho + t              (VecAYPX, VecScale, VecAXPY of matpenalized.c:12-22)
// The pieces the kernels below share.  gt_epilogue: the two epilogues above for row r with sum s = (G'w)_r; mode 1 returns the new y_r and stores it where STORE.
template <bool STORE = true>
static __device__ __forceinline__ double gt_epilogue(int mode, int r, double sum, const double *__restrict__ x, double *__restrict__ y, double *__restrict__ z, double rho)
{
  if (mode == 0) {
    y[r] = sum;
    z[r] = -1.0 * sum + x[r];
    return 0.0;
  }
  const double t   = x[r] + -1.0 * sum;
  const double out = y[r] * rho + t;
  if (STORE) y[r] = out;
  return out;
}
// gt_row_sum: entries [k0, k1) of a CSR row against NV coarse vectors that share the loads of the row, each sum left to right as the plain loop, the loads of 16
// entries in flight together (G0' has 6 or 12 entries per row: one trip)
template <int NV>
static __device__ __forceinline__ void gt_row_sum(int k0, int k1, const int *__restrict__ col, const double *__restrict__ val, const double *w0, const double *w1, double (&s)[NV])
{
  for (int k = k0; k < k1; k += 16) {
    double v[16];
    int    c[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const bool in = k + j < k1;
      v[j] = in ? val[k + j] : 0.0, c[j] = in ? col[k + j] : 0;
    }
#pragma unroll
    for (int j = 0; j < 16; j++)
      if (k + j < k1) {
        s[0] += v[j] * w0[c[j]];
        if (NV == 2) s[NV - 1] += v[j] * w1[c[j]];
      }
  }
}
// gt_chunk_sum: the chunk sums of long row t (k_spmv_long_part) added in chunk order, 8 loads in flight
static __device__ __forceinline__ double gt_chunk_sum(const int *__restrict__ lrow, const double *__restrict__ part, int t)
{
  const int c0 = lrow[t], c1 = lrow[t + 1];
  double    sum = 0.0;
  for (int c = c0; c < c1; c += 8) {
    double v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = (c + j < c1) ? part[c + j] : 0.0;
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (c + j < c1) sum += v[j];
  }
  return sum;
}

__global__ __launch_bounds__(PMH_BLOCK) void k_gt_fused(int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val, const double *__restrict__ w, int mode,
                                                       const double *__restrict__ x, double *__restrict__ y, double *__restrict__ z, double rho)
{
  const int sub = threadIdx.x >> 3, lane = threadIdx.x & 7;
  const int r   = blockIdx.x * (PMH_BLOCK / 8) + sub;
  double    sum = 0.0;
  if (r < n) {
    const int k0 = rowptr[r], k1 = rowptr[r + 1];
    for (int k = k0 + lane; k < k1; k += 8) sum += val[k] * w[col[k]];
  }
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) sum += __shfl_down(sum, o, 8);
  if (r < n && lane == 0) gt_epilogue(mode, r, sum, x, y, z, rho);
}

// the same for short rows (the one-lane-per-row case of the stream kernel: a row is summed left to right by one thread), e.g. the <= 12
// entries per row of an un-filled G0' under implicit orthonormalisation
__global__ __launch_bounds__(PMH_BLOCK) void k_gt_fused1(int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val, const double *__restrict__ w, int mode,
                                                        const double *__restrict__ x, double *__restrict__ y, double *__restrict__ z, double rho)
{
  const int r = blockIdx.x * PMH_BLOCK + threadIdx.x;
  if (r >= n) return;
  double s[1] = {0.0};
  gt_row_sum<1>(rowptr[r], rowptr[r + 1], col, val, w, nullptr, s);
  gt_epilogue(mode, r, s[0], x, y, z, rho);
}

// G not orthonormalised (the dense (G G')^{-1} of QPPFSetUp, qppf.c:213-278): the penalty term rho G'G x and the projector's G'(GG')^{-1}G x are two
// G' products with different coarse vectors -- one pass over G' for both: y = G' t0 (t0 = G x), z = x - G' w (w = (GG')^{-1} t0), each sum left to right
__global__ __launch_bounds__(PMH_BLOCK) void k_gt_dual1(int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val, const double *__restrict__ t0,
                                                       const double *__restrict__ w, const double *__restrict__ x, double *__restrict__ y, double *__restrict__ z)
{
  const int r = blockIdx.x * PMH_BLOCK + threadIdx.x;
  if (r >= n) return;
  double s[2] = {0.0, 0.0};
  gt_row_sum<2>(rowptr[r], rowptr[r + 1], col, val, t0, w, s);
  y[r] = s[0];
  z[r] = -1.0 * s[1] + x[r];
}

// ... and with the finishing step of G0 v and the dense T'T product folded in (implicit orthonormalisation, m <= 64): every workgroup adds the chunk sums of
// k_spmv_long_part per row in chunk order and applies the m x m matrix exactly as k_rows_then_dense does (same order => same bits), then takes its rows -- one
// launch less per projector application aux (workgroup 0 only; SMALXE's ||B u|| riding along): the chunk sums of G0 u (part2, from k_spmv_long_part2) are added
// per row, T is applied and ||T G0 u||^2 is summed exactly as k_rows_then_dense does it -- the same bits as the two launches of pmh_qppf_apply_G_norm2. epi:
// the MPGP vector phase that follows the product, folded in (mode 1 only; one row per thread = the grid of the streaming Vec kernels, so the block partials
// equal those of k_p1_dots / k_axpy + k_split_setp).
struct gt_aux {
  const double *part2, *Mt2; // chunk sums of G0 u, T' (row-major)
  double       *y2, *norm_d, *norm_h;
};
template <int EPI>
__global__ __launch_bounds__(PMH_BLOCK) void k_gt_fused1d(int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val, int m, const int *__restrict__ lrow,
                                                         const double *__restrict__ part, const double *__restrict__ Mt, int mode, const double *__restrict__ x, double *__restrict__ y,
                                                         double *__restrict__ z, double rho, gt_aux aux, pmh_vec_epi epi, const double *__restrict__ pin)
{
  // A 5-8 us kernel is made of memory latencies, not of bytes: every loop below keeps the order of its sum (the same bits as the plain loops) but sends its
  // loads out together -- the plain forms compile to load - wait - add per entry, i.e. ~6 + 12 + 12 latencies in a row (measured 7.7 us against ~4 for a
  // launch).
  __shared__ double t0[64], w[64], Ms[64 * 64];
  const int t = threadIdx.x, mm = m * m;
  // the small matrix goes to LDS while the chunk sums are added (m <= 64: at most 16 entries per thread)
  double mreg[16];
#pragma unroll
  for (int e = 0; e < 16; e++) mreg[e] = (t + PMH_BLOCK * e < mm) ? Mt[t + PMH_BLOCK * e] : 0.0;
  const int r  = blockIdx.x * PMH_BLOCK + t;
  int       k0 = 0, k1 = 0;
  if (r < n) k0 = rowptr[r], k1 = rowptr[r + 1];
  if (t < m) t0[t] = gt_chunk_sum(lrow, part, t);
#pragma unroll
  for (int e = 0; e < 16; e++)
    if (t + PMH_BLOCK * e < mm) Ms[t + PMH_BLOCK * e] = mreg[e];
  __syncthreads();
  if (t < m) {
    double s = 0.0;
    for (int c = 0; c < m; c++) s += Ms[c * m + t] * t0[c];
    w[t] = s;
  }
  __syncthreads();
  if (aux.part2 && blockIdx.x == 0) { // uniform per workgroup.  k_rows_then_dense(m, lrow, part2, Mt2, y2, norm): same sums, same order
    __shared__ double t2[64], red2[PMH_BLOCK / 64];
    if (t < m) t2[t] = gt_chunk_sum(lrow, aux.part2, t);
    __syncthreads();
    double sq = 0.0;
    if (t < m) {
      double s = 0.0;
      for (int c = 0; c < m; c += 16) {
        double v[16];
#pragma unroll
        for (int j = 0; j < 16; j++) v[j] = (c + j < m) ? aux.Mt2[(size_t)(c + j) * m + t] : 0.0;
#pragma unroll
        for (int j = 0; j < 16; j++)
          if (c + j < m) s += v[j] * t2[c + j];
      }
      aux.y2[t] = s;
      sq += s * s;
    }
    sq = pmh_block_reduce<PMH_RED_SUM>(sq, red2);
    if (t == 0) *aux.norm_d = sq, *aux.norm_h = sq;
  }
  double sum[1] = {0.0}, out = 0.0;
  if (r < n) {
    gt_row_sum<1>(k0, k1, col, val, w, nullptr, sum);
    out = gt_epilogue<EPI != PMH_VEPI_GRAD_SPLIT>(mode, r, sum[0], x, y, z, rho);
  }
  double *const rows = epi.partials + (size_t)epi.prow * epi.ld; // this epilogue's rows of the block partials
  if (EPI == PMH_VEPI_P1) { // k_p1_dots (mpgp.hip) on this workgroup's rows: p'Ap, g'p, QPCFeas -- `out` is Ap[r], pin the operator's input p
    __shared__ double redp[PMH_BLOCK / 64];
    double            s[3] = {0.0, 0.0, INFINITY};
    if (r < n) pmh_p1_terms(s, pin[r], out, epi.g[r], epi.xx, epi.lb, epi.ub, r);
    write_partials<3>(s, {PMH_RED_SUM, PMH_RED_SUM, PMH_RED_MIN}, redp, rows, epi.ld);
  }
  // k_axpy(g, -1, b) + k_split_setp (mpgp.hip): g = A x - b, gf, p = gf, the partials of (0, |gP|^2, |gc|^2, |gf|^2) -- pin is the iterate
  if (EPI == PMH_VEPI_GRAD_SPLIT) {
    __shared__ double redg[PMH_BLOCK / 64];
    double            acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (r < n) {
      double gi = out;
      gi += -1.0 * epi.b[r];
      y[r]           = gi;
      const double f = pmh_split_terms(acc, pin[r], gi, epi.lb, epi.ub, r, epi.astol);
      epi.gf[r]      = f;
      epi.p[r]       = f;
    }
    write_partials<4>(acc, redg, rows, epi.ld);
  }
}

// the fused path applies when G' is summed in the order of a row-block plan (8 lanes per row for a few dozen entries per row: the rigid-body
// modes of the subdomains a dual row touches; 1 for shorter rows), otherwise the callers keep the unfused sequence
static bool gt_fusable(pmh_qppf pf)
{
  if (pf->onerow || !pf->orthonormal || pf->d_inv || pf->m == 0 || !pmh_knobs().gt_fusion) return false;
  if (!pf->G->transpose && pmh_csr_ensure_transpose(pf->G)) return false;
  return pmh_csr_row_lanes(pf->G->transpose) != 0;
}

// the same for G with its dense (G G')^{-1}: one-lane-per-row G' only (k_gt_dual1 / k_gt_fused1)
static bool gt_fusable_dense_inverse(pmh_qppf pf)
{
  if (pf->onerow || pf->orthonormal || !pf->d_inv || pf->m == 0 || !pmh_knobs().gt_fusion) return false;
  if (!pf->G->transpose && pmh_csr_ensure_transpose(pf->G)) return false;
  return pmh_csr_row_lanes(pf->G->transpose) == 1;
}

// Q v's G' product with its vector epilogue, starting from v: G0 v (chunk sums), then everything else in ONE launch where the folded kernel
// applies (implicit orthonormalisation, long-row G0, short-row G0', m <= 64); otherwise qppf_left + gt_fused
static int gt_fused(pmh_qppf pf, const double *w, int mode, const double *x, double *y, double *z, double rho);
static int qppf_left(pmh_qppf pf, const double *v);
// the one-launch form (k_gt_fused1d) applies: implicit orthonormalisation, long-row G0, one-lane-per-row G0', m <= 64
static bool q_fused_dense(pmh_qppf pf)
{
  return pf->implicit_orth && pf->G->l_nchunks > 0 && pf->m <= 64 && pf->G->transpose && pmh_csr_row_lanes(pf->G->transpose) == 1;
}
// aux_u != nullptr (one-launch form only): G0 aux_u shares the pass over G0, T G0 aux_u -> aux_Gu and its squared norm -> scalar slot aux_slot by workgroup 0.
// epi (mode 1, one-launch form only): the vector phase folded into the kernel, pin = the operator's input vector.
static int q_fused(pmh_qppf pf, const double *v, int mode, const double *x, double *y, double *z, double rho, const double *aux_u = nullptr, double *aux_Gu = nullptr, int aux_slot = -1,
                   const pmh_vec_epi *epi = nullptr, const double *pin = nullptr)
{
  const pmh_csr Gt = pf->G->transpose;
  if (q_fused_dense(pf)) {
    const int    *lrow;
    const double *part, *part2 = nullptr;
    if (aux_u) PMH_CHK(pmh_csr_mult_partials2(pf->G, v, aux_u, &lrow, &part, &part2));
    else PMH_CHK(pmh_csr_mult_partials(pf->G, v, &lrow, &part));
    gt_aux aux;
    memset(&aux, 0, sizeof(aux));
    if (aux_u) aux.part2 = part2, aux.Mt2 = pf->d_Tt, aux.y2 = aux_Gu, aux.norm_d = pf->ctx->d_scal + aux_slot, aux.norm_h = pf->ctx->h_scal + aux_slot;
    pmh_vec_epi e;
    memset(&e, 0, sizeof(e));
    if (epi) e = *epi;
    const dim3 grid((Gt->nrows + PMH_BLOCK - 1) / PMH_BLOCK);
#define GT1D(EPI)                                                                                                                                                                                            \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gt_fused1d<EPI>), grid, dim3(PMH_BLOCK), 0, pf->ctx->stream, Gt->nrows, (const int *)Gt->d_rowptr, (const int *)Gt->d_col, (const double *)Gt->d_val, pf->m, lrow, part, \
                     (const double *)pf->d_S, mode, x, y, z, rho, aux, e, pin)
    if (e.kind == PMH_VEPI_P1) GT1D(PMH_VEPI_P1);
    else if (e.kind == PMH_VEPI_GRAD_SPLIT) GT1D(PMH_VEPI_GRAD_SPLIT);
    else GT1D(0);
#undef GT1D
    PMH_HIP(hipGetLastError());
    return PMH_SUCCESS;
  }
  if (aux_u || epi) return pmh_set_error(PMH_ERR_STATE, "q_fused: the folded forms need the one-launch projector kernel");
  PMH_CHK(qppf_left(pf, v));
  return gt_fused(pf, pf->G_left, mode, x, y, z, rho);
}

static int gt_fused(pmh_qppf pf, const double *w, int mode, const double *x, double *y, double *z, double rho)
{
  const pmh_csr Gt = pf->G->transpose;
  if (pmh_csr_row_lanes(Gt) == 1)
    hipLaunchKernelGGL(k_gt_fused1, dim3((Gt->nrows + PMH_BLOCK - 1) / PMH_BLOCK), dim3(PMH_BLOCK), 0, pf->ctx->stream, Gt->nrows, (const int *)Gt->d_rowptr, (const int *)Gt->d_col, (const double *)Gt->d_val, w,
                       mode, x, y, z, rho);
  else
  hipLaunchKernelGGL(k_gt_fused, dim3((Gt->nrows + PMH_BLOCK / 8 - 1) / (PMH_BLOCK / 8)), dim3(PMH_BLOCK), 0, pf->ctx->stream, Gt->nrows, (const int *)Gt->d_rowptr, (const int *)Gt->d_col,
                     (const double *)Gt->d_val, w, mode, x, y, z, rho);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

// ---- shell operators of the transform chain ------------------------------------------------------------------------
struct ProjectedOp : pmh_op_s {
  pmh_op   A;
  pmh_qppf pf;
  int      symmetric;
  double  *w1, *w2;
  ~ProjectedOp() override
  {
    pmh_free(ctx, w1);
    pmh_free(ctx, w2);
  }
  // MatCreateProd(P,A,P) / (P,A): qptransform.c:273-284, matprod.c:42-48
  int mult(const double *x, double *y) override
  {
    if (symmetric) {
      PMH_CHK(pmh_qppf_apply_P(pf, x, w1));
      PMH_CHK(A->mult(w1, w2));
    } else {
      PMH_CHK(A->mult(x, w2));
    }
    return pmh_qppf_apply_P(pf, w2, y);
  }
  // (P A P)' = P A' P; (P A)' = A' P
  int mult_transpose(const double *x, double *y) override
  {
    PMH_CHK(pmh_qppf_apply_P(pf, x, w1));
    if (symmetric) {
      PMH_CHK(A->mult_transpose(w1, w2));
      return pmh_qppf_apply_P(pf, w2, y);
    }
    return A->mult_transpose(w1, y);
  }
  // same, with Q x supplied by the caller (the QPPFApplyQ cache hit of qppf.c:464-467)
  int mult_with_Qx(const double *x, const double *Qx, double *y)
  {
    if (symmetric) {
      PMH_CHK(pmh_vec_waxpy(ctx, n, w1, -1.0, Qx, x)); // P x = x - Q x
      PMH_CHK(A->mult(w1, w2));
    } else {
      PMH_CHK(A->mult(x, w2));
    }
    return pmh_qppf_apply_P(pf, w2, y);
  }
};

struct PenalizedOp : pmh_op_s {
  pmh_op   A;
  pmh_qppf pf;
  double   rho;
  double  *t, *xwork = nullptr;
  // ||G u|| request riding on the next product (pmh_op_penalized_arm_aux_normG)
  const double *aux_u = nullptr;
  double       *aux_Gu = nullptr;
  int           aux_slot = -1, aux_done = 0;
  // the five-launch chain (dualchain.hip) where F offers its stages: created at the first product
  pmh_dualchain dc = nullptr;
  int           dc_state = -1; // -1 not asked yet, 0 does not apply, 1 live
  int           chain_allowed = 1; // pmh_set_knob("chain") as it stood when the operator was created
  // the inner operator where it is P . P with this very projector (the forms below fold the two projections into the penalty term's pass), else null
  ProjectedOp *projected()
  {
    ProjectedOp *pa = dynamic_cast<ProjectedOp *>(A);
    return pa && pa->pf == pf && pa->symmetric ? pa : nullptr;
  }
  pmh_dualchain chain()
  {
    if (dc_state < 0) {
      dc_state        = 0;
      ProjectedOp *pa = projected();
      if (chain_allowed && !pf->onerow && pa && pmh_dc_create(pf, pa->A, &dc) == PMH_SUCCESS && dc) {
        dc_state = 1;
        if (norm_Gu) (void)pmh_dc_set_norm_target(dc, norm_Gu, norm_slot);
      }
    }
    return dc_state == 1 ? dc : nullptr;
  }
  double *norm_Gu = nullptr;
  int     norm_slot = -1;
  // The dense-row SVM operator under a one-row projector whose row is c y (the bias equality y'a = 0): rho G'G = rho c^2 y y' is the operator's own rank-one
  // term -- the product is the operator's, with sigma_fold set around it (the operator on its own, e.g. in SMALXE's power iterations, stays unpenalised), every
  // fused epilogue it has stays on, and ||G u|| = |c sum_i y_i u_i| comes out of the pass that holds the iterate's rows (svm.hip aux_*).  rho is read at every
  // product, so pmh_op_penalized_set_penalty needs nothing more.  Probed once, at the first product (one pass over the row and the labels)
  // The CSR operator (svm_csr.hip) folds the same way; it has no fused epilogue and does not serve the ||G u|| request (the projector's own dot runs).
  SvmDualBase *sv = nullptr;
  double       sv_c = 0.0;
  int          sv_state = -1;
  SvmDualBase *fold()
  {
    if (sv_state < 0) {
      sv_state       = 0;
      SvmDualBase *o = pf->onerow ? dynamic_cast<SvmDualBase *>(A) : nullptr;
      if (o && pmh_svm_op_row_is_labels(o, pf, &sv_c) == 1) sv = o, sv_state = 1;
    }
    return sv_state == 1 ? sv : nullptr;
  }
  int spec_expansion_ready() override { return sv_state == 1 ? sv->spec_expansion_ready() : 0; }
  int fold_apply(const double *x, double *y, const pmh_vec_epi *e)
  {
    const double *au = aux_u;
    sv->sigma_fold   = rho * sv_c * sv_c;
    sv->aux_done     = 0;
    if (au) sv->aux_u = au, sv->aux_Gu = aux_Gu, sv->aux_slot = aux_slot, sv->aux_c = sv_c;
    const int rc   = e ? sv->mult_epi(x, y, *e) : sv->mult(x, y);
    sv->sigma_fold = 0.0, sv->aux_u = nullptr;
    if (rc != PMH_EPI_UNSUPPORTED) aux_u = nullptr; // (a declined epilogue is followed by the plain product of the same vector: the request waits for it)
    if (sv->aux_done) aux_done = 1, sv->aux_done = 0;
    return rc;
  }
  int  emit_begin(const double *x, const double *p, pmh_emit_args *ea) override { return chain() ? pmh_dc_emit_begin(dc, x, p, ea) : PMH_EPI_UNSUPPORTED; }
  void emit_invalidate(bool keep_applied = false) override
  {
    if (dc) pmh_dc_invalidate(dc, keep_applied);
  }
  // the one-launch projector form applies (asked on its own by pmh_op_penalized_arm_aux_normG, which must not set the chain up)
  bool one_launch() { return projected() && gt_fusable(pf) && q_fused_dense(pf); }
  // Which product the knobs and the operands allow (PMH_PEN_*): asked at every product, because gt_fusion, vec_epi and svm_pairing may change between two products
  // of one operator; only the fold's and the chain's own probes are kept
  int form()
  {
    if (fold()) return PMH_PEN_FOLD;
    if (chain()) return PMH_PEN_CHAIN;
    if (projected()) {
      if (gt_fusable(pf)) return q_fused_dense(pf) ? PMH_PEN_ONE_LAUNCH : PMH_PEN_TEN_LAUNCH;
      if (gt_fusable_dense_inverse(pf)) return PMH_PEN_DENSE_INVERSE;
    }
    return PMH_PEN_PLAIN;
  }
  // y = rho Q x + P F (P x) [+ vector epilogue]: 10 launches (see k_gt_fused), one launch per projector where q_fused folds it (PMH_PEN_ONE_LAUNCH)
  int mult_fused_dense(const double *x, double *y, const pmh_vec_epi *epi)
  {
    ProjectedOp *pa = static_cast<ProjectedOp *>(A);
    const double *au = aux_u;
    aux_u            = nullptr;
    PMH_CHK(q_fused(pf, x, 0, x, y, pa->w1, 0.0, au, aux_Gu, aux_slot)); // y = Q x, w1 = P x (+ T G0 u and its squared norm)
    if (au) aux_done = 1;
    PMH_CHK(pa->A->mult(pa->w1, pa->w2));
    return q_fused(pf, pa->w2, 1, pa->w2, y, nullptr, rho, nullptr, nullptr, -1, epi, x); // y = rho y + (w2 - Q w2) (+ the vector phase)
  }
  // y = rho G'G x + P F P x, P = I - G'(GG')^{-1}G: G x once for both terms, one pass over G' for G'(G x) and x - G'(GG')^{-1}(G x), the second
  // projector with the penalty update in its epilogue -- 12 launches instead of 19, the same bits as the plain sequence
  int mult_dense_inverse(const double *x, double *y)
  {
    ProjectedOp  *pa = static_cast<ProjectedOp *>(A);
    const pmh_csr Gt = pf->G->transpose;
    const dim3    grid((Gt->nrows + PMH_BLOCK - 1) / PMH_BLOCK);
    PMH_CHK(pmh_csr_mult(pf->G, x, pf->G_left));
    PMH_CHK(pmh_qppf_apply_CP(pf, pf->G_left, pf->Gt_right));
    hipLaunchKernelGGL(k_gt_dual1, grid, dim3(PMH_BLOCK), 0, ctx->stream, Gt->nrows, (const int *)Gt->d_rowptr, (const int *)Gt->d_col, (const double *)Gt->d_val, (const double *)pf->G_left,
                       (const double *)pf->Gt_right, x, y, pa->w1);
    PMH_HIP(hipGetLastError());
    PMH_CHK(pa->A->mult(pa->w1, pa->w2));
    PMH_CHK(pmh_csr_mult(pf->G, pa->w2, pf->G_left));
    PMH_CHK(pmh_qppf_apply_CP(pf, pf->G_left, pf->Gt_right));
    hipLaunchKernelGGL(k_gt_fused1, grid, dim3(PMH_BLOCK), 0, ctx->stream, Gt->nrows, (const int *)Gt->d_rowptr, (const int *)Gt->d_col, (const double *)Gt->d_val, (const double *)pf->Gt_right, 1,
                       (const double *)pa->w2, y, (double *)nullptr, rho);
    PMH_HIP(hipGetLastError());
    return PMH_SUCCESS;
  }
  // MatMult_Penalized matpenalized.c:12-22: y = BtB x; y *= rho; y = y + A x
  int mult_plain(const double *x, double *y)
  {
    ProjectedOp *pa = projected();
    PMH_CHK(pmh_qppf_apply_GtG(pf, x, y));
    if (pa && pf->orthonormal) {
      PMH_CHK(pa->mult_with_Qx(x, y, t)); // y currently holds Q x: reuse it before scaling
    } else {
      PMH_CHK(A->mult(x, t));
    }
    PMH_CHK(pmh_vec_scale(ctx, n, y, rho));
    return pmh_vec_axpy(ctx, n, y, 1.0, t);
  }
  int mult(const double *x, double *y) override
  {
    const int f = form();
    if (f != PMH_PEN_FOLD && f != PMH_PEN_CHAIN && f != PMH_PEN_ONE_LAUNCH) aux_u = nullptr; // a ||G u|| request rides on the fold's pass or the one-launch form only
    switch (f) {
    case PMH_PEN_FOLD: return fold_apply(x, y, nullptr);
    case PMH_PEN_CHAIN: return pmh_dc_apply(dc, x, y, rho, nullptr);
    case PMH_PEN_ONE_LAUNCH:
    case PMH_PEN_TEN_LAUNCH: return mult_fused_dense(x, y, nullptr);
    case PMH_PEN_DENSE_INVERSE: return mult_dense_inverse(x, y);
    default: return mult_plain(x, y);
    }
  }
  // The vector phase in the product's last kernel, or PMH_EPI_UNSUPPORTED: the caller then runs the separate vector kernels behind the plain product.
  // (The chain leaves its block partials per 1024-entry tile for the HOST to sum: a caller that finalises on the device -- row-distributed scalars, e.hosted == NULL --
  // counts on one partial per workgroup of the streaming Vec kernels' grid.  The one-launch form gives exactly that where the grid is one row per thread.)
  int mult_epi(const double *x, double *y, const pmh_vec_epi &e) override
  {
    switch (form()) {
    case PMH_PEN_FOLD: return pmh_knobs().vec_epi ? fold_apply(x, y, &e) : PMH_EPI_UNSUPPORTED;
    case PMH_PEN_CHAIN: return !e.hosted ? PMH_EPI_UNSUPPORTED : (e.same_input ? pmh_dc_replay(dc, x, y, rho, &e, e.replayed) : pmh_dc_apply(dc, x, y, rho, &e));
    case PMH_PEN_ONE_LAUNCH:
      if (!pmh_knobs().vec_epi || n > PMH_MAX_VEC_BLOCKS * PMH_BLOCK || pmh_vec_grid(n) != (n + PMH_BLOCK - 1) / PMH_BLOCK) return PMH_EPI_UNSUPPORTED;
      return mult_fused_dense(x, y, &e);
    default: return PMH_EPI_UNSUPPORTED;
    }
  }
  ~PenalizedOp() override
  {
    pmh_dc_destroy(dc);
    pmh_free(ctx, t);
    if (xwork) pmh_free(ctx, xwork);
  }
  // only the chain has anything to gain from the caller's assertion (it keeps the intermediates that do not depend on rho)
  int mult_same_input(const double *x, double *y, int *replayed = nullptr) override
  {
    return form() == PMH_PEN_CHAIN ? pmh_dc_replay(dc, x, y, rho, nullptr, replayed) : mult(x, y);
  }
  // MatMultTranspose_Penalized matpenalized.c:26-36: y = BtB x; y *= rho; y = y + A' x
  int mult_transpose(const double *x, double *y) override
  {
    PMH_CHK(pmh_qppf_apply_GtG(pf, x, y));
    PMH_CHK(A->mult_transpose(x, t));
    PMH_CHK(pmh_vec_scale(ctx, n, y, rho));
    return pmh_vec_axpy(ctx, n, y, 1.0, t);
  }
  // MatMultAdd_Penalized / MatMultTransposeAdd_Penalized matpenalized.c:40-78: x2 != y: y = BtB x; y = rho y + x2;
  // x2 == y: xwork = BtB x; xwork *= rho; y += xwork.  Then y = y + A x (resp. A' x).
  int mult_add(const double *x, const double *x2, double *y, bool transpose)
  {
    if (x2 != y) {
      PMH_CHK(pmh_qppf_apply_GtG(pf, x, y));
      PMH_CHK(pmh_vec_aypx(ctx, n, y, rho, x2));
    } else {
      if (!xwork) PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)n, (void **)&xwork));
      PMH_CHK(pmh_qppf_apply_GtG(pf, x, xwork));
      PMH_CHK(pmh_vec_scale(ctx, n, xwork, rho));
      PMH_CHK(pmh_vec_axpy(ctx, n, y, 1.0, xwork));
    }
    PMH_CHK(transpose ? A->mult_transpose(x, t) : A->mult(x, t));
    return pmh_vec_axpy(ctx, n, y, 1.0, t);
  }
};

extern "C" int pmh_op_create_penalized(pmh_op A, pmh_qppf pf, double rho, pmh_op *op)
{
  PMH_ARG(A && pf && op && rho >= 0);
  PMH_ARG(A->n == pf->n);
  PenalizedOp *o = new PenalizedOp();
  o->ctx         = A->ctx;
  o->n           = A->n;
  o->A           = A;
  o->pf          = pf;
  o->rho         = rho;
  o->chain_allowed = pmh_knobs().chain;
  PMH_CHK(pmh_malloc(o->ctx, sizeof(double) * (size_t)o->n, (void **)&o->t));
  *op = o;
  return PMH_SUCCESS;
}

extern "C" int pmh_op_penalized_mult_add(pmh_op op, const double *x, const double *x2, double *y)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  PMH_ARG(o && x && x2 && y);
  return o->mult_add(x, x2, y, false);
}

extern "C" int pmh_op_penalized_mult_transpose_add(pmh_op op, const double *x, const double *x2, double *y)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  PMH_ARG(o && x && x2 && y);
  return o->mult_add(x, x2, y, true);
}

int pmh_op_penalized_arm_aux_normG(pmh_op op, const double *u, double *Gu, int slot)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  PMH_ARG(o && u && Gu && slot >= 0 && slot < PMH_NSCAL);
  o->aux_done = 0;
  if (o->fold()) { // the SVM operator's own pass serves it (one GPU; otherwise the request is dropped there and the caller's own launches follow)
    o->aux_u = u, o->aux_Gu = Gu, o->aux_slot = slot;
    return PMH_SUCCESS;
  }
  if (o->dc || !o->one_launch()) return PMH_SUCCESS; // not armed: the caller's own launches follow
  o->aux_u = u, o->aux_Gu = Gu, o->aux_slot = slot;
  return PMH_SUCCESS;
}

// SMALXE's ||B u|| from the chain: every emission of the iterate leaves T G0 u in Gu and its squared norm in the scalar slot (pmh_dc_set_norm_target);
// ready = the last such emission was for this very u and nothing has invalidated it since
int pmh_op_penalized_set_normG_target(pmh_op op, double *Gu, int slot)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  PMH_ARG(o && Gu && slot >= 0 && slot < PMH_NSCAL);
  o->norm_Gu = Gu, o->norm_slot = slot;
  if (o->dc) PMH_CHK(pmh_dc_set_norm_target(o->dc, Gu, slot));
  return PMH_SUCCESS;
}
int pmh_op_penalized_normG_ready(pmh_op op, const double *u)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  return (o && o->dc && pmh_dc_norm_ready(o->dc, u)) ? 1 : 0;
}
int pmh_op_penalized_chain_launches(pmh_op op)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  return (o && o->dc) ? pmh_dc_last_launches(o->dc) : -1;
}

extern "C" int pmh_op_penalized_test_emit(pmh_op op, int what, const double *x)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  PMH_ARG(o && (what == 0 || (what == 1 && x)));
  if (!o->chain()) return pmh_set_error(PMH_ERR_SUP, "pmh_op_penalized_test_emit: the operator does not run on the dual-space chain");
  if (what == 0) {
    o->emit_invalidate();
    return PMH_SUCCESS;
  }
  return pmh_dc_test_emit(o->dc, x);
}

extern "C" int pmh_op_penalized_test_mult_epi(pmh_op op, int kind, int same_input, const double *x, const double *b, const double *lb, double astol, double *y, double *gf, double *p, int cap,
                                              double *partials_host, double *psums_host, int *nblocks, int *nseg)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  PMH_ARG(o && x && y && (kind == 0 || kind == PMH_VEPI_GRAD_SPLIT));
  if (!o->chain()) return pmh_set_error(PMH_ERR_SUP, "pmh_op_penalized_test_mult_epi: the operator does not run on the dual-space chain");
  pmh_ctx ctx = o->ctx;
  if (kind == 0) {
    PMH_CHK(same_input ? o->mult_same_input(x, y) : o->mult(x, y));
    return pmh_sync(ctx);
  }
  PMH_ARG(b && gf && p && partials_host && psums_host && nblocks && nseg);
  pmh_vec_epi e;
  memset(&e, 0, sizeof(e));
  int hosted = 0, p_emitted = 0;
  e.kind = PMH_VEPI_GRAD_SPLIT, e.b = b, e.lb = lb, e.astol = astol, e.gf = gf, e.p = p, e.partials = ctx->d_partials, e.ld = ctx->partials_cap, e.prow = 0;
  e.hosted = &hosted, e.emitted_p = &p_emitted, e.same_input = same_input;
  PMH_CHK(o->mult_epi(x, y, e));
  PMH_CHK(pmh_sync(ctx));
  if (!hosted || !p_emitted || hosted > cap) return pmh_set_error(PMH_ERR_STATE, "pmh_op_penalized_test_mult_epi: %d blocks of partials (room for %d), direction emitted: %d", hosted, cap, p_emitted);
  for (int k = 0; k < 4; k++) memcpy(partials_host + (size_t)k * hosted, ctx->h_partials + (size_t)k * ctx->partials_cap, sizeof(double) * (size_t)hosted);
  *nblocks = hosted;
  return pmh_dc_test_direction_sums(o->dc, cap, psums_host, nseg);
}

// the sibling with every operand of the two epilogues, the caller's in_slot and the block partials of both copies (include/permon_hip.h)
extern "C" int pmh_op_penalized_test_mult_epi2(pmh_op op, int kind, int same_input, int in_slot, const double *x, const double *b, const double *g, const double *xx, const double *lb,
                                               const double *ub, double astol, double *y, double *gf, double *p, double *partials_dev_host, double *partials_pinned_host, int *nblocks,
                                               int *replayed)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  PMH_ARG(o && x && y && (kind == 0 || kind == PMH_VEPI_P1 || kind == PMH_VEPI_GRAD_SPLIT) && in_slot >= 0 && in_slot <= 2 && partials_dev_host && partials_pinned_host && nblocks && replayed);
  PMH_ARG(kind != PMH_VEPI_P1 || (g && xx));
  PMH_ARG(kind != PMH_VEPI_GRAD_SPLIT || (b && gf && p));
  PMH_ARG(kind != 0 || in_slot == 0); // (a plain product always forms its own sums)
  const bool chained = o->chain() != nullptr;
  if (!chained && (in_slot || same_input)) return pmh_set_error(PMH_ERR_SUP, "pmh_op_penalized_test_mult_epi2: the operator does not run on the dual-space chain");
  pmh_ctx      ctx    = o->ctx;
  const size_t pbytes = sizeof(double) * PMH_MAX_RED * (size_t)ctx->partials_cap;
  PMH_CHK(pmh_sync(ctx));
  PMH_CHK(pmh_memcpy_h2d(ctx, ctx->d_partials, partials_dev_host, pbytes));
  memcpy(ctx->h_partials, partials_pinned_host, pbytes);
  *nblocks = 0, *replayed = 0;
  if (kind == 0) {
    PMH_CHK(same_input ? o->mult_same_input(x, y, replayed) : o->mult(x, y));
  } else {
    pmh_vec_epi e;
    memset(&e, 0, sizeof(e));
    int hosted = 0, p_emitted = 0;
    e.kind = kind, e.b = b, e.g = g, e.xx = xx, e.lb = lb, e.ub = ub, e.astol = astol, e.gf = gf, e.p = p, e.partials = ctx->d_partials, e.ld = ctx->partials_cap;
    e.prow = kind == PMH_VEPI_P1 ? 4 : 0; // as f_apply_p1 / f_gradient_split (mpgp.hip) place them
    if (chained) {
      e.hosted = &hosted, e.emitted_p = &p_emitted, e.same_input = same_input, e.in_slot = in_slot, e.replayed = replayed;
      PMH_CHK(o->mult_epi(x, y, e));
      *nblocks = hosted;
    } else { // device rows only, one partial per workgroup of the streaming grid
      const int rc = o->mult_epi(x, y, e);
      if (rc == PMH_EPI_UNSUPPORTED) return pmh_set_error(PMH_ERR_SUP, "pmh_op_penalized_test_mult_epi2: the operator's product has no vector epilogue as it is configured");
      PMH_CHK(rc);
      *nblocks = pmh_vec_grid(o->n);
    }
  }
  PMH_CHK(pmh_sync(ctx));
  PMH_CHK(pmh_memcpy_d2h(ctx, partials_dev_host, ctx->d_partials, pbytes));
  memcpy(partials_pinned_host, ctx->h_partials, pbytes);
  return PMH_SUCCESS;
}

extern "C" int pmh_op_penalized_test_form(pmh_op op, int *form)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  PMH_ARG(o && form);
  *form = o->form();
  return PMH_SUCCESS;
}

// ||G u||^2 as SMALXE asks for it: armed = 0, the two launches of pmh_qppf_apply_G_norm2; armed = 1, the request riding on the product y = A x (include/permon_hip.h)
extern "C" int pmh_op_penalized_test_aux_normG(pmh_op op, int armed, const double *u, double *Gu, int slot, const double *x, double *y, double scal[2], int *served)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  PMH_ARG(o && u && Gu && slot >= 0 && slot < PMH_NSCAL && scal && served && (!armed || (x && y)));
  pmh_ctx ctx = o->ctx;
  PMH_CHK(pmh_sync(ctx));
  PMH_CHK(pmh_memcpy_h2d(ctx, ctx->d_scal + slot, &scal[0], sizeof(double)));
  ctx->h_scal[slot] = scal[1];
  *served           = 0;
  if (armed) {
    PMH_CHK(pmh_op_penalized_arm_aux_normG(op, u, Gu, slot));
    PMH_CHK(o->mult(x, y));
    *served = pmh_op_penalized_take_aux_done(op);
  } else {
    PMH_CHK(pmh_qppf_apply_G_norm2(o->pf, u, Gu, slot));
  }
  PMH_CHK(pmh_sync(ctx));
  PMH_CHK(pmh_memcpy_d2h(ctx, &scal[0], ctx->d_scal + slot, sizeof(double)));
  scal[1] = ctx->h_scal[slot];
  return PMH_SUCCESS;
}

extern "C" int pmh_op_penalized_test_chain_info(pmh_op op, long long info[10])
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  PMH_ARG(o && info);
  if (!o->chain()) return pmh_set_error(PMH_ERR_SUP, "pmh_op_penalized_test_chain_info: the operator does not run on the dual-space chain");
  return pmh_dc_test_info(o->dc, info);
}

extern "C" int pmh_op_penalized_test_chain_read(pmh_op op, int what, int cap, double *host, int *len)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  PMH_ARG(o);
  if (!o->chain()) return pmh_set_error(PMH_ERR_SUP, "pmh_op_penalized_test_chain_read: the operator does not run on the dual-space chain");
  return pmh_dc_test_read(o->dc, what, cap, host, len);
}

// SMALXE's norm target as smalxe.hip sets it; ready: pmh_op_penalized_normG_ready (which launches k_dc_norm where the sums wait and no application followed)
extern "C" int pmh_op_penalized_test_norm_target(pmh_op op, double *Gu, int slot, const double *u, int *ready)
{
  PMH_ARG(op && ((Gu && !u) || (u && ready)));
  if (Gu) return pmh_op_penalized_set_normG_target(op, Gu, slot);
  *ready = pmh_op_penalized_normG_ready(op, u);
  return pmh_sync(op->ctx);
}

int pmh_op_penalized_take_aux_done(pmh_op op)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  if (!o) return 0;
  const int d = o->aux_done;
  o->aux_done = 0, o->aux_u = nullptr;
  return d;
}

extern "C" int pmh_op_penalized_set_penalty(pmh_op op, double rho)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  PMH_ARG(o && rho >= 0);
  o->rho = rho;
  return PMH_SUCCESS;
}

extern "C" int pmh_op_penalized_get_penalty(pmh_op op, double *rho)
{
  PenalizedOp *o = dynamic_cast<PenalizedOp *>(op);
  PMH_ARG(o && rho);
  *rho = o->rho;
  return PMH_SUCCESS;
}

extern "C" int pmh_op_create_projected(pmh_op A, pmh_qppf pf, int symmetric, pmh_op *op)
{
  PMH_ARG(A && pf && op);
  PMH_ARG(A->n == pf->n);
  ProjectedOp *o = new ProjectedOp();
  o->ctx         = A->ctx;
  o->n           = A->n;
  o->A           = A;
  o->pf          = pf;
  o->symmetric   = symmetric ? 1 : 0;
  PMH_CHK(pmh_malloc(o->ctx, sizeof(double) * (size_t)o->n, (void **)&o->w1));
  PMH_CHK(pmh_malloc(o->ctx, sizeof(double) * (size_t)o->n, (void **)&o->w2));
  *op = o;
  return PMH_SUCCESS;
}
