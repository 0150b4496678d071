// Nystroem features (Williams and Seeger): z(x) = M' k(L, x) with landmarks L (m x d) taken from the data and M = U_r Lambda_r^{-1/2} from k(L, L) = U Lambda U',
// so that z(x) . z(x') = k(x, L) k(L, L)^+ k(L, x') ~ k(x, x') for any kernel that is a function of x . l, |x|^2 and |l|^2: here
//   poly  k(x, l) = (gamma x . l + coef0)^degree        rbf  k(x, l) = exp(-gamma |x - l|^2)
// A linear SVM / SVR on Z (n x D row-major) is then an approximate kernel machine, as with the random Fourier features of rff.hip, and nothing in a solver, an
// operator or a scoring kernel knows about it.  The library computes no eigen-decomposition and draws nothing: L and M are the caller's.
//
// Two stages per chunk of rows:
//   A  k_rff<TX, double, EPI, NG> (rff_kernel.h), the kernel of the random Fourier features under this map's functors: C = k(X, L) (rows x m, fp64), with
//      Omega := L' (d x m, transposed once at create) and |l|^2 where that map has beta: v_mfma_f64_16x16x4_f64, RFF_WAVES waves of 16 rows, a column tile of
//      RFF_CT landmarks, k-blocks of RFF_KB in LDS; the layouts and the order of a row's sum are described in rff.hip.  The functor EPI (nys_internal.h) runs on the
//      accumulators: lane (c, g), register r, tile jm of group q is row g + 4 r, column 64 q + 4 c + jm.
//        poly  b = gamma t + coef0 (two roundings), then v = b multiplied by b another degree - 1 times, left to right.  It takes no value of a row or a column:
//              nothing is staged and nothing loaded for it
//        rbf   q = max((nx_i + nl_j) - 2 t, 0), k = exp(-(gamma q)).  nl_j = |l_j|^2, the launch's column vector, is computed once at create and sits in LDS at
//              rff_pos positions; nx_i = |x_i|^2, the functor's row value, comes from k_nys_norms over the chunk (it reads the chunk of X a first time; k_rff then
//              reads it from cache), one double per row, and a lane reads the 4 values of its rows g + 4 r
//        nys_t, nys_q  the identities of pmh_nys_test_args
//      NG as for the Fourier features: rff_tile_launches chooses the instances.
//   B  Z = C M: k_rff<double, TZ, rff_arg, NG> of rff.hip on (m, D, M, beta = 0) through rff_identity_apply -- the kernel tests/test_gpu_rff.py pins.
// One walk, nys_walk, takes X in chunks of chunk_rows rows.  pmh_nys_apply: norms (rbf), stage A into the handle's workspace of chunk_rows x m doubles, stage B
// from the workspace into Z, so that C never exists as an n x m array in HBM and a chunk of it can be read back from the Infinity Cache.  pmh_nys_kernel and
// pmh_nys_test_args: stage A straight into the caller's array.
//
// The contract:
//   - no atomics (the count of non-finite entries at create apart: an integer, the same in any order);
//   - a row's results depend on d, m, D and the row alone: k_nys_norms sums a row in an order fixed by d, the product phase in an order fixed by d (stage A) and m
//     (stage B).  A sample has the same bits alone and in any batch, whatever the chunk size, and across two calls;
//   - a float32 X enters as (double)x: the bits of its widened copy; a float32 Z is the fp64 Z rounded once, at the store;
//   - rows >= n, k >= d and landmarks >= m are ZEROS in the operands (selected, never loaded), nx of a row >= n is not loaded: nothing beside the arrays is read;
//   - output row i takes only row i of X and nx_i: a NaN in one sample stays in that sample;
//   - q >= 0, so rbf values are at most 1;
//   - |x - l|^2 is formed from norms and a product, as the matrix cores require: a sample that is itself a landmark gets q of the order of u d |x|^2, not 0.
// Bytes: n d size_x read (twice for rbf, the second time from cache) + n D size_z written (+ the chunk of C through the cache); flops 2 n (d m + m D) on the
// matrix cores + n m exponentials or degree - 1 products on the vector ALU.
#include <climits>

#include "pmh_internal.h"

#include "nys_internal.h"

// nx[i] = sum_j X[i][j]^2, 16 lanes per row: lane e sums the products of j = e, e + 16, ... in that order, then the 16 sums meet in a butterfly (8, 4, 2, 1 apart):
// an order fixed by d alone
template <class TX> __global__ __launch_bounds__(PMH_BLOCK) void k_nys_norms(long long n, int d, const TX *__restrict__ X, double *__restrict__ nx)
{
  const int e = threadIdx.x & 15;
  for (long long i = ((long long)blockIdx.x * PMH_BLOCK + threadIdx.x) >> 4; i < n; i += ((long long)gridDim.x * PMH_BLOCK) >> 4) { // (the 16 lanes of a row share i: they leave together)
    const TX *xr = X + (size_t)i * d;
    double    s  = 0.0;
    for (int j = e; j < d; j += 16) {
      const double x = (double)xr[j];
      s = s + x * x;
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) s = s + __shfl_xor(s, o, 16);
    if (e == 0) nx[i] = s;
  }
}

// Lt (d x m) = L' (m x d)
__global__ __launch_bounds__(PMH_BLOCK) void k_nys_transpose(int m, int d, const double *__restrict__ L, double *__restrict__ Lt)
{
  const long long tot = (long long)m * d;
  for (long long p = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; p < tot; p += (long long)gridDim.x * PMH_BLOCK) Lt[p] = L[(p % m) * d + p / m];
}

template <class TX> static int nys_norms(pmh_ctx ctx, long long n, int d, const void *X, double *nx)
{
  const long long threads = 16 * n;
  hipLaunchKernelGGL(k_nys_norms<TX>, dim3(pmh_vec_grid((int)(threads < (1 << 30) ? threads : (1 << 30)))), dim3(PMH_BLOCK), 0, ctx->stream, n, d, (const TX *)X, nx);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

// stage A of at most chunk_rows rows: the norms where the epilogue takes them, then k_rff<TX, double, EPI, NG> on (m, L', |l|^2) over the m landmarks
template <class TX, class EPI> static int nys_stage_a(pmh_nys f, long long n, const void *X, double *C, EPI epi)
{
  if (EPI::rows) PMH_CHK(nys_norms<TX>(f->ctx, n, f->d, X, f->nx));
  return rff_launch<TX, double>(rff_operands{f->ctx, f->d, f->m, f->lt, f->nl}, n, X, C, epi);
}
template <class EPI> static int nys_stage_a(pmh_nys f, long long n, const void *X, int x_type, double *C, EPI epi)
{
  return x_type == PMH_F64 ? nys_stage_a<double>(f, n, X, C, epi) : nys_stage_a<float>(f, n, X, C, epi);
}
// what: -1 the map's kernel, 0 t, 1 q
static int nys_stage_a(pmh_nys f, long long n, const void *X, int x_type, double *C, int what)
{
  if (what == 0) return nys_stage_a(f, n, X, x_type, C, nys_t{});
  if (what == 1) return nys_stage_a(f, n, X, x_type, C, nys_q{f->nx});
  if (f->kernel == PMH_NYS_RBF) return nys_stage_a(f, n, X, x_type, C, nys_rbf{f->gamma, f->nx});
  return nys_stage_a(f, n, X, x_type, C, nys_poly{f->gamma, f->coef0, f->degree});
}

// The walk over all n rows, chunk by chunk (the norms live in the handle's chunk_rows doubles).  Z == nullptr: stage A straight into C (n x m).  Else stage A into
// the handle's workspace and stage B from there into the chunk's rows of Z (n x D of z_type)
static int nys_walk(pmh_nys f, long long n, const void *X, int x_type, int what, double *C, void *Z, int z_type)
{
  const size_t sx = x_type == PMH_F64 ? sizeof(double) : sizeof(float), sz = z_type == PMH_F64 ? sizeof(double) : sizeof(float);
  for (long long i0 = 0; i0 < n; i0 += f->chunk_rows) {
    const long long nc = n - i0 < f->chunk_rows ? n - i0 : f->chunk_rows;
    PMH_CHK(nys_stage_a(f, nc, (const char *)X + (size_t)i0 * f->d * sx, x_type, Z ? f->work : C + (size_t)i0 * f->m, what));
    if (Z) PMH_CHK(rff_identity_apply(f->stage_b, nc, f->work, (char *)Z + (size_t)i0 * f->D * sz, z_type));
  }
  return PMH_SUCCESS;
}

static void nys_free_chunk(pmh_nys f)
{
  if (f->work) pmh_free(f->ctx, f->work);
  if (f->nx) pmh_free(f->ctx, f->nx);
  f->work = f->nx = nullptr;
}
static int nys_alloc_chunk(pmh_nys f, long long rows)
{
  nys_free_chunk(f);
  f->chunk_rows = rows;
  PMH_CHK(pmh_malloc(f->ctx, sizeof(double) * (size_t)rows * f->m, (void **)&f->work));
  return pmh_malloc(f->ctx, sizeof(double) * (size_t)rows, (void **)&f->nx);
}

extern "C" int pmh_nys_create(pmh_ctx ctx, int d, int m, int D, const double *landmarks_dev, int kernel, double gamma, double coef0, int degree, const double *M_dev, pmh_nys *out)
{
  PMH_ARG(ctx && out);
  *out = nullptr;
  if (d < 1 || m < 1 || D < 1 || D > m) return pmh_set_error(PMH_ERR_ARG, "pmh_nys_create: d = %d, m = %d, D = %d: all must be at least 1 and D at most m", d, m, D);
  if (kernel != PMH_NYS_RBF && kernel != PMH_NYS_POLY) return pmh_set_error(PMH_ERR_ARG, "pmh_nys_create: kernel = %d, must be PMH_NYS_RBF (0) or PMH_NYS_POLY (1)", kernel);
  if (!(gamma > 0.0) || !std::isfinite(gamma)) return pmh_set_error(PMH_ERR_ARG, "pmh_nys_create: gamma = %g, must be positive and finite", gamma);
  if (!std::isfinite(coef0)) return pmh_set_error(PMH_ERR_ARG, "pmh_nys_create: coef0 = %g, must be finite", coef0);
  if (degree < 1 || degree > NYS_MAX_DEGREE) return pmh_set_error(PMH_ERR_ARG, "pmh_nys_create: degree = %d, must be 1 .. %d", degree, NYS_MAX_DEGREE);
  if (!landmarks_dev || !M_dev) return pmh_set_error(PMH_ERR_ARG, "pmh_nys_create: landmarks_dev or M_dev is NULL");
  const long long md = (long long)m * d;
  pmh_nys         f  = new pmh_nys_s();
  f->ctx = ctx, f->d = d, f->m = m, f->D = D, f->kernel = kernel, f->degree = degree, f->gamma = gamma, f->coef0 = coef0;
  f->land = f->lt = f->nl = f->work = f->nx = nullptr, f->stage_b = nullptr, f->chunk_rows = 0;
  int       rc = PMH_SUCCESS;
  long long bad_l = 0, bad_m = 0;
  do {
    if ((rc = rff_count_not_finite(ctx, "pmh_nys_create", "entries of the landmarks", md, landmarks_dev, &bad_l))) break;
    if ((rc = rff_count_not_finite(ctx, "pmh_nys_create", "entries of M", (long long)m * D, M_dev, &bad_m))) break;
    if (bad_l || bad_m) {
      rc = pmh_set_error(PMH_ERR_ARG, "pmh_nys_create: %lld of the entries of the landmarks and %lld of M are not finite", bad_l, bad_m);
      break;
    }
    if ((rc = pmh_malloc(ctx, sizeof(double) * (size_t)md, (void **)&f->land)) || (rc = pmh_malloc(ctx, sizeof(double) * (size_t)md, (void **)&f->lt)) ||
        (rc = pmh_malloc(ctx, sizeof(double) * (size_t)m, (void **)&f->nl)))
      break;
    if ((rc = pmh_memcpy_d2d(ctx, f->land, landmarks_dev, sizeof(double) * (size_t)md))) break;
    hipLaunchKernelGGL(k_nys_transpose, dim3(pmh_vec_grid((int)(md < (1 << 30) ? md : (1 << 30)))), dim3(PMH_BLOCK), 0, ctx->stream, m, d, (const double *)f->land, f->lt);
    if (hipGetLastError() != hipSuccess) {
      rc = pmh_set_error(PMH_ERR_HIP, "pmh_nys_create: the launch that transposes the landmarks failed");
      break;
    }
    if ((rc = nys_norms<double>(ctx, m, d, f->land, f->nl))) break;
    if ((rc = pmh_rff_create(ctx, m, D, M_dev, nullptr, 1.0, &f->stage_b))) break;
    rc = nys_alloc_chunk(f, NYS_CHUNK_ROWS);
  } while (0);
  if (rc) {
    pmh_nys_destroy(f);
    return rc;
  }
  *out = f;
  return PMH_SUCCESS;
}

extern "C" int pmh_nys_destroy(pmh_nys f)
{
  if (!f) return PMH_SUCCESS;
  nys_free_chunk(f);
  if (f->stage_b) pmh_rff_destroy(f->stage_b);
  if (f->land) pmh_free(f->ctx, f->land);
  if (f->lt) pmh_free(f->ctx, f->lt);
  if (f->nl) pmh_free(f->ctx, f->nl);
  delete f;
  return PMH_SUCCESS;
}

extern "C" int pmh_nys_kernel(pmh_nys f, long long n, const void *X_dev, int x_type, double *C_dev)
{
  PMH_ARG(f);
  PMH_CHK(rff_check_entry("pmh_nys_kernel", n, x_type, nullptr, X_dev && C_dev, "X_dev or C_dev"));
  return nys_walk(f, n, X_dev, x_type, -1, C_dev, nullptr, PMH_F64);
}

extern "C" int pmh_nys_apply(pmh_nys f, long long n, const void *X_dev, int x_type, void *Z_dev, int z_type)
{
  PMH_ARG(f);
  PMH_CHK(rff_check_entry("pmh_nys_apply", n, x_type, &z_type, X_dev && Z_dev, "X_dev or Z_dev"));
  return nys_walk(f, n, X_dev, x_type, -1, nullptr, Z_dev, z_type);
}

extern "C" int pmh_nys_test_args(pmh_nys f, long long n, const void *X_dev, int x_type, int what, double *T_dev)
{
  PMH_ARG(f);
  PMH_CHK(rff_check_entry("pmh_nys_test_args", n, x_type, nullptr, X_dev && T_dev, "X_dev or T_dev", [&] {
    if (what != 0 && what != 1) return pmh_set_error(PMH_ERR_ARG, "pmh_nys_test_args: what = %d, must be 0 (t = x . l) or 1 (q = |x - l|^2)", what);
    if (what == 1 && f->kernel != PMH_NYS_RBF) return pmh_set_error(PMH_ERR_ARG, "pmh_nys_test_args: what = 1 (q = |x - l|^2) on a map whose kernel is not PMH_NYS_RBF");
    return (int)PMH_SUCCESS;
  }));
  return nys_walk(f, n, X_dev, x_type, what, T_dev, nullptr, PMH_F64);
}

extern "C" int pmh_nys_get(pmh_nys f, int *d, int *m, int *D, int *kernel, double *gamma, double *coef0, int *degree, double *landmarks_host, double *M_host)
{
  PMH_ARG(f);
  if (d) *d = f->d;
  if (m) *m = f->m;
  if (D) *D = f->D;
  if (kernel) *kernel = f->kernel;
  if (gamma) *gamma = f->gamma;
  if (coef0) *coef0 = f->coef0;
  if (degree) *degree = f->degree;
  if (landmarks_host) PMH_CHK(pmh_memcpy_d2h(f->ctx, landmarks_host, f->land, sizeof(double) * (size_t)f->m * f->d));
  if (M_host) PMH_CHK(pmh_rff_get(f->stage_b, nullptr, nullptr, M_host, nullptr, nullptr));
  return PMH_SUCCESS;
}

extern "C" int pmh_nys_info(pmh_nys f, int info[8])
{
  PMH_ARG(f && info);
  const long long wb = (long long)sizeof(double) * f->chunk_rows * f->m;
  info[0] = RFF_RW, info[1] = 16, info[2] = RFF_CT, info[3] = RFF_KB, info[4] = RFF_LDS_BYTES, info[5] = RFF_WAVES, info[6] = (int)f->chunk_rows, info[7] = wb < INT_MAX ? (int)wb : INT_MAX;
  return PMH_SUCCESS;
}

extern "C" int pmh_nys_set_chunk_rows(pmh_nys f, long long rows)
{
  PMH_ARG(f);
  if (rows < RFF_RW || rows % RFF_RW || rows > INT_MAX - RFF_RW)
    return pmh_set_error(PMH_ERR_ARG, "pmh_nys_set_chunk_rows: rows = %lld, must be a positive multiple of the %d rows of a workgroup (and below 2^31)", rows, RFF_RW);
  if (rows == f->chunk_rows) return PMH_SUCCESS;
  const long long old = f->chunk_rows; // (pmh_free waits for the stream: an enqueued call has finished with the workspace)
  const int       rc  = nys_alloc_chunk(f, rows);
  if (rc) {
    const int rc2 = nys_alloc_chunk(f, old);
    return rc2 ? rc2 : rc;
  }
  return PMH_SUCCESS;
}
