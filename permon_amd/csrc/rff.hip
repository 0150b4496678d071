// Random Fourier features (Rahimi and Recht): Z[i, k] = s cos(sum_j X[i, j] Omega[j, k] + beta[k]), so that z(x) . z(x') ~ k(x, x') for the shift-invariant kernel
// whose spectral density the columns of Omega were drawn from.  A linear SVM / SVR on Z (n x D row-major, the layout pmh_svm_create takes) is then an
// approximate kernel machine; nothing in a solver, an operator or a scoring kernel knows about it.  The library draws nothing: Omega, beta and s are the caller's.
//
// One kernel, k_rff<TX, TZ, EPI, NG> (rff_kernel.h: the kernel block of the Nystroem map, nys.hip, is the same kernel under other functors; k_rff_dots of
// rff_score.hip shares its product phase and scores on the features without storing them): TX / TZ the types X is read in and Z is written in (double or float: a
// float enters the arithmetic as (double)x, a result is rounded once, at the store; all arithmetic is fp64), EPI what happens in registers to a product
// t = x . omega_k, a value of the row and the column's value beta_k, which sits in LDS beside Omega (rff_cos: s cos(t + beta_k); rff_arg: t + beta_k itself, for
// pmh_rff_test_args; neither takes a value of the row).  There is no n x D array of arguments.
//
// The product runs on v_mfma_f64_16x16x4_f64 (A[m = l & 15][k = l >> 4], B[k = l >> 4][n = l & 15], D column l & 15, rows (l >> 4) + 4 r).  A workgroup of
// RFF_WAVES waves takes RFF_RW = 16 RFF_WAVES rows at a time, a wave 16 of them over a column tile of RFF_CT = 256 columns (16 instruction tiles: 64 accumulator
// doubles per lane), grid.y the column tiles (D <= 256: one, and X is streamed once).  Omega is staged in LDS in k-blocks of RFF_KB = 64 rows and shared by the
// waves; with d <= RFF_KB it is staged ONCE per workgroup, which then walks its row blocks (grid.x <= the CUs), else once per row block and k-block (from L2).
// Which k and which column an operand slot stands for is the kernel's choice, as long as A and B agree:
//   k    lane (row l & 15, g = l >> 4) loads the 4 CONSECUTIVE entries X[row][k0 + 16 t + 4 g + e], e = 0..3, in one 32-byte (float: 16-byte) load per t; the
//        instruction (t, e) multiplies them with rows k0 + 16 t + 4 g + e of Omega.  A row's sum therefore runs over j in the order k-block, t, e, and inside one
//        instruction over g as the hardware adds its 4 products: fixed by d alone -- not by n, the row's position, the grid or which load instruction was used.
//   col  instruction tile j, lane column c holds column 64 (j >> 2) + 4 c + (j & 3) of the column tile: a lane ends with 4 ADJACENT columns per row in tiles
//        4 q .. 4 q + 3 and stores them as one 32-byte (float: 16-byte) store.  Omega's LDS image is permuted accordingly (position 16 j + c), so the operand
//        reads stay contiguous; its row stride RFF_LDW = 260 doubles puts the rows 4 g + e, g = 0..3, a lane quartet reads 32 banks apart.
// NG, the groups of 64 columns a wave multiplies (4 NG instruction tiles), is a template argument: the whole column tiles of D run the NG = 4 instance in one launch,
// the last, narrower tile the instance that covers it in a launch of its own (D = 40: NG = 1; D = 257: NG = 4 over 256 columns, then NG = 1 over the last one), so
// products of zeros stay below 64 columns' worth (columns >= D inside a group are zeros in LDS).  The k-block's steps of 16 are a loop that is not unrolled, X
// loaded one step ahead.  Tiles or steps under run-time conditions instead cost, through the accumulators' merges, the registers the cosines need (256 VGPRs and
// 12 bytes of scratch against 211 and none).
// Rows >= n, k >= d and columns >= D are ZEROS in the operands (selected, never loaded): nothing beside the arrays is read, and since output row i takes only A's
// row i, a NaN in one sample stays in that sample's features.  No atomics, one fixed order: two calls give the same bits.
// The epilogue walks the 4 groups of 64 columns in a loop that is NOT unrolled -- the accumulators are rotated by 4 tiles per trip, 96 register moves beside 16
// cosines -- so the kernel holds 16 copies of the cosine, not 64.
// Bytes: n d size_x read + n D size_z written (+ d D 8 of Omega per workgroup, from L2); flops 2 n d D on the matrix cores + n D cosines on the vector ALU.
#include "pmh_internal.h"

#include "rff_kernel.h"
#include "svm_front.h"

// how many entries are not finite (a count: any order gives the same integer)
__global__ __launch_bounds__(PMH_BLOCK) void k_rff_bad(long long m, const double *__restrict__ a, int *__restrict__ bad)
{
  int b = 0;
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < m; i += (long long)gridDim.x * PMH_BLOCK) b += isfinite(a[i]) ? 0 : 1;
  if (b) atomicAdd(bad, b);
}

int rff_count_not_finite(pmh_ctx ctx, const char *who, const char *what, long long m, const double *a_dev, long long *nbad)
{
  return sv_count_bad(ctx, who, what, [&](int *cnt) { hipLaunchKernelGGL(k_rff_bad, dim3(pmh_vec_grid((int)(m < (1 << 30) ? m : (1 << 30)))), dim3(PMH_BLOCK), 0, ctx->stream, m, a_dev, cnt); }, nbad);
}

static rff_operands rff_operands_of(pmh_rff f) { return {f->ctx, f->d, f->D, f->omega, f->beta}; }

int rff_identity_apply(pmh_rff f, long long n, const double *X_dev, void *Z_dev, int z_type)
{
  const rff_operands o = rff_operands_of(f);
  return z_type == PMH_F64 ? rff_launch<double, double>(o, n, X_dev, Z_dev, rff_arg{}) : rff_launch<double, float>(o, n, X_dev, Z_dev, rff_arg{});
}

extern "C" int pmh_rff_create(pmh_ctx ctx, int d, int D, const double *omega_dev, const double *beta_dev, double scale, pmh_rff *out)
{
  PMH_ARG(ctx && out);
  *out = nullptr;
  if (d < 1 || D < 1) return pmh_set_error(PMH_ERR_ARG, "pmh_rff_create: d = %d, D = %d, both must be at least 1", d, D);
  if (!omega_dev) return pmh_set_error(PMH_ERR_ARG, "pmh_rff_create: omega_dev is NULL");
  if (!std::isfinite(scale)) return pmh_set_error(PMH_ERR_ARG, "pmh_rff_create: scale = %g, must be finite", scale);
  const long long m = (long long)d * D;
  pmh_rff         f = new pmh_rff_s();
  f->ctx = ctx, f->d = d, f->D = D, f->scale = scale, f->omega = nullptr, f->beta = nullptr;
  int       rc = PMH_SUCCESS;
  long long bad_o = 0, bad_b = 0;
  do {
    if ((rc = pmh_malloc(ctx, sizeof(double) * (size_t)m, (void **)&f->omega)) || (rc = pmh_malloc(ctx, sizeof(double) * (size_t)D, (void **)&f->beta))) break;
    if ((rc = pmh_memcpy_d2d(ctx, f->omega, omega_dev, sizeof(double) * (size_t)m))) break;
    if ((rc = beta_dev ? pmh_memcpy_d2d(ctx, f->beta, beta_dev, sizeof(double) * (size_t)D) : pmh_memset(ctx, f->beta, 0, sizeof(double) * (size_t)D))) break;
    if ((rc = rff_count_not_finite(ctx, "pmh_rff_create", "entries of omega", m, f->omega, &bad_o))) break;
    if ((rc = rff_count_not_finite(ctx, "pmh_rff_create", "entries of beta", D, f->beta, &bad_b))) break;
    if (bad_o || bad_b) rc = pmh_set_error(PMH_ERR_ARG, "pmh_rff_create: %lld of the entries of omega and %lld of beta are not finite", bad_o, bad_b);
  } while (0);
  if (rc) {
    pmh_rff_destroy(f);
    return rc;
  }
  *out = f;
  return PMH_SUCCESS;
}

extern "C" int pmh_rff_destroy(pmh_rff f)
{
  if (!f) return PMH_SUCCESS;
  if (f->omega) pmh_free(f->ctx, f->omega);
  if (f->beta) pmh_free(f->ctx, f->beta);
  delete f;
  return PMH_SUCCESS;
}

extern "C" int pmh_rff_apply(pmh_rff f, long long n, const void *X_dev, int x_type, void *Z_dev, int z_type)
{
  PMH_ARG(f);
  PMH_CHK(rff_check_entry("pmh_rff_apply", n, x_type, &z_type, X_dev && Z_dev, "X_dev or Z_dev"));
  if (n == 0) return PMH_SUCCESS;
  const rff_operands o = rff_operands_of(f);
  const rff_cos      epi{f->scale};
  if (x_type == PMH_F64) return z_type == PMH_F64 ? rff_launch<double, double>(o, n, X_dev, Z_dev, epi) : rff_launch<double, float>(o, n, X_dev, Z_dev, epi);
  return z_type == PMH_F64 ? rff_launch<float, double>(o, n, X_dev, Z_dev, epi) : rff_launch<float, float>(o, n, X_dev, Z_dev, epi);
}

extern "C" int pmh_rff_test_args(pmh_rff f, long long n, const void *X_dev, int x_type, double *T_dev)
{
  PMH_ARG(f);
  PMH_CHK(rff_check_entry("pmh_rff_test_args", n, x_type, nullptr, X_dev && T_dev, "X_dev or T_dev"));
  if (n == 0) return PMH_SUCCESS;
  const rff_operands o = rff_operands_of(f);
  return x_type == PMH_F64 ? rff_launch<double, double>(o, n, X_dev, T_dev, rff_arg{}) : rff_launch<float, double>(o, n, X_dev, T_dev, rff_arg{});
}

extern "C" int pmh_rff_get(pmh_rff f, int *d, int *D, double *omega_host, double *beta_host, double *scale)
{
  PMH_ARG(f);
  if (d) *d = f->d;
  if (D) *D = f->D;
  if (scale) *scale = f->scale;
  if (omega_host) PMH_CHK(pmh_memcpy_d2h(f->ctx, omega_host, f->omega, sizeof(double) * (size_t)f->d * f->D));
  if (beta_host) PMH_CHK(pmh_memcpy_d2h(f->ctx, beta_host, f->beta, sizeof(double) * (size_t)f->D));
  return PMH_SUCCESS;
}

extern "C" int pmh_rff_info(pmh_rff f, int info[8])
{
  PMH_ARG(f && info);
  info[0] = RFF_RW, info[1] = 16, info[2] = RFF_CT, info[3] = RFF_KB, info[4] = RFF_LDS_BYTES, info[5] = RFF_WAVES, info[6] = RFF_KC, info[7] = RFF_DOTS_LDS_BYTES;
  return PMH_SUCCESS;
}
