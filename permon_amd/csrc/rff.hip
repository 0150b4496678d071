// Random Fourier features (Rahimi and Recht): Z[i, k] = s cos(sum_j X[i, j] Omega[j, k] + beta[k]), so that z(x) . z(x') ~ k(x, x') for the shift-invariant kernel
// whose spectral density the columns of Omega were drawn from.  A linear SVM / SVR on Z (n x D row-major, the layout pmh_svm_create takes) is then an
// approximate kernel machine; nothing in a solver, an operator or a scoring kernel knows about it.  The library draws nothing: Omega, beta and s are the caller's.
//
// One kernel here, k_rff<TX, TZ, EPI, NG> (k_rff_dots of rff_score.hip shares its product phase and scores on the features without storing them): TX / TZ the types X is read in and Z is written in (double or float: a float enters the arithmetic as (double)x, a result is
// rounded once, at the store; all arithmetic is fp64), EPI what happens to an argument t = x . omega_k + beta_k in registers (rff_cos: s cos(t); rff_arg: t
// itself, for pmh_rff_test_args).  There is no n x D array of arguments.
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

#include "rff_internal.h"
#include "svm_front.h"

static __device__ __forceinline__ void rff_store4(double *z, const double v[4]) { *(rff_d4 *)z = rff_d4{v[0], v[1], v[2], v[3]}; }
static __device__ __forceinline__ void rff_store4(float *z, const double v[4]) { *(rff_f4 *)z = rff_f4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]}; }

template <class TX, class TZ, class EPI, int NG>
__global__ __launch_bounds__(RFF_NT) void k_rff(long long n, int d, int D, const TX *__restrict__ X, const double *__restrict__ Om, const double *__restrict__ beta, TZ *__restrict__ Z, EPI epi,
                                                int xvec, int zvec, int c0base)
{
  extern __shared__ double rff_lds[];
  double   *Ws = rff_lds, *Bs = rff_lds + RFF_KB * RFF_LDW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int c0 = c0base + blockIdx.y * RFF_CT, Dt = min(64 * NG, D - c0); // the launch's tiles have at most NG groups of 64 columns in use
  const int nkb = (d + RFF_KB - 1) / RFF_KB;
  const long long nrb = (n + RFF_RW - 1) / RFF_RW;
  const int sc = threadIdx.x & (RFF_CT - 1), sp = rff_pos(sc); // staging: this thread's column of the tile and its LDS position
  if (threadIdx.x < 64 * NG) Bs[sp] = sc < Dt ? beta[c0 + sc] : 0.0;
  bool staged = false;
  for (long long rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    RFF_PRODUCT_ROW_BLOCK(acc, rb)
    // the epilogue on the accumulators: group q of 64 columns sits in acc[0 .. 3] on trip q
    const long long r0 = rb * RFF_RW + wave * 16 + g;
#pragma nounroll
    for (int q = 0; q < NG; q++) {
      const int cc = 64 * q + 4 * c; // the lane's 4 columns of the tile: cc .. cc + 3
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const long long i = r0 + 4 * r;
        if (i < n && cc < Dt) {
          double v[4];
#pragma unroll
          for (int jm = 0; jm < 4; jm++) {
            v[jm] = epi(acc[jm][r] + Bs[64 * q + 16 * jm + c]);
            __builtin_amdgcn_sched_barrier(0); // one cosine at a time: interleaved, their temporaries do not fit beside 128 accumulator registers
          }
          TZ *z = Z + (size_t)i * D + c0 + cc;
          if (zvec) {
            rff_store4(z, v); // (D % 4 == 0: the 4 columns are inside together)
          } else {
#pragma unroll
            for (int jm = 0; jm < 4; jm++)
              if (cc + jm < Dt) z[jm] = (TZ)v[jm];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4 * NG - 4; j++) acc[j] = acc[j + 4];
    }
  }
}

// how many entries are not finite (a count: any order gives the same integer)
__global__ __launch_bounds__(PMH_BLOCK) void k_rff_bad(long long m, const double *__restrict__ a, int *__restrict__ bad)
{
  int b = 0;
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < m; i += (long long)gridDim.x * PMH_BLOCK) b += isfinite(a[i]) ? 0 : 1;
  if (b) atomicAdd(bad, b);
}

// one launch over ntiles column tiles from column c0base on, each with at most NG groups of 64 columns in use
template <class TX, class TZ, class EPI, int NG> static int rff_launch_ng(pmh_rff f, long long n, const void *X, void *Z, EPI epi, int c0base, int ntiles)
{
  auto *k = k_rff<TX, TZ, EPI, NG>;
  PMH_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, RFF_LDS_BYTES));
  const long long nrb  = (n + RFF_RW - 1) / RFF_RW;
  const int       cus  = f->ctx->num_cus > 0 ? f->ctx->num_cus : 256;
  const int       xvec = f->d % 4 == 0 && (uintptr_t)X % (4 * sizeof(TX)) == 0, zvec = f->D % 4 == 0 && (uintptr_t)Z % (4 * sizeof(TZ)) == 0;
  const dim3      grid((unsigned)(nrb < cus ? nrb : cus), (unsigned)ntiles);
  hipLaunchKernelGGL(k, grid, dim3(RFF_NT), RFF_LDS_BYTES, f->ctx->stream, n, f->d, f->D, (const TX *)X, (const double *)f->omega, (const double *)f->beta, (TZ *)Z, epi, xvec, zvec, c0base);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}
template <class TX, class TZ, class EPI> static int rff_launch(pmh_rff f, long long n, const void *X, void *Z, EPI epi)
{
  return rff_tile_launches(f->D, [&](auto ng, int tile0, int ntiles) { return rff_launch_ng<TX, TZ, EPI, decltype(ng)::value>(f, n, X, Z, epi, tile0 * RFF_CT, ntiles); });
}

int rff_count_not_finite(pmh_ctx ctx, const char *who, const char *what, long long m, const double *a_dev, long long *nbad)
{
  return sv_count_bad(ctx, who, what, [&](int *cnt) { hipLaunchKernelGGL(k_rff_bad, dim3(pmh_vec_grid((int)(m < (1 << 30) ? m : (1 << 30)))), dim3(PMH_BLOCK), 0, ctx->stream, m, a_dev, cnt); }, nbad);
}

int rff_identity_apply(pmh_rff f, long long n, const double *X_dev, void *Z_dev, int z_type)
{
  return z_type == PMH_F64 ? rff_launch<double, double>(f, n, X_dev, Z_dev, rff_arg{}) : rff_launch<double, float>(f, n, X_dev, Z_dev, rff_arg{});
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
  if (n < 0) return pmh_set_error(PMH_ERR_ARG, "pmh_rff_apply: n = %lld, must not be negative", n);
  PMH_CHK(rff_check_type("pmh_rff_apply", "x_type", x_type));
  PMH_CHK(rff_check_type("pmh_rff_apply", "z_type", z_type));
  if (n == 0) return PMH_SUCCESS;
  if (!X_dev || !Z_dev) return pmh_set_error(PMH_ERR_ARG, "pmh_rff_apply: X_dev or Z_dev is NULL with n = %lld", n);
  const rff_cos epi{f->scale};
  if (x_type == PMH_F64) return z_type == PMH_F64 ? rff_launch<double, double>(f, n, X_dev, Z_dev, epi) : rff_launch<double, float>(f, n, X_dev, Z_dev, epi);
  return z_type == PMH_F64 ? rff_launch<float, double>(f, n, X_dev, Z_dev, epi) : rff_launch<float, float>(f, n, X_dev, Z_dev, epi);
}

extern "C" int pmh_rff_test_args(pmh_rff f, long long n, const void *X_dev, int x_type, double *T_dev)
{
  PMH_ARG(f);
  if (n < 0) return pmh_set_error(PMH_ERR_ARG, "pmh_rff_test_args: n = %lld, must not be negative", n);
  PMH_CHK(rff_check_type("pmh_rff_test_args", "x_type", x_type));
  if (n == 0) return PMH_SUCCESS;
  if (!X_dev || !T_dev) return pmh_set_error(PMH_ERR_ARG, "pmh_rff_test_args: X_dev or T_dev is NULL with n = %lld", n);
  return x_type == PMH_F64 ? rff_launch<double, double>(f, n, X_dev, T_dev, rff_arg{}) : rff_launch<float, double>(f, n, X_dev, T_dev, rff_arg{});
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
