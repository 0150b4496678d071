// Scoring on random Fourier features without storing them: for a model W (K x D row-major, row stride ldw) over the features of the map of rff.hip,
//   dots[i, k] = sum_c  epi(x_i . omega_c + beta_c) W[k, c],   c = 0 .. D - 1                                     (n x K row-major; no bias is added),
// the quantity x_i . w the CSR paths of the front ends hand to k_svm_dots<F> and svmm_row_done.  There is no n x D array: the map's kernel holds 16 rows x 256
// columns of arguments per wave in accumulators, and where k_rff stores a feature, k_rff_dots multiplies it with the weights and keeps the sum.
//
// One kernel, k_rff_dots<TX, EPI, NG, KC>, for a chunk of kc <= KC = RFF_KC classes.  TX, EPI, NG are k_rff's (rff.hip); the product phase is k_rff's own text
// (RFF_PRODUCT_ROW_BLOCK, rff_internal.h): the operand layouts, Omega's LDS image and its permutation, the k-block loop, X one step ahead, zeros selected for rows
// >= n and k >= d, and the NG instances with the last tile in a launch of its own (rff_tile_launches).
//   weights   the chunk's weights over the column tile sit in LDS behind beta, KC x RFF_CT doubles at beta's permuted positions (rff_pos).  Columns >= D and
//             classes >= kc are ZEROS that are selected, never loaded: nothing past W[K - 1, D - 1] is read.  A padded column's feature is s cos(0) = s, not 0:
//             its zero weight alone keeps it out of the sum.
//   epilogue  a feature v is consumed where k_rff would store it: p[r][k] = fma(v, w, p[r][k]) -- a FUSED multiply-add, one rounding (the library is built
//             with -ffp-contract=off: this one is asked for by name) -- for the lane's 4 rows r and the chunk's classes k.  A lane's sum runs over its columns
//             in the order group q of 64 columns ascending, then jm ascending (column 64 q + 4 c + jm of the tile, c = lane & 15).
//   rows      the 16 lanes c of a row group (the same g = lane >> 4) hold 4 KC sums each, (row r, class k) at index r KC + k: the halving butterfly rff_halve_step over
//             the lane offsets 8, 4, 2, 1 -- at each step a lane gives half of its sums to its partner and adds what it receives to the half it keeps -- leaves one
//             complete (row, class) sum per lane (KC = 4; KC = 2: per lane pair), which that lane stores.  The tree has one shape for every index, and a + b is
//             b + a: class k's sum does not depend on where in the chunk k sits.  No atomics, no LDS reduction.
//   tiles     D <= RFF_CT: one launch per chunk, X read once, the sums stored straight into dots.  D > RFF_CT: every column tile (grid.y, the last one in its own
//             launch) stores its sums into part[i][tile][KC], and k_rff_dots_fin adds a row's tiles in ascending order: fixed by D alone.
//   chunks    K > KC: one launch (sequence) per chunk of KC classes, chunks ascending; the features are computed again for every chunk.
// So a sample's dots have the same bits alone and in any batch, at any row, in two calls, with K = 1 and as any class of a wider model; float X gives the bits
// of its widened copy; a NaN in a sample stays in that sample's dots (output row i takes only A's row i, and the butterfly adds nothing across rows).
// Registers (gfx950; docs/LAB_NOTEBOOK.md, "SVM fused feature scoring"): the NG = 4 cosine instance holds 128 accumulator registers, 8 KC of sums and the
// cosine's temporaries in 255 VGPRs, without scratch.
// Bytes per chunk: n d size_x read + 8 n kc written; flops 2 n d D on the matrix cores + n D cosines and 2 n D kc on the vector ALU.
#include "pmh_internal.h"

#include "rff_internal.h"

// The halving butterfly over the 16 lanes c of a row group, the idea of svmm_halve (svm_multi.hip): a lane holds NS = 2 M sums; at lane offset OFF it gives one
// half of them to its partner and adds what it receives to the half it keeps, then goes on with M / 2 at OFF / 2; the lanes complete what is left when one sum
// per lane remains (NS < 16).  Lane c ends with the complete sum of index c / (16 / NS).  One step per instantiation, so that every index into s is a constant:
// svmm_halve's loop over the steps is not unrolled at 16 sums, and the sums, indexed at run time, then take 50 registers more and a thousand selects
template <int M, int OFF, int NS> static __device__ __forceinline__ void rff_halve_step(double (&s)[NS], int c)
{
  if constexpr (M >= 1) {
    const bool up = (c & OFF) != 0;
#pragma unroll
    for (int j = 0; j < M; j++) {
      const double give = up ? s[j] : s[j + M], keep = up ? s[j + M] : s[j];
      s[j] = keep + __shfl_xor(give, OFF, 64);
    }
    rff_halve_step<M / 2, OFF / 2>(s, c);
  } else if constexpr (OFF >= 1) {
    s[0] += __shfl_xor(s[0], OFF, 64);
    rff_halve_step<0, OFF / 2>(s, c);
  }
}

template <class TX, class EPI, int NG, int KC>
__global__ __launch_bounds__(RFF_NT) void k_rff_dots(long long n, int d, int D, const TX *__restrict__ X, const double *__restrict__ Om, const double *__restrict__ beta, const double *__restrict__ W,
                                                     int ldw, int kc, double *__restrict__ out, long long ldo, int tstride, EPI epi, int xvec, int tile0)
{
  static_assert(KC == 1 || KC == 2 || KC == 4, "RFF_KC: the 4 KC sums of a lane are shared out over the 16 lanes of its rows");
  constexpr int LPS = 16 / (4 * KC); // lanes per finished sum
  extern __shared__ double rff_lds[];
  double   *Ws = rff_lds, *Bs = rff_lds + RFF_KB * RFF_LDW, *Vs = Bs + RFF_CT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int tile = tile0 + blockIdx.y, c0 = tile * RFF_CT, Dt = min(64 * NG, D - c0); // the launch's tiles have at most NG groups of 64 columns in use
  const int nkb = (d + RFF_KB - 1) / RFF_KB;
  const long long nrb = (n + RFF_RW - 1) / RFF_RW;
  const int sc = threadIdx.x & (RFF_CT - 1), sp = rff_pos(sc); // staging: this thread's column of the tile and its LDS position
  if (threadIdx.x < 64 * NG) Bs[sp] = sc < Dt ? beta[c0 + sc] : 0.0;
  if (sc < 64 * NG)
    for (int k = threadIdx.x / RFF_CT; k < KC; k += RFF_NT / RFF_CT) Vs[k * RFF_CT + sp] = (k < kc && sc < Dt) ? W[(size_t)k * ldw + c0 + sc] : 0.0;
  bool staged = false;
  for (long long rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    RFF_PRODUCT_ROW_BLOCK(acc, rb)
    // the epilogue on the accumulators: group q of 64 columns sits in acc[0 .. 3] on trip q.  A row >= n or a group of 4 columns >= Dt is passed over
    const long long r0 = rb * RFF_RW + wave * 16 + g;
    double          p[4 * KC];
#pragma unroll
    for (int j = 0; j < 4 * KC; j++) p[j] = 0.0;
#pragma nounroll
    for (int q = 0; q < NG; q++) {
      const int cc = 64 * q + 4 * c; // the lane's 4 columns of the tile: cc .. cc + 3
#pragma unroll
      for (int r = 0; r < 4; r++) {
        if (r0 + 4 * r < n && cc < Dt) {
#pragma unroll
          for (int jm = 0; jm < 4; jm++) {
            const int    pos = 64 * q + 16 * jm + c;
            const double v   = epi(acc[jm][r], 0.0, Bs[pos]);
#pragma unroll
            for (int k = 0; k < KC; k++) p[r * KC + k] = fma(v, Vs[k * RFF_CT + pos], p[r * KC + k]);
            __builtin_amdgcn_sched_barrier(0); // one cosine at a time, as in k_rff
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4 * NG - 4; j++) acc[j] = acc[j + 4];
    }
    // every lane takes part in the butterfly, whatever its rows are; lane c ends with the sum of index c / LPS
    rff_halve_step<2 * KC, 8>(p, c);
    const double    t   = p[0];
    const int       idx = c / LPS, k = idx % KC;
    const long long i   = r0 + 4 * (idx / KC);
    if (c % LPS == 0 && i < n && k < kc) out[(size_t)i * ldo + (size_t)tile * tstride + k] = t;
  }
}

// dots[i K + k] = part[i][0][k] + part[i][1][k] + .. (tiles ascending), k < kc: one thread per sum
__global__ __launch_bounds__(PMH_BLOCK) void k_rff_dots_fin(long long n, int ntiles, int KC, int kc, const double *__restrict__ part, double *__restrict__ dots, int K)
{
  for (long long t = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; t < n * kc; t += (long long)gridDim.x * PMH_BLOCK) {
    const long long i = t / kc;
    const int       k = (int)(t % kc);
    const double   *q = part + (size_t)i * ntiles * KC + k;
    double          s = q[0];
    for (int j = 1; j < ntiles; j++) s += q[(size_t)j * KC];
    dots[(size_t)i * K + k] = s;
  }
}

// one launch over ntiles column tiles from tile0 on, each with at most NG groups of 64 columns in use
template <class TX, class EPI, int NG>
static int rffd_launch_ng(pmh_rff f, long long n, const void *X, const double *W, int ldw, int kc, double *out, long long ldo, int tstride, EPI epi, int tile0, int ntiles)
{
  auto *k = k_rff_dots<TX, EPI, NG, RFF_KC>;
  PMH_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, RFF_DOTS_LDS_BYTES));
  const rff_shape s = rff_launch_shape<TX>(f->ctx, n, f->d, X, ntiles);
  hipLaunchKernelGGL(k, s.grid, dim3(RFF_NT), RFF_DOTS_LDS_BYTES, f->ctx->stream, n, f->d, f->D, (const TX *)X, (const double *)f->omega, (const double *)f->beta, W, ldw, kc, out, ldo, tstride, epi, s.xvec,
                     tile0);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

// the chunks ascending; D > RFF_CT: the tiles' sums go through part (n x ntiles x RFF_KC doubles of this call)
template <class TX, class EPI> static int rffd_run(pmh_rff f, long long n, const void *X, int K, const double *W, int ldw, double *dots, EPI epi)
{
  pmh_ctx   ctx    = f->ctx;
  const int ntiles = (f->D + RFF_CT - 1) / RFF_CT;
  double   *part   = nullptr;
  if (ntiles > 1) PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)n * ntiles * RFF_KC, (void **)&part));
  int rc = PMH_SUCCESS;
  for (int k0 = 0; k0 < K && !rc; k0 += RFF_KC) {
    const int     kc  = K - k0 < RFF_KC ? K - k0 : RFF_KC;
    const double *Wc  = W + (size_t)k0 * ldw;
    double       *out = part ? part : dots + k0;
    rc = rff_tile_launches(f->D, [&](auto ng, int tile0, int nt) {
      return rffd_launch_ng<TX, EPI, decltype(ng)::value>(f, n, X, Wc, ldw, kc, out, part ? (long long)ntiles * RFF_KC : (long long)K, part ? RFF_KC : 0, epi, tile0, nt);
    });
    if (!rc && part) {
      const long long nbl = (n * kc + PMH_BLOCK - 1) / PMH_BLOCK;
      hipLaunchKernelGGL(k_rff_dots_fin, dim3((unsigned)(nbl < PMH_MAX_VEC_BLOCKS ? nbl : PMH_MAX_VEC_BLOCKS)), dim3(PMH_BLOCK), 0, ctx->stream, n, ntiles, RFF_KC, kc, (const double *)part, dots + k0, K);
      if (hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "pmh_rffdots: the launch that adds the column tiles failed");
    }
  }
  if (part) pmh_free(ctx, part); // (waits for the stream)
  return rc;
}

static int rffd_check(const char *who, pmh_rff f, long long n, const void *X, int x_type, int K, const double *W, int ldw, const double *dots)
{
  return rff_check_entry(who, n, x_type, nullptr, X && W && dots, "X_dev, W_dev or dots_dev", [&] {
    if (K < 1) return pmh_set_error(PMH_ERR_ARG, "%s: K = %d, must be at least 1", who, K);
    if (ldw < f->D) return pmh_set_error(PMH_ERR_ARG, "%s: ldw = %d, must be at least D = %d", who, ldw, f->D);
    return (int)PMH_SUCCESS;
  });
}

extern "C" int pmh_rffdots(pmh_rff f, long long n, const void *X_dev, int x_type, int K, const double *W_dev, int ldw, double *dots_dev)
{
  PMH_ARG(f);
  PMH_CHK(rffd_check("pmh_rffdots", f, n, X_dev, x_type, K, W_dev, ldw, dots_dev));
  if (n == 0) return PMH_SUCCESS;
  const rff_cos epi{f->scale};
  return x_type == PMH_F64 ? rffd_run<double>(f, n, X_dev, K, W_dev, ldw, dots_dev, epi) : rffd_run<float>(f, n, X_dev, K, W_dev, ldw, dots_dev, epi);
}

extern "C" int pmh_rffdots_test_args(pmh_rff f, long long n, const void *X_dev, int x_type, int K, const double *W_dev, int ldw, double *dots_dev)
{
  PMH_ARG(f);
  PMH_CHK(rffd_check("pmh_rffdots_test_args", f, n, X_dev, x_type, K, W_dev, ldw, dots_dev));
  if (n == 0) return PMH_SUCCESS;
  return x_type == PMH_F64 ? rffd_run<double>(f, n, X_dev, K, W_dev, ldw, dots_dev, rff_arg{}) : rffd_run<float>(f, n, X_dev, K, W_dev, ldw, dots_dev, rff_arg{});
}
