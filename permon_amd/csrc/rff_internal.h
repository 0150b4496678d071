// What the kernels over the product x . omega_k share, each written once: k_rff (rff_kernel.h: Z = epi(X Omega), stored -- the random Fourier features of rff.hip
// and the kernel block of the Nystroem map, nys.hip) and k_rff_dots (rff_score.hip: the Fourier features multiplied by a model's weights and summed over the
// columns, never stored).
//   RFF_*                 the tiling: RFF_WAVES waves of 16 rows, a column tile of RFF_CT columns, k-blocks of RFF_KB rows of Omega in LDS
//   rff_cos, rff_arg      the epilogue functors of the Fourier features, in the one form every functor of k_rff has (rff_kernel.h): what happens in registers to a
//                         product t = x . omega_k, a value of the row (none here) and the column's value beta_k
//   rff_pos               where a column of the tile sits in LDS (Omega's image, beta and the weights of k_rff_dots are permuted alike)
//   rff_load4             4 consecutive entries of a row of X as doubles, zeros past d
//   RFF_PRODUCT_ROW_BLOCK the product phase of a row block: the staging of Omega, the k-block loop with X one step ahead and the MFMAs.  The layouts and the order
//                         of a row's sum are described in rff.hip
//   rff_tile_launches     which instance is launched over which column tiles
//   rff_launch_shape      the grid of such a launch and whether X is read in vectors
//   rff_check_entry       the argument checks every entry over n samples opens with
//   pmh_rff_s             the map's handle
// Device code and the handle: included by rff.hip, rff_score.hip and nys.hip only.
#pragma once
#include <type_traits>

#include "pmh_internal.h"

#define RFF_WAVES 8
#define RFF_NT (64 * RFF_WAVES)
#define RFF_RW (16 * RFF_WAVES) // rows per workgroup and trip
#define RFF_CT 256              // column tile
#define RFF_KB 64               // k-block
#define RFF_LDW 260             // row stride of Omega's LDS image (doubles)
#define RFF_LDS_BYTES ((RFF_KB * RFF_LDW + RFF_CT) * (int)sizeof(double)) // the k-block of Omega and the tile's beta, permuted alike
// k_rff_dots: the classes of a chunk (a power of two, at most 4: the 4 RFF_KC sums of a lane are shared out over the 16 lanes of its rows), and its LDS: the
// chunk's weights over the column tile behind beta, permuted as beta is
#ifndef RFF_KC
#define RFF_KC 4
#endif
#define RFF_DOTS_LDS_BYTES (RFF_LDS_BYTES + RFF_KC * RFF_CT * (int)sizeof(double))

typedef double rff_d4 __attribute__((ext_vector_type(4)));
typedef float  rff_f4 __attribute__((ext_vector_type(4)));

// t + beta is one rounded sum, then the cosine (the library is built with -ffp-contract=off)
struct rff_cos {
  static constexpr bool cols = true, rows = false;
  double                s;
  __device__ __forceinline__ double operator()(double t, double, double beta) const { return s * cos(t + beta); }
};
struct rff_arg {
  static constexpr bool cols = true, rows = false;
  __device__ __forceinline__ double operator()(double t, double, double beta) const { return t + beta; }
};

// LDS position of column cc of the column tile: tile j = 4 (cc >> 6) + (cc & 3), lane column (cc & 63) >> 2
static __device__ __forceinline__ int rff_pos(int cc) { return (cc & ~63) + 16 * (cc & 3) + ((cc & 63) >> 2); }

// X[row][k .. k + 4) as doubles, zeros past d (xr == nullptr: a row past n, all zeros); vec: d % 4 == 0 and X aligned to the vector
static __device__ __forceinline__ rff_d4 rff_load4(const double *xr, int k, int d, int vec)
{
  rff_d4 v = {0.0, 0.0, 0.0, 0.0};
  if (!xr || k >= d) return v;
  if (vec) return __builtin_nontemporal_load((const rff_d4 *)(xr + k));
#pragma unroll
  for (int e = 0; e < 4; e++)
    if (k + e < d) v[e] = xr[k + e];
  return v;
}
static __device__ __forceinline__ rff_d4 rff_load4(const float *xr, int k, int d, int vec)
{
  rff_d4 v = {0.0, 0.0, 0.0, 0.0};
  if (!xr || k >= d) return v;
  if (vec) {
    const rff_f4 f = __builtin_nontemporal_load((const rff_f4 *)(xr + k));
    v[0] = (double)f[0], v[1] = (double)f[1], v[2] = (double)f[2], v[3] = (double)f[3];
    return v;
  }
#pragma unroll
  for (int e = 0; e < 4; e++)
    if (k + e < d) v[e] = (double)xr[k + e];
  return v;
}

// The product phase of one row block rb, the text k_rff and k_rff_dots expand inside their walk `for (rb = blockIdx.x; rb < nrb; rb += gridDim.x)`: it declares
// acc[4 NG] and leaves in acc[j] the instruction tile j of X[the wave's 16 rows of rb] times Omega[:, c0 .. c0 + Dt) (NG groups of 64 columns).  A macro and not
// a function: a kernel that reaches this loop through a call, however it is inlined, is scheduled and given registers differently from the kernel that
// contains it (docs/LAB_NOTEBOOK.md, "SVM fused feature scoring"), and k_rff's instances must stay what they were.  It reads the names of the kernel around it:
//   the template arguments TX and NG; the arguments n, d, D, X, Om, xvec; Ws (Omega's LDS image, RFF_KB x RFF_LDW doubles); wave, c = lane & 15, g = lane >> 4;
//   c0, Dt (the tile's first column and its columns in use); nkb (k-blocks); sc, sp (the thread's staging column of the tile and its LDS position: rff_pos);
//   bool staged (false before the first row block).
// The first staging ends in a __syncthreads, which also publishes what the kernel put into LDS before its walk (beta, the weights)
#define RFF_PRODUCT_ROW_BLOCK(acc, rb)                                                                                                                               \
  const long long row = (rb) * RFF_RW + wave * 16 + c;                                                                                                               \
  const TX       *xr  = row < n ? X + (size_t)row * d : nullptr;                                                                                                     \
  rff_d4          acc[4 * NG];                                                                                                                                       \
  _Pragma("unroll") for (int j = 0; j < 4 * NG; j++) acc[j] = rff_d4{0.0, 0.0, 0.0, 0.0};                                                                            \
  for (int kb = 0; kb < nkb; kb++) {                                                                                                                                 \
    const int k0 = kb * RFF_KB, nt = (min(RFF_KB, d - k0) + 15) >> 4; /* nt: the k-block's steps of 16 in use */                                                     \
    rff_d4    xn = rff_load4(xr, k0 + 4 * g, d, xvec);                /* X one step of 16 ahead of the products */                                                   \
    if (nkb > 1 || !staged) {                                                                                                                                        \
      if (staged) __syncthreads(); /* the previous image has been read by all waves */                                                                               \
      if (sc < 64 * NG)                                                                                                                                              \
        for (int kk = threadIdx.x / RFF_CT; kk < 16 * nt; kk += RFF_NT / RFF_CT)                                                                                     \
          Ws[kk * RFF_LDW + sp] = (k0 + kk < d && sc < Dt) ? Om[(size_t)(k0 + kk) * D + c0 + sc] : 0.0;                                                              \
      __syncthreads();                                                                                                                                               \
      staged = true;                                                                                                                                                 \
    }                                                                                                                                                                \
    _Pragma("nounroll") for (int t = 0; t < nt; t++) {                                                                                                               \
      const rff_d4 xa = xn;                                                                                                                                          \
      if (t + 1 < nt) xn = rff_load4(xr, k0 + 16 * (t + 1) + 4 * g, d, xvec);                                                                                        \
      _Pragma("unroll") for (int e = 0; e < 4; e++) {                                                                                                                \
        const double *wr = Ws + (16 * t + 4 * g + e) * RFF_LDW + c;                                                                                                  \
        _Pragma("unroll") for (int j = 0; j < 4 * NG; j++) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[e], wr[16 * j], acc[j], 0, 0, 0);                        \
      }                                                                                                                                                              \
    }                                                                                                                                                                \
  }

// The launches that cover D columns: the whole column tiles in one launch of the NG = 4 instance, the last, narrower one in a launch of the instance with as many
// groups of 64 columns as it needs, so that its products of zeros stay below 64 columns' worth.  launch(ng, tile0, ntiles): ng an integral constant
template <class L> static int rff_tile_launches(int D, L launch)
{
  const int nfull = D / RFF_CT, tail = D % RFF_CT;
  if (nfull) PMH_CHK(launch(std::integral_constant<int, 4>{}, 0, nfull));
  switch ((tail + 63) / 64) {
  case 0: return PMH_SUCCESS;
  case 1: return launch(std::integral_constant<int, 1>{}, nfull, 1);
  case 2: return launch(std::integral_constant<int, 2>{}, nfull, 1);
  case 3: return launch(std::integral_constant<int, 3>{}, nfull, 1);
  default: return launch(std::integral_constant<int, 4>{}, nfull, 1);
  }
}

struct pmh_rff_s {
  pmh_ctx ctx;
  int     d, D;
  double  scale;
  double *omega, *beta; // device copies: d x D row-major, D
};

// The grid of a launch over ntiles column tiles -- a workgroup per row block, at most one per CU: it walks its row blocks -- and whether X is read in vectors
struct rff_shape {
  dim3 grid;
  int  xvec;
};
template <class TX> static inline rff_shape rff_launch_shape(pmh_ctx ctx, long long n, int d, const void *X, int ntiles)
{
  const long long nrb = (n + RFF_RW - 1) / RFF_RW;
  const int       cus = ctx->num_cus > 0 ? ctx->num_cus : 256;
  return {dim3((unsigned)(nrb < cus ? nrb : cus), (unsigned)ntiles), d % 4 == 0 && (uintptr_t)X % (4 * sizeof(TX)) == 0};
}

// For nys.hip (definitions: rff.hip).  rff_identity_apply: Z (n x f->D of z_type) = X f->omega + f->beta for fp64 X on the device -- the launches of
// pmh_rff_test_args, k_rff<double, TZ, rff_arg, NG>, with either type of Z.  rff_count_not_finite: *nbad = how many of a[0 .. m) are not finite, as
// pmh_rff_create counts them (k_rff_bad)
int rff_identity_apply(pmh_rff f, long long n, const double *X_dev, void *Z_dev, int z_type);
int rff_count_not_finite(pmh_ctx ctx, const char *who, const char *what, long long m, const double *a_dev, long long *nbad);

static inline int rff_check_type(const char *who, const char *what, int t)
{
  if (t != PMH_F64 && t != PMH_F32) return pmh_set_error(PMH_ERR_ARG, "%s: %s = %d, must be PMH_F64 (0) or PMH_F32 (1)", who, what, t);
  return PMH_SUCCESS;
}

// What the entry `who` over n samples opens with, in the order it is reported: n < 0, the type codes (z_type: nullptr where the entry has none), what the entry
// alone checks (more(): PMH_SUCCESS or its error) and, with n > 0, a NULL among its arrays (arrays: none is NULL; names: how the message lists them).  n == 0
// passes whatever the pointers are: the caller then returns PMH_SUCCESS before it touches them
template <class MORE> static int rff_check_entry(const char *who, long long n, int x_type, const int *z_type, bool arrays, const char *names, MORE more)
{
  if (n < 0) return pmh_set_error(PMH_ERR_ARG, "%s: n = %lld, must not be negative", who, n);
  PMH_CHK(rff_check_type(who, "x_type", x_type));
  if (z_type) PMH_CHK(rff_check_type(who, "z_type", *z_type));
  PMH_CHK(more());
  if (n > 0 && !arrays) return pmh_set_error(PMH_ERR_ARG, "%s: %s is NULL with n = %lld", who, names, n);
  return PMH_SUCCESS;
}
static inline int rff_check_entry(const char *who, long long n, int x_type, const int *z_type, bool arrays, const char *names)
{
  return rff_check_entry(who, n, x_type, z_type, arrays, names, [] { return PMH_SUCCESS; });
}
