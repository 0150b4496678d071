// Structures of the multigrid V-cycle (mg.hip) shared with its multi-right-hand-side form (mg_mv.hip); internal
#pragma once
#include <vector>

#include "pmh_internal.h"

struct mg_level {
  pmh_csr  A, P;          // P: n_l x n_{l+1} (NULL on the coarsest level); A is used directly only if Ab == NULL
  pmh_bsr3 Ab;            // 3x3-block copy of A in the cycle's precision, or NULL
  int      n;
  void    *dinv, *x, *b, *r, *d, *t, *xa; // vectors in the cycle's precision; in fp64 x and b of level 0 are the caller's
  void    *pv, *rv;       // values of P and P' in the cycle's precision (fp32 copies: 8 instead of 12 bytes per entry; the
                          // trilinear weights 1, 1/2, 1/4, 1/8 are exact in any precision), or the CSR's own fp64 arrays
  bool     pv_owned;
  bool     long_rows = false; // P has > 12 entries per row on average (an aggregation hierarchy): the wavefront-per-row transfer kernels
  // node-level copies of P and P' when P = P_node (x) I_3 (cycle precision values), else NULL
  int     *pn_rowptr, *pn_col, *rn_rowptr, *rn_col;
  void    *pn_val, *rn_val;
  double   theta, delta;
  std::vector<double> c1, c2; // Chebyshev recurrence coefficients of steps 1..degree-1
};

struct pmh_mg_s {
  pmh_ctx               ctx;
  int                   nlevels, degree, is_float;
  std::vector<mg_level> L;
  int                   nb_coarse;
  int                  *d_crs;   // coarse block row starts [nb_coarse+1]
  long long            *d_cofs;  // offsets of the dense blocks [nb_coarse]
  void                 *d_cpinv; // concatenated dense pseudo-inverses, row-major, cycle precision (fp16 entries / cp_scale with PMH_MG_FP16)
  int                   cp_half;
  int                   coarse_m16; // every dense block has a multiple of 16 rows, at least 512 (the 8-column cycle's matrix-core coarse solve, mg_mv.hip)
  double                cp_scale;
  const int            *halt;
  long long             fine_spmv; // fine-level SpMVs issued (statistics)
  int                       timing_on;
  int                       fused; // degree 2 + block operators: smoothing steps finished inside the operator kernel
  std::vector<pmh_csr>      owned; // CSR handles created for this hierarchy by pmh_mg_create_box (destroyed with it)
};

// does level l run mg_fused_level (its first smoothing direction can then be produced by the kernel that makes its b: it rides on the restriction)?
static inline bool mg_is_fused_level(pmh_mg mg, int l) { return l < mg->nlevels - 1 && mg->fused && mg->L[l].Ab; }

// which pair of transfer kernels a level launches, as pmh_mg_test_info and pmh_mg_mv_test_info report it.  Node-wise where the node-level copies exist (both or none:
// P = P_node (x) I_3); else one column takes the scalar CSR by the row length of P, 8 columns the rectangular ELL pair of mv.hip where it could be built
// (2 and 3 mean one thing per column count -- the numbers the two test entries have always reported; the launchers of mg_transfer.h refuse ELL, which is mv.hip's)
enum { MG_TRANSFER_NONE = 0, MG_TRANSFER_NODAL = 1, /* one column */ MG_TRANSFER_SHORT = 2, MG_TRANSFER_LONG = 3, /* 8 columns */ MG_TRANSFER_ELL = 2, MG_TRANSFER_SCALAR = 3 };

// grid of a grid-stride kernel over work_items lanes
static inline dim3 mg_grid(long long work_items)
{
  const long long g = (work_items + PMH_BLOCK - 1) / PMH_BLOCK;
  return dim3((unsigned)(g < 1 ? 1 : (g > PMH_MAX_VEC_BLOCKS ? PMH_MAX_VEC_BLOCKS : g)));
}

// coarsest level: the dense block of a row, rs[lo] <= row < rs[lo + 1]
static __device__ __forceinline__ int mg_coarse_block(const int *__restrict__ rs, int nb, int row)
{
  int lo = 0, hi = nb;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (rs[mid] <= row) lo = mid;
    else hi = mid;
  }
  return lo;
}

// One smoothed level with the degree-2 Chebyshev steps finished inside the operator kernel (7 launches instead of 10), for one column and for 8:
//   d0 = D^-1 b/theta | xa = (1+c1) d0 + c2 D^-1 (b - A d0) | t = A xa - b | b_c = P't (+ the coarse d0) | ... | xa -= P x_c |
//   r, d, x = xa + d from A xa | x += c1 d + c2 (r - D^-1 A d)
// b64 / z64: fp64 input / output of an fp32 cycle's fine level (the conversions ride on the first and last kernel).  d0_ready: d (and the cycle-precision copy of b) were
// written by the producer of b.  F is the form:
//   typedef T; pmh_mg mg;             the cycle's scalar and the hierarchy
//   mg_vecs<T> vecs(l)                  level l's own vectors (b and x of the level the cycle enters are the arguments: in fp64 they are the caller's)
//   void d0(l, b, b64, dinv, itheta, d) the d0 kernel; with b64 it also writes b
//   int op(l, x, y, epi, e)             y = A_l x with an epilogue of the block kernel
//   int restrict_to(l, t, bc, dc), int prolong_sub(l, xc, x)   level l's transfers (dc == NULL: no coarse d0)
//   int descend(l, b, x, d0_ready)      the cycle on level l
template <typename T> struct mg_vecs {
  T *x, *b, *r, *d, *t, *xa;
};
template <typename F>
static int mg_fused_level(F &f, int l, const typename F::T *b, typename F::T *x, const double *b64, double *z64, bool d0_ready)
{
  typedef typename F::T T;
  const mg_level     &Lv = f.mg->L[l];
  const mg_vecs<T>    v = f.vecs(l), vc = f.vecs(l + 1);
  const T            *dinv   = (const T *)Lv.dinv;
  const T             itheta = (T)(1.0 / Lv.theta), c1 = (T)Lv.c1[1], c2 = (T)Lv.c2[1];
  if (!d0_ready) f.d0(l, b, b64, dinv, itheta, v.d);
  pmh_bsr3_epi<T> e;
  memset(&e, 0, sizeof(e));
  e.y1 = b, e.dinv = dinv, e.r = v.r, e.d = v.d;
  e.c0 = (T)1 + c1, e.c1 = c1, e.c2 = c2;
  PMH_CHK(f.op(l, v.d, v.xa, PMH_BSR_EPI_PRE, e));
  PMH_CHK(f.op(l, v.xa, v.t, PMH_EPI_SUB, e));
  const bool cf = mg_is_fused_level(f.mg, l + 1); // the coarse level's d0 rides on the restriction
  PMH_CHK(f.restrict_to(l, v.t, vc.b, cf ? vc.d : (T *)nullptr));
  PMH_CHK(f.descend(l + 1, vc.b, vc.x, cf));
  PMH_CHK(f.prolong_sub(l, vc.x, v.xa));
  PMH_HIP(hipGetLastError());
  e.c0 = itheta;
  PMH_CHK(f.op(l, v.xa, x, PMH_BSR_EPI_POST1, e));
  e.z64 = z64;
  return f.op(l, v.d, x, PMH_BSR_EPI_POST2, e);
}

