// The transfer operators of the V-cycle, one column (mg.hip) and R = 8 interleaved columns (mg_mv.hip): b_c = P' t and x -= P x_c on the CSR of P' / P.
//
// Both are ONE loop: R G lanes walk a CSR row, lane (entry group g < G, column r < R) adds the entries g, g + G, ... of the row into NC sums -- an entry serves the
// NC components of its node (NC = 3: P = P_node (x) I_3, one node-level entry for three dofs, a third of the index / value bytes; NC = 1: the scalar CSR) -- and the G
// groups are summed by a butterfly in a fixed order.  Vectors are interleaved, v[(NC node + c) R + r].  The instances and why they have these shapes:
//   restriction  <TV, 1, 1, 8, 0>     rows of P' with <= 27 entries
//                <TV, 1, 1, 64, 0>    smoothed aggregation (mgsa.hip): hundreds of entries per row of P', a wavefront per row
//                <TV, 1, 3, 8, 0>     node-wise
//                <float, 8, 3, 4, 1>  node-wise; one lane per (node, column) walking the up to 27 entries alone takes 14 us per launch on every level of a 43^3 hierarchy
//                <float, 8, 1, 8, 1>  scalar; one lane per (row, column) takes 330 us per launch where the operator products take 55
//   prolongation <TV, 1, 1, 1>        <= 8 entries per row of P
//                <TV, 1, 1, 8>        ~ 30 entries per row of P (smoothed aggregation)
//                <TV, 1, 3, 1>        node-wise          <float, 8, 3, 1>  node-wise          <float, 8, 1, 1>  scalar
// The one-column kernels sum the groups over the lane offsets G/2 ... 1, the 8-column ones over R ... R G/2: both orders are pinned (tests/mg_cases.py: tree_halving,
// tree_adjacent), so the order is the template argument ASC and each form keeps its own.
// Every instance tests the halt word first and strides the rows by lane group: the R G lanes of a row share i, so a butterfly never meets a lane that has left
// the loop.  (Fetching the halt word beside the first row pointers behind a uniform trip count per workgroup gains nothing -- the compiler waits for the scalar load
// at the top all the same -- and its guarded loop costs the long-row instances 1 - 1.5 %: docs/LAB_NOTEBOOK.md, "V-cycle transfers".)
#pragma once
#include "mg_internal.h"

// dinv_c != NULL: the first smoothing direction of the coarse level, d_c = D_c^-1 b_c / theta_c, is written on the way (saves the d0 launch of every smoothed coarse
// level); dinv_c is per ROW, not per column
template <typename TV, int R, int NC, int G, int ASC>
__global__ __launch_bounds__(PMH_BLOCK) void k_mg_restrict(int nc, const int *__restrict__ halt, const int *__restrict__ rowptr, const int *__restrict__ col, const TV *__restrict__ val, const TV *__restrict__ t, TV *__restrict__ bc,
                                                         const TV *__restrict__ dinv_c, TV itheta_c, TV *__restrict__ d_c)
{
  constexpr int LPR = R * G, RPB = PMH_BLOCK / LPR; // lanes per row, rows per workgroup
  static_assert(LPR <= 64 && (LPR & (LPR - 1)) == 0, "the lanes of a row are one shuffle group");
  if (halt && *halt) return;
  const int r = threadIdx.x % R, g = (threadIdx.x / R) % G;
  for (int i = blockIdx.x * RPB + threadIdx.x / LPR; i < nc; i += gridDim.x * RPB) {
    TV s[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) s[c] = (TV)0;
    for (int k = rowptr[i] + g; k < rowptr[i + 1]; k += G) {
      const TV  w = val[k];
      const TV *p = t + (size_t)NC * col[k] * R + r;
#pragma unroll
      for (int c = 0; c < NC; c++) s[c] += w * p[c * R];
    }
#pragma unroll
    for (int o = ASC ? R : LPR / 2; ASC ? o < LPR : o >= R; o = ASC ? o << 1 : o >> 1)
#pragma unroll
      for (int c = 0; c < NC; c++) s[c] += __shfl_xor(s[c], o, LPR);
    if (g == 0) {
      const size_t o = (size_t)NC * i * R + r;
#pragma unroll
      for (int c = 0; c < NC; c++) bc[o + c * R] = s[c];
      if (dinv_c) {
#pragma unroll
        for (int c = 0; c < NC; c++) d_c[o + c * R] = dinv_c[NC * i + c] * s[c] * itheta_c;
      }
    }
  }
}

// coarse-grid correction x -= P x_c
template <typename TV, int R, int NC, int G>
__global__ __launch_bounds__(PMH_BLOCK) void k_mg_prolong_sub(int n, const int *__restrict__ halt, const int *__restrict__ rowptr, const int *__restrict__ col, const TV *__restrict__ val, const TV *__restrict__ xc, TV *__restrict__ x)
{
  constexpr int LPR = R * G, RPB = PMH_BLOCK / LPR;
  static_assert(LPR <= 64 && (LPR & (LPR - 1)) == 0, "the lanes of a row are one shuffle group");
  if (halt && *halt) return;
  const int r = threadIdx.x % R, g = (threadIdx.x / R) % G;
  for (int i = blockIdx.x * RPB + threadIdx.x / LPR; i < n; i += gridDim.x * RPB) {
    TV *xi = x + (size_t)NC * i * R + r;
    TV  a[NC], s[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) s[c] = (TV)0;
    if constexpr (G == 1) { // every lane stores: x is on its way while the row is walked (loaded at the end the node-wise one-column instance took 2.5 % longer)
#pragma unroll
      for (int c = 0; c < NC; c++) a[c] = xi[c * R];
    }
    for (int k = rowptr[i] + g; k < rowptr[i + 1]; k += G) {
      const TV  w = val[k];
      const TV *p = xc + (size_t)NC * col[k] * R + r;
#pragma unroll
      for (int c = 0; c < NC; c++) s[c] += w * p[c * R];
    }
#pragma unroll
    for (int o = LPR / 2; o >= R; o >>= 1)
#pragma unroll
      for (int c = 0; c < NC; c++) s[c] += __shfl_xor(s[c], o, LPR);
    if (g == 0) {
      if constexpr (G > 1) { // one lane of G stores: it loads x here (a predicated load in front of the row walk took 6.6 % longer)
#pragma unroll
        for (int c = 0; c < NC; c++) a[c] = xi[c * R];
      }
#pragma unroll
      for (int c = 0; c < NC; c++) xi[c * R] = a[c] - s[c];
    }
  }
}

// The launchers of level l's pair, by the transfer kind pmh_mg_test_info / pmh_mg_mv_test_info report (MG_TRANSFER_ELL is the 8-column form's own business: mv.hip).
// rows x lanes per row in long long; nrep > 1: the first of nrep congruent blocks (a prefix of the node-wise arrays).  d_c != NULL: the coarse level's d0 rides along.
// With R > 1 the kind 2 is MG_TRANSFER_ELL, which has no kernel here: refused, not taken for MG_TRANSFER_SHORT.
template <typename TV, int R>
static int mg_restrict(pmh_mg mg, int l, int kind, int nrep, const int *halt, const TV *t, TV *bc, TV *d_c)
{
  const mg_level &Lv = mg->L[l], &Lc = mg->L[l + 1];
  hipStream_t     st = mg->ctx->stream;
  const dim3      blk(PMH_BLOCK);
  const TV       *dv = d_c ? (const TV *)Lc.dinv : (const TV *)nullptr;
  const TV        it = d_c ? (TV)(1.0 / Lc.theta) : (TV)0;
  constexpr int   MV = R > 1; // the 8-column kernels: ascending butterfly, 4 entry groups on the node-wise rows
  PMH_ARG(kind != MG_TRANSFER_NONE && !(MV && kind == MG_TRANSFER_ELL));
  if (kind == MG_TRANSFER_NODAL) {
    const int ncn = Lc.n / 3 / nrep;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mg_restrict<TV, R, 3, MV ? 4 : 8, MV>), mg_grid((long long)ncn * R * (MV ? 4 : 8)), blk, 0, st, ncn, halt, (const int *)Lv.rn_rowptr, (const int *)Lv.rn_col, (const TV *)Lv.rn_val, t, bc, dv, it, d_c);
    return PMH_SUCCESS;
  }
  pmh_csr Rt = Lv.P->transpose;
  if constexpr (!MV)
    if (kind == MG_TRANSFER_LONG) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mg_restrict<TV, 1, 1, 64, 0>), mg_grid((long long)Lc.n * 64), blk, 0, st, Lc.n, halt, (const int *)Rt->d_rowptr, (const int *)Rt->d_col, (const TV *)Lv.rv, t, bc, dv, it, d_c);
      return PMH_SUCCESS;
    }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mg_restrict<TV, R, 1, 8, MV>), mg_grid((long long)Lc.n * R * 8), blk, 0, st, Lc.n, halt, (const int *)Rt->d_rowptr, (const int *)Rt->d_col, (const TV *)Lv.rv, t, bc, dv, it, d_c);
  return PMH_SUCCESS;
}

template <typename TV, int R>
static int mg_prolong_sub(pmh_mg mg, int l, int kind, int nrep, const int *halt, const TV *xc, TV *x)
{
  const mg_level &Lv = mg->L[l];
  hipStream_t     st = mg->ctx->stream;
  const dim3      blk(PMH_BLOCK);
  PMH_ARG(kind != MG_TRANSFER_NONE && !(R > 1 && kind == MG_TRANSFER_ELL));
  if (kind == MG_TRANSFER_NODAL) {
    const int nn = Lv.n / 3 / nrep;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mg_prolong_sub<TV, R, 3, 1>), mg_grid((long long)nn * R), blk, 0, st, nn, halt, (const int *)Lv.pn_rowptr, (const int *)Lv.pn_col, (const TV *)Lv.pn_val, xc, x);
    return PMH_SUCCESS;
  }
  if constexpr (R == 1)
    if (kind == MG_TRANSFER_LONG) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mg_prolong_sub<TV, 1, 1, 8>), mg_grid((long long)Lv.n * 8), blk, 0, st, Lv.n, halt, (const int *)Lv.P->d_rowptr, (const int *)Lv.P->d_col, (const TV *)Lv.pv, xc, x);
      return PMH_SUCCESS;
    }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mg_prolong_sub<TV, R, 1, 1>), mg_grid((long long)Lv.n * R), blk, 0, st, Lv.n, halt, (const int *)Lv.P->d_rowptr, (const int *)Lv.P->d_col, (const TV *)Lv.pv, xc, x);
  return PMH_SUCCESS;
}
