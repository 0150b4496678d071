// Jacobi scaling from a CSR matrix: the block CG of MATINV (feti.hip) and every smoothed level of the V-cycle (mg.hip); internal
#pragma once
#include <algorithm>

#include "pmh_internal.h"

// position of the LAST entry (row i, column i) of a CSR row, -1 if there is none: 8 lanes walk the row together (one thread per row read 81 entries one after the
// other: 2 ms for the 2 M rows of configs[2])
static __device__ __forceinline__ int pmh_diag_pos8(const int *__restrict__ rowptr, const int *__restrict__ col, int i, int lane8)
{
  int best = -1;
  for (int k = rowptr[i] + lane8; k < rowptr[i + 1]; k += 8)
    if (col[k] == i) best = k;
  best = max(best, __shfl_xor(best, 4, 8));
  best = max(best, __shfl_xor(best, 2, 8));
  best = max(best, __shfl_xor(best, 1, 8));
  return best;
}
// dinv = 1 / diagonal in TV, 1 where the row stores no diagonal or a zero one; jacobi == 0: all ones.  Grid: pmh_diag_inv_grid(n)
template <typename TV>
__global__ __launch_bounds__(PMH_BLOCK) void k_extract_dinv(int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val, int jacobi, TV *__restrict__ dinv)
{
  const int lane8 = threadIdx.x & 7;
  for (int i0 = (blockIdx.x * PMH_BLOCK + threadIdx.x) >> 3; i0 < ((n + 7) & ~7); i0 += (gridDim.x * PMH_BLOCK) >> 3) { // uniform trip count within every group of 8 lanes
    const int i = min(i0, n - 1);
    double    d = 1.0;
    if (jacobi) {
      const int k = pmh_diag_pos8(rowptr, col, i, lane8);
      d           = (k >= 0) ? val[k] : 0.0;
      d           = (d != 0.0) ? 1.0 / d : 1.0;
    }
    if (lane8 == 0 && i0 < n) dinv[i] = (TV)d;
  }
}
static inline dim3 pmh_diag_inv_grid(int n) { return dim3(pmh_vec_grid((int)std::min<long long>(8LL * n, 0x7fffff00LL))); }
