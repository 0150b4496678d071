// What stage A of the Nystroem map (nys.hip: C = k(X, L), the kernel block) hands to k_rff, the kernel it shares with the random Fourier features (rff_kernel.h),
// each written once:
//   nys_poly, nys_rbf   the epilogue functors, in the one form every functor of k_rff has: what happens in registers to a product t = x . l, the row's value
//                       nx = |x|^2 (row(i): the chunk's norms, the functor's member) and the column's value nl = |l|^2; nys_poly takes neither
//   nys_t, nys_q        the identities of pmh_nys_test_args: t itself, and the rbf instance's q = max((nx + nl) - 2 t, 0)
//   pmh_nys_s           the map's handle
// The library is built with -ffp-contract=off: every product and every sum below is rounded on its own.
// Device code and the handle: included by nys.hip only.
#pragma once
#include "rff_kernel.h"

#define NYS_CHUNK_ROWS 65536 // rows of C that exist at a time in pmh_nys_apply: 512 row blocks, two per CU -- the smallest chunk on the plateau of the measured sweep (docs/LAB_NOTEBOOK.md, "SVM Nystroem features")
#define NYS_MAX_DEGREE 16

// |x - l|^2 from the norms and the product; a NaN stays a NaN (the comparison is false), a negative rounding residue becomes 0
static __device__ __forceinline__ double nys_dist2(double t, double nx, double nl)
{
  const double q = (nx + nl) - 2.0 * t;
  return q < 0.0 ? 0.0 : q;
}

struct nys_poly {
  static constexpr bool cols = false, rows = false;
  double                gamma, coef0;
  int                   degree;
  __device__ __forceinline__ double operator()(double t, double, double) const
  {
    const double b = gamma * t + coef0;
    double       v = b;
    for (int p = 1; p < degree; p++) v = v * b;
    return v;
  }
};
struct nys_rbf {
  static constexpr bool cols = true, rows = true;
  double                gamma;
  const double         *nx;
  __device__ __forceinline__ double row(long long i) const { return nx[i]; }
  __device__ __forceinline__ double operator()(double t, double nx, double nl) const { return exp(-(gamma * nys_dist2(t, nx, nl))); } // q >= 0: at most 1
};
struct nys_t {
  static constexpr bool cols = false, rows = false;
  __device__ __forceinline__ double operator()(double t, double, double) const { return t; }
};
struct nys_q {
  static constexpr bool cols = true, rows = true;
  const double         *nx;
  __device__ __forceinline__ double row(long long i) const { return nx[i]; }
  __device__ __forceinline__ double operator()(double t, double nx, double nl) const { return nys_dist2(t, nx, nl); }
};

struct pmh_nys_s {
  pmh_ctx   ctx;
  int       d, m, D, kernel, degree;
  double    gamma, coef0;
  double   *land, *lt, *nl; // device: the landmarks m x d as given, their transpose d x m (the Omega of the product phase), their squared norms (m)
  pmh_rff   stage_b;        // Z = C M: k_rff with the identity, on (m, D, M, beta = 0, 1.0); owns the device copy of M
  long long chunk_rows;
  double   *work, *nx; // chunk_rows x m doubles of C; chunk_rows squared norms of the chunk's rows
};
