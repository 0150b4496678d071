// The box predicates of src/qpc/impls/box/qpcbox.c restated per element, shared by every kernel that folds a gradient split, a reduced gradient or a feasible step
// length into another pass (mpgp.hip, qppf.hip, dualchain.hip, vec.hip, spmv.hip, svm.hip), and on top of them the per-entry terms of MPGP's two vector phases
// (pmh_p1_terms, pmh_split_terms).  Two forms of the same arithmetic: on the bound ARRAYS (a null pointer = no bound on that side) and on the
// bound VALUES (-inf / +inf = no bound: every comparison then falls as with the null pointer), for kernels that load a row's scalars once, ahead of their use.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

// QPCGrads_Box qpcbox.c:41-55 (lower bound wins ties, `else if`)
static __device__ __forceinline__ void pmh_box_split(double xi, double gi, const double *lb, const double *ub, long long i, double astol, double &gf, double &gc)
{
  gf = gi;
  gc = 0.0;
  if (lb && fabs(xi - lb[i]) <= astol) {
    gf = 0.0;
    gc = (gi < 0.0) ? gi : 0.0;
  } else if (ub && fabs(xi - ub[i]) <= astol) {
    gf = 0.0;
    gc = (gi > 0.0) ? gi : 0.0;
  }
}
static __device__ __forceinline__ void pmh_box_split_v(double xi, double gi, double l, double u, double astol, double &gf, double &gc)
{
  gf = gi;
  gc = 0.0;
  if (fabs(xi - l) <= astol) {
    gf = 0.0;
    gc = (gi < 0.0) ? gi : 0.0;
  } else if (fabs(xi - u) <= astol) {
    gf = 0.0;
    gc = (gi > 0.0) ? gi : 0.0;
  }
}

// QPCGradReduced_Box qpcbox.c:86-92
static __device__ __forceinline__ double pmh_box_reduced(double xi, double gf, const double *lb, const double *ub, long long i, double alpha)
{
  double r = gf;
  if (lb && gf > 0.0) {
    double t = (xi - lb[i]) / alpha;
    r        = (gf < t) ? gf : t;
  } else if (ub && gf < 0.0) {
    double t = (xi - ub[i]) / alpha;
    r        = (gf < t) ? t : gf;
  }
  return r;
}
static __device__ __forceinline__ double pmh_box_reduced_v(double xi, double gf, double l, double u, bool has_l, bool has_u, double alpha)
{
  double r = gf;
  if (has_l && gf > 0.0) {
    double t = (xi - l) / alpha;
    r        = (gf < t) ? gf : t;
  } else if (has_u && gf < 0.0) {
    double t = (xi - u) / alpha;
    r        = (gf < t) ? t : gf;
  }
  return r;
}

// QPCFeas_Box (qpcbox.c:290-305), one entry: the step length along -p that keeps x on the box, folded into a running minimum
static __device__ __forceinline__ double pmh_box_feas_v(double m, double xi, double pi, double l, double u)
{
  if (pi > 0. && l > -INFINITY) m = fmin(m, (xi - l) / pi);
  if (pi < 0. && u < INFINITY) m = fmin(m, (xi - u) / pi);
  return m;
}
// ... on the arrays: a bound is loaded only where the sign of pi asks for it, x only where that bound is finite
static __device__ __forceinline__ double pmh_box_feas(double m, const double *x, double pi, const double *lb, const double *ub, long long i)
{
  if (pi > 0. && lb) {
    const double l = lb[i];
    if (l > -INFINITY) m = fmin(m, (x[i] - l) / pi);
  }
  if (pi < 0. && ub) {
    const double u = ub[i];
    if (u < INFINITY) m = fmin(m, (x[i] - u) / pi);
  }
  return m;
}

// ---- the two vector phases MPGP folds into an operator's last kernel (mpgp.hip k_p1_dots, k_split_setp, k_step_update; qppf.hip k_gt_fused1d; dualchain.hip
// k_dc_final), one entry each.  The operands stand in the order the reference's Vec calls take them: without contraction that order is the arithmetic. ----
// P1 (mpgp.c:537-544): s = (p'Ap, g'p, QPCFeas), from (0, 0, +inf)
static __device__ __forceinline__ void pmh_p1_terms(double (&s)[3], double pi, double api, double gi, const double *x, const double *lb, const double *ub, long long i)
{
  s[0] += pi * api;
  s[1] += gi * pi;
  s[2] = pmh_box_feas(s[2], x, pi, lb, ub, i);
}
static __device__ __forceinline__ void pmh_p1_terms_v(double (&s)[3], double pi, double api, double gi, double xi, double l, double u)
{
  s[0] += pi * api;
  s[1] += gi * pi;
  s[2] = pmh_box_feas_v(s[2], xi, pi, l, u);
}
// the gradient split of entry i and its squares (MPGPGrads mpgp.c:198-223, the reductions of :514-521): acc[1] += gP^2 (gP = gf + gc: VecWAXPY), acc[2] += gc^2,
// acc[3] += gf^2; acc[0] is the caller's (k_step_update's Ap'gf, else 0).  Returns gf
static __device__ __forceinline__ double pmh_split_terms(double (&acc)[4], double xi, double gi, const double *lb, const double *ub, long long i, double astol)
{
  double f, c;
  pmh_box_split(xi, gi, lb, ub, i, astol, f, c);
  const double gPi = f + c;
  acc[1] += gPi * gPi;
  acc[2] += c * c;
  acc[3] += f * f;
  return f;
}
