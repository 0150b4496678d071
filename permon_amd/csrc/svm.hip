// Dense-row Hessian of the PermonSVM-style hinge-loss dual (BASELINE.json configs[4], SURVEY 8d "C5"):
//   H = diag(y) X X' diag(y),  X in R^{N x d} row-major (one sample per row), applied matrix-free as two GEMV
//   passes over X:  w = X'(y o a)  (d-vector),  (H a)_i = y_i (x_i . w).
// PermonSVM is a separate repository (README.md:12) with no code or tests in the reference tree, so this operator
// is "parity unpinned" beyond the MPGP solver that calls it; the oracle side of its test is a numpy restatement.
// HBM-bound: algorithmic bytes per apply 2*8*N*d + 40*N (X read twice; a, y read, Ha written, y read again).
// Samples shard over GPUs by rows; the only exchange is the all-reduce of w (d doubles) between the passes.
// The samples are stored in fp64 or in float32 (pmh_op_create_svm_dual_f32: 4 bytes per feature in memory and in every pass, 2*4*N*d + 40*N per apply); a float
// is widened where it is loaded and everything else -- w, the n-vectors, every sum, the all-reduce -- is fp64 either way (svm_rows.h).
#include "pmh_internal.h"
#include "reduce.h"
#include "box_inline.h"

#include "svm_internal.h"
#include "svm_rows.h"

// pass 1: per-workgroup partial of w = sum_i (y_i a_i) x_i ; one wavefront per row, lane j owns columns j, j+64, ...
// AUG: also s = sum_i y_i a_i (-> spart[workgroup]) and, where u is given, sum_i y_i u_i (-> upart[workgroup]); every lane of a wave holds the same two sums
// SUB (every kernel below that has it): y holds the masked labels m_i y_i of a sample subset (pmh_op_svm_dual_set_subset); it is read first, and a held-out row
// (y_i == 0) is not loaded and adds to no sum, whatever a_i holds.  SUB = 0: the kernels without subsets
// T (every kernel below that has it): the type the samples are stored in, double or float; a float is widened where it is loaded and the arithmetic is the same
template <int AUG, int SUB, class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_xt(int n, int d, const T *__restrict__ X, const double *__restrict__ y, const double *__restrict__ a, double *__restrict__ part,
                                                      double *__restrict__ spart, const double *__restrict__ u, double *__restrict__ upart)
{
  __shared__ double lds[PMH_BLOCK / 64][64 * SVM_KMAX];
  __shared__ double sred[AUG ? 2 : 1][AUG ? PMH_BLOCK / 64 : 1]; // (used by the augmented form only)
  double            as = 0.0, au = 0.0;
  const int         lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long   gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  double            acc[SVM_KMAX];
#pragma unroll
  for (int k = 0; k < SVM_KMAX; k++) acc[k] = 0.0;
  for (long long i = gw; i < n; i += nw) {
    if (SUB && y[i] == 0.0) continue; // (uniform over the wave)
    const double s  = y[i] * a[i];
    const T     *xr = X + (size_t)i * d;
    if (AUG) {
      as += s;
      if (u) au += y[i] * u[i];
    }
#pragma unroll
    for (int k = 0; k < SVM_KMAX; k++) {
      const int c = lane + 64 * k;
      if (c < d) acc[k] += s * (double)__builtin_nontemporal_load(&xr[c]);
    }
  }
  if (AUG && lane == 0) sred[0][wave] = as, sred[AUG][wave] = au;
#pragma unroll
  for (int k = 0; k < SVM_KMAX; k++) lds[wave][lane + 64 * k] = acc[k];
  __syncthreads();
  for (int c = threadIdx.x; c < d; c += PMH_BLOCK) {
    double v = lds[0][c];
#pragma unroll
    for (int wv = 1; wv < PMH_BLOCK / 64; wv++) v += lds[wv][c];
    part[(size_t)blockIdx.x * d + c] = v;
  }
  if (AUG && threadIdx.x == 0) {
    double v0 = sred[0][0], v1 = sred[AUG][0];
#pragma unroll
    for (int wv = 1; wv < PMH_BLOCK / 64; wv++) v0 += sred[0][wv], v1 += sred[AUG][wv];
    spart[blockIdx.x] = v0;
    if (upart) upart[blockIdx.x] = v1;
  }
}

// w[c] = sum over workgroups of part[b][c], one wavefront per column, fixed order; spart != nullptr: one column more, w[d] = sum over workgroups of spart[b]
static __device__ __forceinline__ void svm_colsum(int nblocks, int d, const double *__restrict__ part, double *__restrict__ w, const double *__restrict__ spart)
{
  const int lane = threadIdx.x & 63, c = blockIdx.x * (PMH_BLOCK / 64) + (threadIdx.x >> 6);
  if (c >= d + (spart ? 1 : 0)) return;
  double v = 0.0;
  if (c == d) {
    for (int b = lane; b < nblocks; b += 64) v += spart[b];
  } else
  for (int b = lane; b < nblocks; b += 64) v += part[(size_t)b * d + c];
  v = pmh_wave_sum(v);
  if (lane == 0) w[c] = v;
}
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_colsum(int nblocks, int d, const double *__restrict__ part, double *__restrict__ w, const double *__restrict__ spart) { svm_colsum(nblocks, d, part, w, spart); }
int pmh_svm_colsum(pmh_ctx ctx, int nblocks, int d, const double *part, double *w, const double *spart)
{
  hipLaunchKernelGGL(k_svm_colsum, dim3((d + (spart ? 1 : 0) + 3) / 4), dim3(PMH_BLOCK), 0, ctx->stream, nblocks, d, part, w, spart);
  PMH_HIP(hipGetLastError()); // (also the launch of the pass that filled part)
  return PMH_SUCCESS;
}

// pass 2: (H a)_i = y_i (x_i . w); AUG 1: + sigma s y_i + shift a_i; AUG 2: + sigma s y_i + diag_i a_i
template <int AUG, int SUB, class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_x(int n, int d, const T *__restrict__ X, const double *__restrict__ y, const double *__restrict__ w, double *__restrict__ Ha,
                                                     const double *__restrict__ a, double sigma, double shift, const double *__restrict__ diag)
{
  const double sS = AUG ? sigma * w[d] : 0.0;
  svm_sweep_rows<SUB>(n, d, X, w, [&](long long i, double s) { Ha[i] = (SUB && y[i] == 0.0) ? 0.0 : (AUG ? svm_aug_row(y[i], s, sS, AUG == 2 ? diag[i] : shift, a[i]) : y[i] * s); }, y);
}

// ---- d == 64 fast path: the RPI-rows-per-wave-instruction layout of svm_rows.h (double: 2 rows, float: 4), 4-fold unroll ----
// (svm_fold_cols, which finishes a lane's column sums, is in svm_rows.h: svr.hip folds the same way)
// pass 1 for d = 64.  A wave takes RPI SVM_UNR rows at a time, rows r0 + RPI u + sub to the LPR lanes sub; a lane's column sums take its rows in the order
// it visits them (u ascending within a group, groups ascending), then svm_fold_cols
template <int SVM_UNR, int AUG, int SUB, class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_xt64(int n, const T *__restrict__ X, const double *__restrict__ y, const double *__restrict__ a, double *__restrict__ part,
                                                        double *__restrict__ spart, const double *__restrict__ uu, double *__restrict__ upart)
{
  typedef svm_row64<T> R;
  __shared__ double lds[PMH_BLOCK / 64][64];
  __shared__ double red[PMH_BLOCK / 64];
  double            as = 0.0, au = 0.0; // AUG: sum_i y_i a_i, sum_i y_i u_i, taken by the first of the LPR lanes of a row for its rows
  const int         lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / R::LPR, lq = lane & (R::LPR - 1);
  const long long   gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  double            acc[R::CPL];
#pragma unroll
  for (int c = 0; c < R::CPL; c++) acc[c] = 0.0;
  for (long long r0 = gw * R::RPI * SVM_UNR; r0 < n; r0 += nw * R::RPI * SVM_UNR) {
    typename R::vec v[SVM_UNR];
    double          s[SVM_UNR];
#pragma unroll
    for (int u = 0; u < SVM_UNR; u++) {
      const long long i = r0 + R::RPI * u + sub;
      const bool      ok = i < n && (!SUB || y[i] != 0.0);
      v[u] = ok ? __builtin_nontemporal_load((const typename R::vec *)(X + (size_t)i * 64) + lq) : R::zero();
      s[u] = ok ? y[i] * a[i] : 0.0;
      if (AUG && lq == 0) {
        as += s[u];
        if (uu && ok) au += y[i] * uu[i];
      }
    }
#pragma unroll
    for (int u = 0; u < SVM_UNR; u++) {
#pragma unroll
      for (int c = 0; c < R::CPL; c++) acc[c] += s[u] * R::col(v[u], c);
    }
  }
  svm_fold_cols<T>(acc, lds, part);
  if (AUG) {
    const double r0 = pmh_block_reduce<PMH_RED_SUM>(as, red), r1 = pmh_block_reduce<PMH_RED_SUM>(au, red);
    if (threadIdx.x == 0) {
      spart[blockIdx.x] = r0;
      if (upart) upart[blockIdx.x] = r1;
    }
  }
}

template <int SVM_UNR, int AUG, int SUB, class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_x64(int n, const T *__restrict__ X, const double *__restrict__ y, const double *__restrict__ w, double *__restrict__ Ha,
                                                       const double *__restrict__ a, double sigma, double shift, const double *__restrict__ diag)
{
  const double sS = AUG ? sigma * w[64] : 0.0;
  svm_sweep_rows64<SVM_UNR, SUB>(n, X, w, [&](long long i, double s) { Ha[i] = (SUB && y[i] == 0.0) ? 0.0 : (AUG ? svm_aug_row(y[i], s, sS, AUG == 2 ? diag[i] : shift, a[i]) : y[i] * s); }, y);
}

// ---- paired passes -------------------------------------------------------------------------------------------------------------------------
// One application of H streams X twice (w = X'(y o a), then y o (X w)); an MPGP expansion step applies H twice (Ap = H p, then g = H x+ - b): four passes over
// X, 2.56 GB each for configs[4], and the kernels already run at the box's streaming rate.  But the row that pass 2 of one application has in registers is the
// row pass 1 of the NEXT application needs, and what that next application multiplies is an elementwise function of this pass's result:
//   * the gradient pass g_i = y_i (x_i . w) - b_i knows gf_i, hence p_i = gf_i, hence (y_i p_i) x_i: it accumulates X'(y o p) for the P1 that follows, and the
//     feasible step length QPCFeas(x, p) (which needs no Ap);
//   * the P1 pass  (Ap)_i = y_i (x_i . w)  knows, with that afeas and the fixed alpha, the iterate an expansion step would produce,
//     x+_i = k_expansion_std(x_i, g_i, p_i, (Ap)_i): it stores it and accumulates X'(y o x+) for the gradient that follows IF the host then chooses the
//       expansion.
// A run of expansion steps costs two passes over X per step instead of four; a CG or proportioning step discards the prepared sums and pays the usual passes.
// The driver says what is fresh (pmh_vec_epi::p_fresh / spec_alpha / x_from_spec); the partial sums of the MPGP reductions go to the same rows of the context's
// partials as the separate Vec kernels write, one entry per workgroup of pmh_vec_grid(n) (the elements a workgroup sums are other ones: same values to
// rounding).

struct svm_grad_args {
  const double *b, *x_in, *lb, *ub;
  double       *x_out, *g, *gf, *p, *partials, *feas_part, *part_next;
  double        astol;
  int           ld, prow;
  // AUG
  double       *spart_next;
  double        sigma, shift;
  const double *diag; // AUG 2: the diagonal, in place of shift
};
// what a lane asks for of its row before the dot products arrive (svm_sweep_rows64_lanes' pre); sh: the shift or diag_i
struct svm_grad_row {
  double yi, xi, bi, li, ui, sh;
};
// pass 2 of g = H x - b with the gradient split, p = gf, the partial sums of (0, |gP|^2, |gc|^2, |gf|^2), QPCFeas(x, p) and X'(y o p)
#define SVM_EU 4
template <int AUG, int SUB, class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_x64_grad(int n, const T *__restrict__ X, const double *__restrict__ y, const double *__restrict__ w, svm_grad_args a)
{
  __shared__ double lds[PMH_BLOCK / 64][64];
  __shared__ double red[PMH_BLOCK / 64];
  const double      sS = AUG ? a.sigma * w[64] : 0.0;
  double            cs[svm_row64<T>::CPL] = {}, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0, m = INFINITY, ts = 0.0;
  svm_sweep_rows64_lanes<SVM_EU, SUB, 1>(
    n, X, y, w, cs,
    [&](long long i, bool act, double ym) {
      svm_grad_row r = {0.0, 0.0, 0.0, -INFINITY, INFINITY, AUG == 1 ? a.shift : 0.0};
      if (act) {
        r.yi = SUB ? ym : y[i], r.xi = a.x_in[i], r.bi = a.b[i];
        if (AUG == 2) r.sh = a.diag[i];
        if (a.lb) r.li = a.lb[i];
        if (a.ub) r.ui = a.ub[i];
      }
      return r;
    },
    [&](long long i, bool act, double sm, svm_grad_row r) {
      const double yi = r.yi, xi = r.xi, bi = r.bi, li = r.li, ui = r.ui, sh = r.sh;
      double       t = 0.0; // y_i p_i: the row's weight in X'(y o p)
      if (act) {
        const double gi = ((SUB && yi == 0.0) ? 0.0 : (AUG ? svm_aug_row(yi, sm, sS, sh, xi) : yi * sm)) - bi;
        double       f, c;
        pmh_box_split_v(xi, gi, li, ui, a.astol, f, c);
        a.g[i] = gi, a.gf[i] = f, a.p[i] = f;
        if (a.x_out) a.x_out[i] = xi;
        const double gPi = f + c;
        acc1 += gPi * gPi, acc2 += c * c, acc3 += f * f;
        m = pmh_box_feas_v(m, xi, f, li, ui);
        t = yi * f;
        if (AUG) ts += t;
      }
      return t;
    });
  svm_fold_cols<T>(cs, lds, a.part_next);
  if (AUG) {
    const double rs = pmh_block_reduce<PMH_RED_SUM>(ts, red);
    if (threadIdx.x == 0) a.spart_next[blockIdx.x] = rs;
  }
  const double z  = pmh_block_reduce<PMH_RED_SUM>(0.0, red);
  const double r1 = pmh_block_reduce<PMH_RED_SUM>(acc1, red), r2 = pmh_block_reduce<PMH_RED_SUM>(acc2, red), r3 = pmh_block_reduce<PMH_RED_SUM>(acc3, red);
  const double rm = pmh_block_reduce<PMH_RED_MIN>(m, red);
  if (threadIdx.x == 0) {
    double *pp = a.partials + (size_t)a.prow * a.ld + blockIdx.x;
    pp[0] = z, pp[a.ld] = r1, pp[2 * (size_t)a.ld] = r2, pp[3 * (size_t)a.ld] = r3;
    a.feas_part[blockIdx.x] = rm;
  }
}

struct svm_p1_args {
  const double *p, *g, *x, *lb, *ub, *afeas;
  double       *Ap, *partials, *x_spec, *part_next;
  double        alpha, astol;
  int           ld, prow;
  // AUG
  double       *spart_next, *aux_part; // aux_part != nullptr: sum_i y_i x_i of the iterate (the one-row equality's B u up to the row's scale)
  double        sigma, shift;
  const double *diag; // AUG 2: the diagonal, in place of shift
};
struct svm_p1_row {
  double yi, pi, gi, xi, li, ui, sh;
};
// pass 2 of Ap = H p with the partial sums of p'Ap, g'p, QPCFeas(x, p); SPEC: + the iterate of the expansion step and X'(y o x+)
template <int SPEC, int AUG, int SUB, class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_x64_p1(int n, const T *__restrict__ X, const double *__restrict__ y, const double *__restrict__ w, svm_p1_args a)
{
  __shared__ double lds[PMH_BLOCK / 64][64];
  __shared__ double red[PMH_BLOCK / 64];
  const double      maf = SPEC ? -(*a.afeas) : 0.0, mal = -a.alpha;
  const double      sS = AUG ? a.sigma * w[64] : 0.0;
  double            cs[svm_row64<T>::CPL] = {}, s0 = 0.0, s1 = 0.0, m = INFINITY, ts = 0.0, sux = 0.0;
  svm_sweep_rows64_lanes<SVM_EU, SUB, SPEC>(
    n, X, y, w, cs,
    [&](long long i, bool act, double ym) {
      svm_p1_row r = {0.0, 0.0, 0.0, 0.0, -INFINITY, INFINITY, AUG == 1 ? a.shift : 0.0};
      if (act) {
        r.yi = SUB ? ym : y[i], r.pi = a.p[i], r.gi = a.g[i], r.xi = a.x[i];
        if (AUG == 2) r.sh = a.diag[i];
        if (a.lb) r.li = a.lb[i];
        if (a.ub) r.ui = a.ub[i];
      }
      return r;
    },
    [&](long long i, bool act, double sm, svm_p1_row r) {
      const double yi = r.yi, pi = r.pi, gi = r.gi, xi = r.xi, li = r.li, ui = r.ui, sh = r.sh;
      double       t = 0.0; // y_i x+_i: the row's weight in X'(y o x+)
      if (act) {
        const double api = (SUB && yi == 0.0) ? 0.0 : (AUG ? svm_aug_row(yi, sm, sS, sh, pi) : yi * sm);
        a.Ap[i] = api;
        if (AUG && (!SUB || yi != 0.0)) sux += yi * xi;
        s0 += pi * api, s1 += gi * pi;
        m = pmh_box_feas_v(m, xi, pi, li, ui);
        if (SPEC) { // k_expansion_std (mpgp.hip) on this entry
          const double xs = xi + maf * pi, gs = gi + maf * api;
          double       f, c;
          pmh_box_split_v(xs, gs, li, ui, a.astol, f, c);
          const double rr = pmh_box_reduced_v(xs, f, li, ui, a.lb != nullptr, a.ub != nullptr, a.alpha), xn = xs + mal * rr;
          a.x_spec[i] = xn;
          t = yi * xn;
          if (AUG) ts += t;
        }
      }
      return t;
    });
  if (SPEC) svm_fold_cols<T>(cs, lds, a.part_next);
  if (AUG) {
    const double rs = pmh_block_reduce<PMH_RED_SUM>(ts, red), ru = pmh_block_reduce<PMH_RED_SUM>(sux, red);
    if (threadIdx.x == 0) {
      if (SPEC) a.spart_next[blockIdx.x] = rs;
      if (a.aux_part) a.aux_part[blockIdx.x] = ru;
    }
  }
  const double r0s = pmh_block_reduce<PMH_RED_SUM>(s0, red), r1s = pmh_block_reduce<PMH_RED_SUM>(s1, red), rm = pmh_block_reduce<PMH_RED_MIN>(m, red);
  if (threadIdx.x == 0) {
    double *pp = a.partials + (size_t)a.prow * a.ld + blockIdx.x;
    pp[0] = r0s, pp[a.ld] = r1s, pp[2 * (size_t)a.ld] = rm;
  }
}

// w[c] = sum over workgroups of part[b][c] (as k_svm_colsum) and, in the last workgroup, afeas = min over workgroups of feas_part (exact: a min has no order)
// spart != nullptr: a 65th column, w[64] = sum over workgroups of spart[b] (the grid then has one workgroup more)
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_colsum_feas(int nblocks, const double *__restrict__ part, double *__restrict__ w, const double *__restrict__ feas_part, double *__restrict__ afeas,
                                                               const double *__restrict__ spart)
{
  __shared__ double red[PMH_BLOCK / 64];
  if (blockIdx.x == gridDim.x - 1) {
    double m = INFINITY;
    for (int b = threadIdx.x; b < nblocks; b += PMH_BLOCK) m = fmin(m, feas_part[b]);
    m = pmh_block_reduce<PMH_RED_MIN>(m, red);
    if (threadIdx.x == 0) *afeas = m;
    return;
  }
  svm_colsum(nblocks, 64, part, w, spart);
}

// Gu[0] = c sum_b part[b], its square -> the scalar slot (device + pinned host): ||B u||^2 of the one-row equality with row c y.  One workgroup, fixed order
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_aux_finish(int nb, const double *__restrict__ part, double c, double *__restrict__ Gu, double *__restrict__ dslot, double *__restrict__ hslot)
{
  __shared__ double red[PMH_BLOCK / 64];
  double            v = 0.0;
  for (int b = threadIdx.x; b < nb; b += PMH_BLOCK) v += part[b];
  v = pmh_block_reduce<PMH_RED_SUM>(v, red);
  if (threadIdx.x == 0) {
    const double bu = c * v;
    Gu[0] = bu, *dslot = bu * bu, *hslot = bu * bu;
  }
}
int SvmDualOp::aux_finish(int nb)
{
  hipLaunchKernelGGL(k_svm_aux_finish, dim3(1), dim3(PMH_BLOCK), 0, ctx->stream, nb, (const double *)aux_part, aux_c, aux_Gu, ctx->d_scal + aux_slot, ctx->h_scal + aux_slot);
  PMH_HIP(hipGetLastError());
  aux_done = 1;
  return PMH_SUCCESS;
}
// the armed ||B u|| request can ride on this product: the augmented kernels, one GPU, the buffer at hand
static int svm_aux_ready(SvmDualOp *o, bool aug, bool *ok)
{
  *ok = o->aux_u && aug && !pmh_comm_on(o->ctx) && o->aux_Gu && o->aux_slot >= 0;
  if (*ok && !o->aux_part) PMH_CHK(pmh_malloc(o->ctx, sizeof(double) * PMH_MAX_VEC_BLOCKS, (void **)&o->aux_part));
  return PMH_SUCCESS;
}

// pass 1 and the column sums: w = X'(y o v) and, augmented, w[d] = s = sum_i y_i v_i (+ sum_i y_i u_i -> upart[workgroup] where u is given).  The plain form
// hands the AUG = 0 kernels null pointers: the kernels of the plain operator, the bits of the plain operator
int SvmDualOp::pass1(const double *v, bool aug, const double *u, double *upart)
{
  double       *sp = aug ? spart : nullptr;
  const double *y  = yk(); // (the masked labels under a subset, with the SUB kernels)
  // d == 64: rows in flight per wave-instruction group: 2 x UNR rows of 512 B (16-byte loads, UNR of them outstanding per lane).  UNR decides which wave visits
  // which rows, i.e. the summation order of pass 1 (last-digit differences between UNR values; fixed for a given UNR).  Measured 4 / 8 / 12 / 16 on configs[4]:
  // 464 / 452-488 / 433 / 487 iterations per second -- inside the run-to-run spread of the box (the two passes already stream X at the box's copy rate): 4 stays,
  // and only that instance is compiled
  // float samples: 4 x UNR rows of 256 B, the same 16-byte loads and the same bytes in flight per lane.  UNR = 4 there too, the one instance compiled: a
  // wave's group is 16 rows, which is what a wave gets of the grid below the cap (64 rows per workgroup)
  svm_pick<2>(aug, ym != nullptr, f32, [&](auto A, auto S, auto F) {
    constexpr int AUG = decltype(A)::value, SUB = decltype(S)::value;
    using T           = svm_sample_t<decltype(F)>;
    if (d == 64) SVM_PASS((k_svm_xt64<4, AUG, SUB, T>), dim3(nblocks), dim3(PMH_BLOCK), 0, ctx->stream, n, (const T *)X, y, v, part, sp, u, upart);
    else SVM_PASS((k_svm_xt<AUG, SUB, T>), dim3(nblocks), dim3(PMH_BLOCK), 0, ctx->stream, n, d, (const T *)X, y, v, part, sp, u, upart);
  });
  return pmh_svm_colsum(ctx, nblocks, d, part, w, sp);
}
// pass 2: out_i = y_i (x_i . w), augmented + (sigma + sigma_fold) w[d] y_i + shift a_i (or + diag_i a_i)
int SvmDualOp::pass2(const double *a, double *out, bool aug)
{
  const double *ap = aug ? a : nullptr;
  const double  sg = aug ? sigma + sigma_fold : 0.0, sh = aug ? shift : 0.0;
  const int     form = aug ? aug_form() : 0;
  const double *y    = yk();
  svm_pick<3>(form, ym != nullptr, f32, [&](auto A, auto S, auto F) {
    constexpr int AUG = decltype(A)::value, SUB = decltype(S)::value;
    using T           = svm_sample_t<decltype(F)>;
    if (d == 64) SVM_PASS((k_svm_x64<4, AUG, SUB, T>), dim3(nblocks), dim3(PMH_BLOCK), 0, ctx->stream, n, (const T *)X, y, (const double *)w, out, ap, sg, sh, diag);
    else SVM_PASS((k_svm_x<AUG, SUB, T>), dim3(nblocks), dim3(PMH_BLOCK), 0, ctx->stream, n, d, (const T *)X, y, (const double *)w, out, ap, sg, sh, diag);
  });
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

int SvmDualOp::mult_epi(const double *in, double *out, const pmh_vec_epi &e)
{
  // (the switch may change between two solves of one process: pmh_set_knob("svm_pairing"), initial value from PMH_SVM_NO_PAIRING -- no getenv on the
  // per-product path.  It is process-wide state that every rank of a job must set alike: ranks that disagree would issue different sequences of collectives)
  if (n <= 0 && pmh_comm_on(ctx)) return pmh_set_error(PMH_ERR_ARG, "SVM dual operator: this rank holds no samples; with a communicator every rank needs at least one row (an empty shard would skip the collectives the other ranks issue)");
  if (!pmh_knobs().svm_pairing || d != 64 || n <= 0) return PMH_EPI_UNSUPPORTED;
  // several GPUs (samples sharded by rows): the 64 column sums w and, where the next pass uses it, the feasible step length afeas are completed across the
  // ranks between the passes -- the same exchange step as the lone application's, one (+ one 8-byte MIN) per pass
  if (!part_next) {
    grid_epi = pmh_vec_grid(n); // one partial sum per workgroup, where pmh_finalize_partials expects them
    PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)grid_epi * 64, (void **)&part_next));
    PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)grid_epi, (void **)&feas_part));
    PMH_CHK(pmh_malloc(ctx, sizeof(double), (void **)&d_afeas));
    PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)n, (void **)&x_spec));
    PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)grid_epi, (void **)&spart_next));
  }
  // the augmented forms (shift or diagonal / rank-one term): the same launches with the 65th column sum s = sum_i y_i v_i beside the 64 of w
  const bool    AG  = aug();
  const int     form = aug_form();
  const double  sg  = sigma + sigma_fold;
  const double *spn = AG ? spart_next : nullptr;
  const size_t  nw  = AG ? 65 : 64;
  const double *y   = yk();
  int           have = next_is;
  if (next_aug != AG) have = NEXT_NONE; // (sums prepared by the other form lack / carry the 65th column)
  next_is  = NEXT_NONE;
  next_aug = AG;
  // w (+ s) of `v`: from the sums the previous pass 2 left (prepared) or by pass 1
  auto form_w = [&](bool prepared, const double *v) -> int {
    if (prepared) {
      hipLaunchKernelGGL(k_svm_colsum_feas, dim3(AG ? 18 : 17), dim3(PMH_BLOCK), 0, ctx->stream, grid_epi, (const double *)part_next, w, (const double *)feas_part, d_afeas, spn);
      PMH_HIP(hipGetLastError());
    } else PMH_CHK(pass1(v, AG, nullptr, nullptr));
    return pmh_comm_allreduce_sum(ctx, w, nw);
  };
  if (e.kind == PMH_VEPI_GRAD_SPLIT) {
    const bool spec = e.x_from_spec && have == NEXT_XSPEC;
    if (e.x_from_spec && !spec) return pmh_set_error(PMH_ERR_STATE, "SVM dual operator: the driver asks for the prepared expansion step, none is prepared");
    // (the min the prepared form also takes is not used here)
    PMH_CHK(form_w(spec, in));
    svm_grad_args a;
    a.b = e.b, a.x_in = spec ? (const double *)x_spec : in, a.lb = e.lb, a.ub = e.ub, a.x_out = spec ? e.x_out : nullptr, a.g = out, a.gf = e.gf, a.p = e.p;
    a.partials = e.partials, a.feas_part = feas_part, a.part_next = part_next, a.astol = e.astol, a.ld = e.ld, a.prow = e.prow;
    a.spart_next = spart_next, a.sigma = sg, a.shift = shift, a.diag = diag;
    if (spec && !e.x_out) return pmh_set_error(PMH_ERR_ARG, "SVM dual operator: x_from_spec needs x_out");
    svm_pick<3>(form, ym != nullptr, f32, [&](auto A, auto S, auto F) {
      using T = svm_sample_t<decltype(F)>;
      SVM_PASS((k_svm_x64_grad<decltype(A)::value, decltype(S)::value, T>), dim3(grid_epi), dim3(PMH_BLOCK), 0, ctx->stream, n, (const T *)X, y, (const double *)w, a);
    });
    PMH_HIP(hipGetLastError());
    next_is = NEXT_P, next_p = e.p;
    return PMH_SUCCESS;
  }
  if (e.kind == PMH_VEPI_P1) {
    const bool paired = e.p_fresh && have == NEXT_P && next_p == in;
    PMH_CHK(form_w(paired, in));
    if (paired) PMH_CHK(pmh_comm_allreduce_min(ctx, d_afeas, 1)); // the P1 pass forms the expansion iterate with it (k_svm_x64_p1<1>)
    // the one-row equality's ||B u|| for the iterate this pass holds in registers
    bool aux = false;
    PMH_CHK(svm_aux_ready(this, AG, &aux));
    aux = aux && aux_u == e.xx;
    svm_p1_args a;
    a.p = in, a.g = e.g, a.x = e.xx, a.lb = e.lb, a.ub = e.ub, a.afeas = d_afeas, a.Ap = out, a.partials = e.partials, a.x_spec = x_spec, a.part_next = part_next;
    a.alpha = e.spec_alpha, a.astol = e.astol, a.ld = e.ld, a.prow = e.prow;
    a.spart_next = spart_next, a.aux_part = aux ? aux_part : nullptr, a.sigma = sg, a.shift = shift, a.diag = diag;
    const bool spec = paired && e.spec_alpha > 0.0; // afeas is known before this pass only when the gradient pass computed it
    svm_pick<3>(form, ym != nullptr, f32, [&](auto A, auto S, auto F) {
      using T = svm_sample_t<decltype(F)>;
      svm_const<2>(spec, [&](auto P) { SVM_PASS((k_svm_x64_p1<decltype(P)::value, decltype(A)::value, decltype(S)::value, T>), dim3(grid_epi), dim3(PMH_BLOCK), 0, ctx->stream, n, (const T *)X, y, (const double *)w, a); });
    });
    PMH_HIP(hipGetLastError());
    if (aux) PMH_CHK(aux_finish(grid_epi));
    if (spec) next_is = NEXT_XSPEC;
    return PMH_SUCCESS;
  }
  return PMH_EPI_UNSUPPORTED;
}

int SvmDualOp::mult(const double *a, double *Ha)
{
  next_is = NEXT_NONE; // (whatever was prepared belonged to the MPGP driver's vectors)
  if (n == 0 && pmh_comm_on(ctx)) return pmh_set_error(PMH_ERR_ARG, "SVM dual operator: this rank holds no samples; with a communicator every rank needs at least one row");
  if (n == 0) return PMH_SUCCESS;
  const bool AG  = aug();
  bool       aux = false;
  PMH_CHK(svm_aux_ready(this, AG, &aux));
  PMH_CHK(pass1(a, AG, aux ? aux_u : nullptr, aux ? aux_part : nullptr));
  if (aux) PMH_CHK(aux_finish(nblocks));
  PMH_CHK(pmh_comm_allreduce_sum(ctx, w, (size_t)d + (AG ? 1 : 0))); // samples sharded over GPUs: the one exchange step
  return pass2(a, Ha, AG);
}

// w = X'(y o a) by pass 1 alone, always the plain form (the model of a trained SVM)
int SvmDualOp::form_w(const double *a, const double **w_dev)
{
  next_is = NEXT_NONE;
  if (n > 0) PMH_CHK(pass1(a, false, nullptr, nullptr));
  else PMH_CHK(pmh_memset(ctx, w, 0, sizeof(double) * (size_t)d));
  PMH_CHK(pmh_comm_allreduce_sum(ctx, w, (size_t)d));
  *w_dev = w;
  return PMH_SUCCESS;
}

// how many entries of row differ from c y (c = row_i0 / y_i0): 0 <=> the row is c y, entry by entry, to the rounding of one multiplication.  Under a subset y
// holds the masked labels and i0 is a sample of the subset; a zero entry of the row against a zero label is a match
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_row_vs_labels(int n, const double *__restrict__ row, const double *__restrict__ y, int *__restrict__ bad, int i0)
{
  const double c = row[i0] / y[i0];
  int          b = 0;
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) b += fabs(row[i] - c * y[i]) > 4.0 * 2.220446049250313e-16 * fabs(row[i]) ? 1 : 0;
  if (b) atomicAdd(bad, b); // (a count of mismatches: any order gives the same integer)
}
// Under a communicator the answer is joined: every rank takes part in ONE all-reduce of (mismatches, ranks that hold rows, sum of c, sum of c^2), so all ranks
// decide alike (ranks that disagreed would issue different collectives afterwards) and c must be the same on every rank that holds rows
int pmh_svm_op_row_is_labels(SvmDualBase *o, pmh_qppf pf, double *c)
{
  if (!pf->onerow) return 0;
  pmh_ctx ctx = o->ctx;
  double  h[4] = {0.0, 0.0, 0.0, 0.0}; // mismatches (or: this rank cannot tell), holds rows, c, c^2
  if (pf->n != o->n) h[0] = 1.0;
  else if (o->n > 0 && !(o->ym && o->n_sub == 0)) { // (a rank whose samples are all held out has no say, as one without rows)
    const double *yk = o->yk();
    const int     i0 = o->ym ? o->sub_first : 0;
    int *d_bad = nullptr, bad = 1;
    double r0 = 0.0, y0 = 0.0;
    int rc = pmh_malloc(ctx, sizeof(int), (void **)&d_bad);
    if (!rc) rc = pmh_memset(ctx, d_bad, 0, sizeof(int));
    if (!rc) {
      hipLaunchKernelGGL(k_svm_row_vs_labels, dim3(pmh_vec_grid(o->n)), dim3(PMH_BLOCK), 0, ctx->stream, o->n, pf->row, yk, d_bad, i0);
      rc = (hipGetLastError() != hipSuccess) || pmh_memcpy_d2h(ctx, &bad, d_bad, sizeof(int)) || pmh_memcpy_d2h(ctx, &r0, pf->row + i0, sizeof(double)) || pmh_memcpy_d2h(ctx, &y0, yk + i0, sizeof(double));
    }
    if (d_bad) pmh_free(ctx, d_bad);
    if (rc || bad || y0 == 0.0 || r0 == 0.0) h[0] = 1.0;
    else h[1] = 1.0, h[2] = r0 / y0, h[3] = h[2] * h[2];
  }
  if (pmh_comm_sum_host(ctx, h, 4)) return 0;
  if (pmh_comm_on(ctx) && h[0] == 0.0 && h[1] > 0.0) {
    const double mean = h[2] / h[1];
    if (fabs(h[3] - h[1] * mean * mean) > 8.0 * 2.220446049250313e-16 * h[3]) return 0; // the ranks' c differ
    h[2] = mean;
  }
  if (h[0] != 0.0 || h[1] == 0.0) return 0;
  *c = h[2];
  return 1;
}

extern "C" int pmh_op_svm_dual_set_terms(pmh_op op, double shift, double sigma)
{
  SvmDualBase *o = dynamic_cast<SvmDualBase *>(op);
  PMH_ARG(o && shift >= 0.0 && sigma >= 0.0);
  if (shift != 0.0 && o->diag) return pmh_set_error(PMH_ERR_ARG, "pmh_op_svm_dual_set_terms: shift = %g while a diagonal is set (pmh_op_svm_dual_set_diag): the operator carries a scalar shift or a diagonal, not both", shift);
  o->shift = shift, o->sigma = sigma;
  o->terms_changed();
  return PMH_SUCCESS;
}

extern "C" int pmh_op_svm_dual_set_diag(pmh_op op, const double *diag_dev)
{
  SvmDualBase *o = dynamic_cast<SvmDualBase *>(op);
  PMH_ARG(o);
  if (diag_dev && o->shift != 0.0) return pmh_set_error(PMH_ERR_ARG, "pmh_op_svm_dual_set_diag: a diagonal while shift = %g is set (pmh_op_svm_dual_set_terms): the operator carries a scalar shift or a diagonal, not both", o->shift);
  o->diag = diag_dev;
  o->terms_changed();
  return PMH_SUCCESS;
}

// ---- sample subsets ----------------------------------------------------------------------------------------------------------------------------------------
// st[0]: entries of m that are neither 0 nor 1 (a NaN is one), st[1]: ones, st[2]: the index of the first one (n: none).  Integer counts and a minimum: any
// order gives the same integers
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_mask_stats(int n, const double *__restrict__ m, int *__restrict__ st)
{
  int bad = 0, ones = 0, first = n;
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    const double mi = m[i];
    if (mi == 1.0) ones++, first = min(first, (int)i);
    else if (!(mi == 0.0)) bad++;
  }
  if (bad) atomicAdd(st, bad);
  if (ones) atomicAdd(st + 1, ones), atomicMin(st + 2, first);
}
// msk = m (m != nullptr: the new mask; nullptr: msk stays) and ym_i = msk_i != 0 ? y_i : +0
__global__ __launch_bounds__(PMH_BLOCK) void k_svm_mask_labels(int n, const double *__restrict__ m, const double *__restrict__ y, double *__restrict__ msk, double *__restrict__ ym)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * PMH_BLOCK) {
    const double mi = m ? m[i] : msk[i];
    if (m) msk[i] = mi != 0.0 ? 1.0 : 0.0;
    ym[i] = mi != 0.0 ? y[i] : 0.0;
  }
}
int SvmDualBase::refresh_ym()
{
  if (!msk || n <= 0) return PMH_SUCCESS;
  hipLaunchKernelGGL(k_svm_mask_labels, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, (const double *)nullptr, y, msk, ym);
  PMH_HIP(hipGetLastError());
  return PMH_SUCCESS;
}

int pmh_svm_check_mask(pmh_ctx ctx, const char *who, int n, const double *m_dev, long long *ones, int *first)
{
  // every rank decides alike: the counts are summed over the communicator before anything is changed
  int  h[3] = {0, 0, n};
  int *d_st = nullptr;
  PMH_CHK(pmh_malloc(ctx, sizeof(h), (void **)&d_st));
  int rc = pmh_memcpy_h2d(ctx, d_st, h, sizeof(h));
  if (!rc && n > 0) {
    hipLaunchKernelGGL(k_svm_mask_stats, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, m_dev, d_st);
    if (hipGetLastError() != hipSuccess) rc = pmh_set_error(PMH_ERR_HIP, "%s: the launch that checks the mask failed", who);
  }
  if (!rc) rc = pmh_memcpy_d2h(ctx, h, d_st, sizeof(h));
  pmh_free(ctx, d_st);
  PMH_CHK(rc);
  double tot[2] = {(double)h[0], (double)h[1]};
  PMH_CHK(pmh_comm_sum_host(ctx, tot, 2));
  if (tot[0] != 0.0) return pmh_set_error(PMH_ERR_ARG, "%s: %lld entries of the mask are neither 0 nor 1", who, (long long)tot[0]);
  if (tot[1] == 0.0) return pmh_set_error(PMH_ERR_ARG, "%s: the mask holds no sample (all zero)", who);
  *ones = h[1], *first = h[1] ? h[2] : 0;
  return PMH_SUCCESS;
}

extern "C" int pmh_op_svm_dual_set_subset(pmh_op op, const double *m_dev)
{
  SvmDualBase *o = dynamic_cast<SvmDualBase *>(op);
  PMH_ARG(o);
  if (o->doubled()) return pmh_set_error(PMH_ERR_SUP, "pmh_op_svm_dual_set_subset: the regression operator (pmh_op_create_svr_dual) takes no sample subset");
  pmh_ctx   ctx = o->ctx;
  const int n   = o->n;
  if (!m_dev) {
    if (o->msk) pmh_free(ctx, o->msk), pmh_free(ctx, o->ym);
    o->msk = o->ym = nullptr, o->n_sub = 0, o->sub_first = 0;
    o->terms_changed();
    return PMH_SUCCESS;
  }
  long long ones  = 0;
  int       first = 0, rc;
  PMH_CHK(pmh_svm_check_mask(ctx, "pmh_op_svm_dual_set_subset", n, m_dev, &ones, &first));
  if (!o->msk) {
    const size_t nb = sizeof(double) * (size_t)(n ? n : 1);
    PMH_CHK(pmh_malloc(ctx, nb, (void **)&o->msk));
    if ((rc = pmh_malloc(ctx, nb, (void **)&o->ym))) {
      pmh_free(ctx, o->msk), o->msk = nullptr;
      return rc;
    }
  }
  if (n > 0) {
    hipLaunchKernelGGL(k_svm_mask_labels, dim3(pmh_vec_grid(n)), dim3(PMH_BLOCK), 0, ctx->stream, n, m_dev, o->y, o->msk, o->ym);
    PMH_HIP(hipGetLastError());
  }
  o->n_sub = ones, o->sub_first = first;
  o->terms_changed();
  return PMH_SUCCESS;
}

extern "C" int pmh_op_svm_dual_set_labels(pmh_op op, const double *y_dev)
{
  SvmDualBase *o = dynamic_cast<SvmDualBase *>(op);
  PMH_ARG(o && y_dev);
  return o->set_labels(y_dev);
}

extern "C" int pmh_op_svm_dual_passes(pmh_op op, long long *passes)
{
  SvmDualBase *o = dynamic_cast<SvmDualBase *>(op);
  PMH_ARG(o && passes);
  *passes = o->npass;
  return PMH_SUCCESS;
}

// X_dev: n_local x d doubles, or floats where f32
static int svm_dual_create(pmh_ctx ctx, int n_local, int d, const void *X_dev, int f32, const double *y_dev, pmh_op *op)
{
  PMH_ARG(ctx && op && n_local >= 0 && d >= 1 && d <= 64 * SVM_KMAX && X_dev && y_dev);
  SvmDualOp *o = new SvmDualOp();
  o->ctx       = ctx;
  o->n         = n_local;
  o->d         = d;
  o->X         = X_dev;
  o->f32       = f32;
  o->y         = y_dev;
  long long nb = ((long long)n_local + 4 * 16 - 1) / (4 * 16); // >= 16 rows per wavefront
  o->nblocks   = (int)(nb < 1 ? 1 : (nb > PMH_MAX_VEC_BLOCKS ? PMH_MAX_VEC_BLOCKS : nb));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * ((size_t)d + 1), (void **)&o->w)); // (w[d]: s = sum_i y_i v_i of the augmented forms)
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)o->nblocks * d, (void **)&o->part));
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * (size_t)o->nblocks, (void **)&o->spart));
  *op = o;
  return PMH_SUCCESS;
}
extern "C" int pmh_op_create_svm_dual(pmh_ctx ctx, int n_local, int d, const double *X_dev, const double *y_dev, pmh_op *op) { return svm_dual_create(ctx, n_local, d, X_dev, 0, y_dev, op); }
extern "C" int pmh_op_create_svm_dual_f32(pmh_ctx ctx, int n_local, int d, const float *X_dev, const double *y_dev, pmh_op *op) { return svm_dual_create(ctx, n_local, d, X_dev, 1, y_dev, op); }
