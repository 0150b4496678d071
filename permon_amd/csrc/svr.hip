// The dual Hessian of epsilon-insensitive support vector regression on u = [p; q] (2 n doubles), matrix-free:
//   H^ = [ Q + D, -Q; -Q, Q + D ],  Q = X X',  D = shift I or diag(diag)   (+ sigma e e', e = [1; -1]: the penalised bias equality sum (p_i - q_i) = 0)
// which is the classification dual of svm.hip on the doubled samples [X; X] with labels [+1; -1].  Posed that way X is stored twice and streamed four times
// per product; here it is kept once and streamed twice, as classification streams it:
//   pass 1  w = X's, s_i = p_i - q_i formed in registers where the classification kernel forms y_i a_i (augmented: S = sum_i s_i travels as w[d]);
//   the column sums (k_svm_colsum, svm.hip) and, under a communicator, the all-reduce of w (d or d + 1 doubles: samples shard by rows);
//   pass 2  out_p[i] = (x_i . w + sigma S) + D_i p_i,  out_q[i] = (-(x_i . w) - sigma S) + D_i q_i: both halves of row i from the one dot product -- svm_aug_row
//           with the labels +1 and -1, so with the same w the bits are the classification operator's on the doubled samples.
// Three launches, no n-vector s or X w through memory.  Algorithmic bytes per product: 2 * 8 n d of X (float32 samples: 2 * 4 n d) + 48 n (p, q read twice, both
// halves written; + 8 n with a diagonal) against 4 * 8 n d + 80 n of the doubled classification operator.  The row loops are those of svm_rows.h; the summation
// orders are fixed (no float atomics): two products give the same bits, and the float instances for d != 64 give the bits of the double ones on the widened
// samples.  Samples in CSR: the entry-balanced sweeps of svm_csr.hip over X with all labels +1 (SvrCsrOp below).
// A sample subset S (pmh_op_svr_dual_set_subset, mask m): out = M^ H^ M^ u + sigma (e^'u) e^, M^ = diag([m; m]), e^ = [m; -m].  The SUB = 1 instances of the four
// dense kernels read m_i first and issue no load of a held-out row of X, nor of its p_i, q_i, diag_i; its two results are +0.  SUB = 0: the kernels as they were.
// No fused MPGP epilogues (mult_epi declines, MPGP takes its unfused path).
#include "pmh_internal.h"
#include "reduce.h"

#include "svr_internal.h"
#include "svm_rows.h"

// pass 1, any d: k_svm_xt's row loop with the row's weight s_i = p_i - q_i; AUG: also S = sum_i s_i -> spart[workgroup]
// SUB: m_i is read first (uniform over the wave) and a held-out row is skipped: it adds to no sum, whatever p_i and q_i hold
template <int AUG, int SUB, class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_xt(int n, int d, const T *__restrict__ X, const double *__restrict__ p, const double *__restrict__ q, double *__restrict__ part, double *__restrict__ spart,
                                                      const double *__restrict__ m)
{
  __shared__ double lds[PMH_BLOCK / 64][64 * SVM_KMAX];
  __shared__ double sred[AUG ? PMH_BLOCK / 64 : 1];
  double            as = 0.0;
  const int         lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long   gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  double            acc[SVM_KMAX];
#pragma unroll
  for (int k = 0; k < SVM_KMAX; k++) acc[k] = 0.0;
  for (long long i = gw; i < n; i += nw) {
    if (SUB && m[i] == 0.0) continue;
    const double s  = p[i] - q[i];
    const T     *xr = X + (size_t)i * d;
    if (AUG) as += s;
#pragma unroll
    for (int k = 0; k < SVM_KMAX; k++) {
      const int c = lane + 64 * k;
      if (c < d) acc[k] += s * (double)__builtin_nontemporal_load(&xr[c]);
    }
  }
  if (AUG && lane == 0) sred[wave] = as;
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
    double v0 = sred[0];
#pragma unroll
    for (int wv = 1; wv < PMH_BLOCK / 64; wv++) v0 += sred[wv];
    spart[blockIdx.x] = v0;
  }
}

// pass 1 for d = 64: k_svm_xt64's row loop (every lane that holds a part of row i needs s_i), the layouts of svm_row64<T>, then svm_fold_cols
// SUB: the mask of the RPI UNR rows in flight comes in ONE coalesced load and a ballot (svm_live_rows64); a held-out row is not loaded (svm_load_rows64<UNR, 1>)
// and s_i = m_i ? p_i - q_i : 0, a selection: p_i and q_i of a held-out row are not read
template <int UNR, int AUG, int SUB, class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_xt64(int n, const T *__restrict__ X, const double *__restrict__ p, const double *__restrict__ q, double *__restrict__ part, double *__restrict__ spart,
                                                        const double *__restrict__ m)
{
  typedef svm_row64<T> R;
  __shared__ double lds[PMH_BLOCK / 64][64];
  __shared__ double red[PMH_BLOCK / 64];
  double            as = 0.0; // AUG: sum_i s_i, taken by the first of the LPR lanes of a row for its rows
  const int         lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / R::LPR, lq = lane & (R::LPR - 1);
  const long long   gw = (long long)blockIdx.x * (PMH_BLOCK / 64) + wave, nw = (long long)gridDim.x * (PMH_BLOCK / 64);
  double            acc[R::CPL];
#pragma unroll
  for (int c = 0; c < R::CPL; c++) acc[c] = 0.0;
  for (long long r0 = gw * R::RPI * UNR; r0 < n; r0 += nw * R::RPI * UNR) {
    typename R::vec v[UNR];
    double          s[UNR];
    if constexpr (SUB) {
      double                   mi;
      const unsigned long long live = svm_live_rows64<R::RPI * UNR>(n, m, r0, mi);
      svm_load_rows64<UNR, 1>(n, X, r0, v, live);
      const unsigned lh = (unsigned)(live >> sub); // bit RPI u: this lane's row of group u (shifted once: a shift per u costs registers, as in svm_load_rows64)
#pragma unroll
      for (int u = 0; u < UNR; u++) {
        const long long i = r0 + R::RPI * u + sub;
        s[u] = ((lh >> (R::RPI * u)) & 1) ? p[i] - q[i] : 0.0; // (a live row is a row below n)
        if (AUG && lq == 0) as += s[u];
      }
    } else {
#pragma unroll
      for (int u = 0; u < UNR; u++) {
        const long long i  = r0 + R::RPI * u + sub;
        const bool      ok = i < n;
        v[u] = ok ? __builtin_nontemporal_load((const typename R::vec *)(X + (size_t)i * 64) + lq) : R::zero();
        s[u] = ok ? p[i] - q[i] : 0.0;
        if (AUG && lq == 0) as += s[u];
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; u++) {
#pragma unroll
      for (int c = 0; c < R::CPL; c++) acc[c] += s[u] * R::col(v[u], c);
    }
  }
  svm_fold_cols<T>(acc, lds, part);
  if (AUG) {
    const double r = pmh_block_reduce<PMH_RED_SUM>(as, red);
    if (threadIdx.x == 0) spart[blockIdx.x] = r;
  }
}

// what pass 2 does with row i's dot product: both halves.  AUG 0: +-dot; 1: the scalar shift; 2: diag_i
// SUB: the sweeps hand a held-out row over with dot = 0; the row is recognised here by m_i == 0 and both halves are +0, p_i, q_i and diag_i unread
struct svr_row_out {
  const double *p, *q, *diag;
  double       *op, *oq;
  double        sS, shift;
  const double *m; // SUB: the mask
};
template <int AUG, int SUB> static __device__ __forceinline__ void svr_store_row(const svr_row_out &o, long long i, double dot)
{
  if (SUB && o.m[i] == 0.0) {
    o.op[i] = 0.0, o.oq[i] = 0.0;
    return;
  }
  if (AUG == 0) {
    o.op[i] = dot, o.oq[i] = -dot;
    return;
  }
  const double D = AUG == 2 ? o.diag[i] : o.shift;
  o.op[i] = svm_aug_row(1.0, dot, o.sS, D, o.p[i]);
  o.oq[i] = svm_aug_row(-1.0, dot, o.sS, D, o.q[i]);
}
template <int AUG, int SUB, class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_x(int n, int d, const T *__restrict__ X, const double *__restrict__ w, svr_row_out o, double sigma)
{
  o.sS = AUG ? sigma * w[d] : 0.0;
  svm_sweep_rows<SUB>(n, d, X, w, [&](long long i, double dot) { svr_store_row<AUG, SUB>(o, i, dot); }, o.m);
}
template <int UNR, int AUG, int SUB, class T>
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_x64(int n, const T *__restrict__ X, const double *__restrict__ w, svr_row_out o, double sigma)
{
  o.sS = AUG ? sigma * w[64] : 0.0;
  svm_sweep_rows64<UNR, SUB>(n, X, w, [&](long long i, double dot) { svr_store_row<AUG, SUB>(o, i, dot); }, o.m);
}

__global__ __launch_bounds__(PMH_BLOCK) void k_svr_labels(int nl, double *__restrict__ yy)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < nl; i += (long long)gridDim.x * PMH_BLOCK) yy[i] = 1.0, yy[nl + i] = -1.0;
}
int SvrDualBase::init_labels()
{
  PMH_CHK(pmh_malloc(ctx, sizeof(double) * 2 * (size_t)(nl ? nl : 1), (void **)&yy));
  if (nl > 0) hipLaunchKernelGGL(k_svr_labels, dim3(pmh_vec_grid(nl)), dim3(PMH_BLOCK), 0, ctx->stream, nl, yy);
  PMH_HIP(hipGetLastError());
  y = yy;
  return PMH_SUCCESS;
}

// ym = [m; -m] with m_i -> 1 or +0: +0 in both halves of a held-out sample
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_mask_labels(int nl, const double *__restrict__ m, double *__restrict__ ym)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < nl; i += (long long)gridDim.x * PMH_BLOCK) {
    const bool in = m[i] != 0.0;
    ym[i] = in ? 1.0 : 0.0, ym[nl + i] = in ? -1.0 : 0.0;
  }
}
int SvrDualBase::take_mask(const double *m_dev, long long ones, int first)
{
  if (!m_dev) {
    if (ym) pmh_free(ctx, ym);
    msk = ym = nullptr, n_sub = 0, sub_first = 0;
    return PMH_SUCCESS;
  }
  if (!ym) PMH_CHK(pmh_malloc(ctx, sizeof(double) * 2 * (size_t)(nl ? nl : 1), (void **)&ym));
  msk = ym;
  if (nl > 0) hipLaunchKernelGGL(k_svr_mask_labels, dim3(pmh_vec_grid(nl)), dim3(PMH_BLOCK), 0, ctx->stream, nl, m_dev, ym);
  PMH_HIP(hipGetLastError());
  n_sub = ones, sub_first = first;
  return PMH_SUCCESS;
}

int SvrDualBase::maxeig_start(double *v)
{
  PMH_CHK(pmh_vec_set(ctx, nl, v, 1.0));
  return pmh_memset(ctx, v + nl, 0, sizeof(double) * (size_t)nl);
}

static const char *const svr_empty_rank = "SVR dual operator: this rank holds no samples; with a communicator every rank needs at least one row";

struct SvrDualOp : SvrDualBase {
  const void *X;       // nl x d row-major, borrowed: doubles, or floats where f32
  int         f32 = 0;
  double     *w = nullptr, *part = nullptr, *spart = nullptr; // [d + 1], [nblocks][d], [nblocks]
  int         nblocks = 1;
  // w = X'(p - q) (+ w[d] = sum (p_i - q_i)) of u = [p; q]: pass 1, the column sums, the all-reduce
  int pass1(const double *u, bool aug)
  {
    svm_pick<2>(aug, ym != nullptr, f32, [&](auto A, auto S, auto F) {
      constexpr int AUG = decltype(A)::value, SUB = decltype(S)::value;
      using T           = svm_sample_t<decltype(F)>;
      // (d == 64: UNR = 4, the one instance compiled, as in SvmDualOp::pass1)
      if (d == 64) SVM_PASS((k_svr_xt64<4, AUG, SUB, T>), dim3(nblocks), dim3(PMH_BLOCK), 0, ctx->stream, nl, (const T *)X, u, u + nl, part, spart, (const double *)msk);
      else SVM_PASS((k_svr_xt<AUG, SUB, T>), dim3(nblocks), dim3(PMH_BLOCK), 0, ctx->stream, nl, d, (const T *)X, u, u + nl, part, spart, (const double *)msk);
    });
    PMH_CHK(pmh_svm_colsum(ctx, nblocks, d, part, w, aug ? spart : nullptr));
    return pmh_comm_allreduce_sum(ctx, w, (size_t)d + (aug ? 1 : 0)); // samples sharded over GPUs: the one exchange step
  }
  int mult(const double *u, double *out) override
  {
    if (nl == 0 && pmh_comm_on(ctx)) return pmh_set_error(PMH_ERR_ARG, "%s", svr_empty_rank);
    if (nl == 0) return PMH_SUCCESS;
    const bool AG = aug();
    PMH_CHK(pass1(u, AG));
    svr_row_out o{u, u + nl, diag, out, out + nl, 0.0, shift, msk};
    const double sg = sigma + sigma_fold;
    svm_pick<3>(aug_form(), ym != nullptr, f32, [&](auto A, auto S, auto F) {
      constexpr int AUG = decltype(A)::value, SUB = decltype(S)::value;
      using T           = svm_sample_t<decltype(F)>;
      if (d == 64) SVM_PASS((k_svr_x64<4, AUG, SUB, T>), dim3(nblocks), dim3(PMH_BLOCK), 0, ctx->stream, nl, (const T *)X, (const double *)w, o, sg);
      else SVM_PASS((k_svr_x<AUG, SUB, T>), dim3(nblocks), dim3(PMH_BLOCK), 0, ctx->stream, nl, d, (const T *)X, (const double *)w, o, sg);
    });
    PMH_HIP(hipGetLastError());
    return PMH_SUCCESS;
  }
  int mult_epi(const double *, double *, const pmh_vec_epi &) override
  {
    if (nl <= 0 && pmh_comm_on(ctx)) return pmh_set_error(PMH_ERR_ARG, "%s", svr_empty_rank);
    return PMH_EPI_UNSUPPORTED;
  }
  int form_w(const double *u, const double **w_dev) override
  {
    if (nl > 0) PMH_CHK(pass1(u, false));
    else {
      PMH_CHK(pmh_memset(ctx, w, 0, sizeof(double) * (size_t)d));
      PMH_CHK(pmh_comm_allreduce_sum(ctx, w, (size_t)d));
    }
    *w_dev = w;
    return PMH_SUCCESS;
  }
  int row_dots(const double *, double *) override { return pmh_set_error(PMH_ERR_SUP, "SVR dual operator: dense rows are swept by the caller's own kernel"); }
  ~SvrDualOp() override
  {
    if (w) pmh_free(ctx, w);
    if (part) pmh_free(ctx, part);
    if (spart) pmh_free(ctx, spart);
  }
};

// ---- samples in CSR --------------------------------------------------------------------------------------------------------------------------------------------
// s = p - q before pass 1; SUB: s_i = m_i ? p_i - q_i : 0, a selection
template <int SUB>
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_diff(int nl, const double *__restrict__ p, const double *__restrict__ q, double *__restrict__ s, const double *__restrict__ m)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < nl; i += (long long)gridDim.x * PMH_BLOCK) s[i] = (SUB && m[i] == 0.0) ? 0.0 : p[i] - q[i];
}
// the two halves after pass 2 from v_i = x_i . w + sigma S: out_p[i] = v_i + D_i p_i, out_q[i] = -v_i + D_i q_i (AUG as in svr_store_row)
// SUB: +0 in both halves of a held-out row, nothing of it read but m_i
template <int AUG, int SUB>
__global__ __launch_bounds__(PMH_BLOCK) void k_svr_halves(int nl, const double *__restrict__ v, svr_row_out o)
{
  for (long long i = (long long)blockIdx.x * PMH_BLOCK + threadIdx.x; i < nl; i += (long long)gridDim.x * PMH_BLOCK) {
    if (SUB && o.m[i] == 0.0) {
      o.op[i] = 0.0, o.oq[i] = 0.0;
      continue;
    }
    const double vi = v[i];
    if (AUG == 0) o.op[i] = vi, o.oq[i] = -vi;
    else {
      const double D = AUG == 2 ? o.diag[i] : o.shift;
      o.op[i] = vi + D * o.p[i], o.oq[i] = -vi + D * o.q[i];
    }
  }
}
// The classification operator of svm_csr.hip over X with all labels +1 does the two sweeps: applied to s = p - q it gives x_i . w + sigma S (its own rank-one
// term; its shift and diagonal stay off: D multiplies p_i and q_i, not s_i).  One column-ordered copy of X, the subset's arrangement of n-vector kernels
struct SvrCsrOp : SvrDualBase {
  pmh_op       inner = nullptr;
  SvmDualBase *in    = nullptr;
  double      *ones = nullptr, *s = nullptr, *v = nullptr; // [nl] each
  int diff(const double *u)
  {
    svm_const<2>(ym != nullptr, [&](auto S) { hipLaunchKernelGGL(k_svr_diff<decltype(S)::value>, dim3(pmh_vec_grid(nl)), dim3(PMH_BLOCK), 0, ctx->stream, nl, u, u + nl, s, (const double *)msk); });
    PMH_HIP(hipGetLastError());
    return PMH_SUCCESS;
  }
  // A subset: the inner operator takes the mask (its labels are all +1, so its masked labels are m: its pass 1 and its sigma term run over S; every stored
  // entry is still swept, and the one column-ordered copy stays), k_svr_halves writes the zeros of the held-out rows: n-vector work only
  int take_mask(const double *m_dev, long long ones, int first) override
  {
    PMH_CHK(pmh_op_svm_dual_set_subset(inner, m_dev));
    return SvrDualBase::take_mask(m_dev, ones, first);
  }
  int mult(const double *u, double *out) override
  {
    if (nl == 0 && pmh_comm_on(ctx)) return pmh_set_error(PMH_ERR_ARG, "%s", svr_empty_rank);
    if (nl == 0) return PMH_SUCCESS;
    PMH_CHK(diff(u));
    in->sigma    = sigma + sigma_fold;
    const int rc = in->mult(s, v);
    npass        = in->npass;
    PMH_CHK(rc);
    svr_row_out o{u, u + nl, diag, out, out + nl, 0.0, shift, msk};
    svm_const<3>(diag ? 2 : (shift != 0.0 ? 1 : 0), [&](auto A) {
      svm_const<2>(ym != nullptr, [&](auto S) { hipLaunchKernelGGL((k_svr_halves<decltype(A)::value, decltype(S)::value>), dim3(pmh_vec_grid(nl)), dim3(PMH_BLOCK), 0, ctx->stream, nl, (const double *)v, o); });
    });
    PMH_HIP(hipGetLastError());
    return PMH_SUCCESS;
  }
  int mult_epi(const double *, double *, const pmh_vec_epi &) override
  {
    if (nl <= 0 && pmh_comm_on(ctx)) return pmh_set_error(PMH_ERR_ARG, "%s", svr_empty_rank);
    return PMH_EPI_UNSUPPORTED;
  }
  int form_w(const double *u, const double **w_dev) override
  {
    if (nl > 0) PMH_CHK(diff(u));
    const int rc = in->form_w(s, w_dev);
    npass        = in->npass;
    return rc;
  }
  int row_dots(const double *w_dev, double *dots) override
  {
    const int rc = pmh_svm_csr_op_row_dots(in, w_dev, dots);
    npass        = in->npass;
    return rc;
  }
  ~SvrCsrOp() override
  {
    if (inner) pmh_op_destroy(inner);
    if (ones) pmh_free(ctx, ones);
    if (s) pmh_free(ctx, s);
    if (v) pmh_free(ctx, v);
  }
};

static int svr_base(pmh_op op, const char *who, SvrDualBase **o)
{
  *o = dynamic_cast<SvrDualBase *>(op);
  return *o ? PMH_SUCCESS : pmh_set_error(PMH_ERR_ARG, "%s: not an operator of pmh_op_create_svr_dual", who);
}
// (the rules and the messages are pmh_op_svm_dual_set_terms / _set_diag's: the one place that checks them)
extern "C" int pmh_op_svr_dual_set_terms(pmh_op op, double shift, double sigma)
{
  SvrDualBase *o;
  PMH_CHK(svr_base(op, "pmh_op_svr_dual_set_terms", &o));
  return pmh_op_svm_dual_set_terms(op, shift, sigma);
}
extern "C" int pmh_op_svr_dual_set_diag(pmh_op op, const double *diag_dev)
{
  SvrDualBase *o;
  PMH_CHK(svr_base(op, "pmh_op_svr_dual_set_diag", &o));
  return pmh_op_svm_dual_set_diag(op, diag_dev);
}
// (the mask's rules and messages are pmh_svm_check_mask's, shared with pmh_op_svm_dual_set_subset; a refused mask changes nothing)
extern "C" int pmh_op_svr_dual_set_subset(pmh_op op, const double *m_dev)
{
  SvrDualBase *o;
  PMH_CHK(svr_base(op, "pmh_op_svr_dual_set_subset", &o));
  long long ones  = 0;
  int       first = 0;
  if (m_dev) PMH_CHK(pmh_svm_check_mask(o->ctx, "pmh_op_svr_dual_set_subset", o->nl, m_dev, &ones, &first));
  return o->take_mask(m_dev, ones, first);
}
extern "C" int pmh_op_svr_dual_passes(pmh_op op, long long *passes)
{
  SvrDualBase *o;
  PMH_CHK(svr_base(op, "pmh_op_svr_dual_passes", &o));
  return pmh_op_svm_dual_passes(op, passes);
}

// X_dev: n_local x d doubles, or floats where f32; the limits and the refusal of svm_dual_create
static int svr_dual_create(pmh_ctx ctx, int n_local, int d, const void *X_dev, int f32, pmh_op *op)
{
  PMH_ARG(ctx && op && n_local >= 0 && d >= 1 && d <= 64 * SVM_KMAX && X_dev);
  if (n_local > (1 << 30)) return pmh_set_error(PMH_ERR_ARG, "pmh_op_create_svr_dual: %d samples, the operator's 2 n_local rows must stay below 2^31", n_local);
  SvrDualOp *o = new SvrDualOp();
  o->ctx = ctx, o->nl = n_local, o->n = 2 * n_local, o->d = d, o->X = X_dev, o->f32 = f32;
  long long nb = ((long long)n_local + 4 * 16 - 1) / (4 * 16); // >= 16 rows per wavefront
  o->nblocks   = (int)(nb < 1 ? 1 : (nb > PMH_MAX_VEC_BLOCKS ? PMH_MAX_VEC_BLOCKS : nb));
  int rc;
  if ((rc = o->init_labels()) || (rc = pmh_malloc(ctx, sizeof(double) * ((size_t)d + 1), (void **)&o->w)) || (rc = pmh_malloc(ctx, sizeof(double) * (size_t)o->nblocks * d, (void **)&o->part)) ||
      (rc = pmh_malloc(ctx, sizeof(double) * (size_t)o->nblocks, (void **)&o->spart))) {
    delete o;
    return rc;
  }
  *op = o;
  return PMH_SUCCESS;
}
extern "C" int pmh_op_create_svr_dual(pmh_ctx ctx, int n_local, int d, const double *X_dev, pmh_op *op) { return svr_dual_create(ctx, n_local, d, X_dev, 0, op); }
extern "C" int pmh_op_create_svr_dual_f32(pmh_ctx ctx, int n_local, int d, const float *X_dev, pmh_op *op) { return svr_dual_create(ctx, n_local, d, X_dev, 1, op); }

extern "C" int pmh_op_create_svr_dual_csr(pmh_ctx ctx, pmh_csr X, pmh_op *op)
{
  PMH_ARG(ctx && X && op && X->ctx == ctx);
  const int nl = X->nrows;
  if (nl > (1 << 30)) return pmh_set_error(PMH_ERR_ARG, "pmh_op_create_svr_dual_csr: %d samples, the operator's 2 n_local rows must stay below 2^31", nl);
  SvrCsrOp *o = new SvrCsrOp();
  o->ctx = ctx, o->nl = nl, o->n = 2 * nl, o->d = X->ncols;
  const size_t nb = sizeof(double) * (size_t)(nl ? nl : 1);
  int          rc;
  if ((rc = o->init_labels()) || (rc = pmh_malloc(ctx, nb, (void **)&o->ones)) || (rc = pmh_malloc(ctx, nb, (void **)&o->s)) || (rc = pmh_malloc(ctx, nb, (void **)&o->v)) ||
      (rc = pmh_vec_set(ctx, nl, o->ones, 1.0)) || (rc = pmh_op_create_svm_dual_csr(ctx, X, o->ones, &o->inner))) {
    delete o;
    return rc;
  }
  o->in = static_cast<SvmDualBase *>(o->inner);
  *op   = o;
  return PMH_SUCCESS;
}
