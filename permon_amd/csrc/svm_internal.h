// The SVM dual operators (svm.hip: dense rows; svm_csr.hip: CSR) as the penalised operator (qppf.hip) and the SVM front end (svm_train.hip) see them.
#pragma once
#include <type_traits>

#include "pmh_internal.h"

#define SVM_KMAX 4 // d <= 64 * SVM_KMAX
// grid of the row sweeps over n samples (svm_rows.h): 64 rows per workgroup, capped
#define SVM_NB(n) ((int)((((long long)(n) + 63) / 64) < 1 ? 1 : ((((long long)(n) + 63) / 64) > PMH_MAX_VEC_BLOCKS ? PMH_MAX_VEC_BLOCKS : (((long long)(n) + 63) / 64))))
// a launch that streams X once (counted: pmh_op_svm_dual_passes); a kernel given as a template-id with a comma goes in parentheses
#define SVM_PASS(...)                 \
  do {                                \
    npass++;                          \
    hipLaunchKernelGGL(__VA_ARGS__);  \
  } while (0)

// What the penalised operator (qppf.hip) and the front end (svm_train.hip) need of an SVM dual operator, whichever way it holds the samples: dense rows
// (SvmDualOp, svm.hip) or CSR (SvmCsrOp, svm_csr.hip)
struct SvmDualBase : pmh_op_s {
  int           d = 0;
  const double *y = nullptr;
  long long     npass = 0; // passes over X so far
  // augmented Hessian H + shift I + (sigma + sigma_fold) y y' (L2 loss: shift = 1/C; the one-row equality y'a = 0 penalised: sigma_fold = rho c^2 for the
  // row c y, set by the penalised operator around each of its products, see qppf.hip).  s = sum_i y_i v_i travels with the column sums: w[d].  All three zero:
  // the kernels of the plain operator, the bits of the plain operator.
  double        shift = 0.0, sigma = 0.0, sigma_fold = 0.0;
  // H + diag(diag) + (sigma + sigma_fold) y y' (pmh_op_svm_dual_set_diag: per-sample penalties of the L2 loss, diag_i = 1 / C_i): n doubles, borrowed, read by
  // pass 2 where it reads a_i and y_i; excludes a non-zero shift.  The kernels' AUG template argument is aug_form(): 0 plain, 1 shift, 2 diag
  const double *diag = nullptr;
  // A sample subset S (pmh_op_svm_dual_set_subset): H_S = M (H + D) M, M = diag(m), m_i in {0, 1}.  The operator keeps the mask (msk) and the masked labels
  // ym = m o y (n doubles each, its own memory; both nullptr: all samples) and hands ym to its kernels where they read y: a held-out row is ym_i == 0 at no
  // extra traffic.  y stays the caller's labels; set_labels rebuilds ym from msk
  double       *msk = nullptr, *ym = nullptr;
  long long     n_sub = 0;    // samples of this rank in S
  int           sub_first = 0; // the first of them (the entry pmh_svm_op_row_is_labels takes the row's scale from)
  const double *yk() const { return ym ? ym : y; }
  int           refresh_ym(); // ym = m o y (after new labels)
  ~SvmDualBase() override
  {
    if (msk) pmh_free(ctx, msk), pmh_free(ctx, ym);
  }
  bool          aug() const { return shift != 0.0 || sigma != 0.0 || sigma_fold != 0.0 || diag != nullptr; }
  int           aug_form() const { return !aug() ? 0 : (diag ? 2 : 1); }
  // ||B u|| of the one-row equality riding on the next product (the penalised operator arms it); an operator that does not serve it leaves aux_done 0 and the
  // caller's own dot product runs
  const double *aux_u = nullptr;
  double       *aux_Gu = nullptr;
  double        aux_c = 0.0;
  int           aux_slot = -1, aux_done = 0;
  // w = X'(y o a) into the operator's own w (d doubles, device; all-reduced under a communicator) by the pass-1 kernels (the model of a trained SVM)
  virtual int   form_w(const double *a, const double **w_dev) = 0;
  virtual void  terms_changed() {} // pmh_op_svm_dual_set_terms / pmh_op_svm_dual_set_diag was called
  // The regression operator (svr.hip) is this dual on the doubled samples [X; X] with labels [+1; -1], X held once: n = 2 n_local, y its own 2 n_local labels
  // (what pmh_svm_op_row_is_labels compares the equality's row with, so that the penalised operator folds rho G'G into sigma_fold as it does here), diag
  // n_local doubles used for both halves.  It takes no new labels, and a subset through its own entry (pmh_op_svr_dual_set_subset: a mask of n_local entries)
  virtual bool  doubled() const { return false; }
  // pmh_op_svm_dual_set_labels: new labels (n doubles of +-1, borrowed; may be the buffer borrowed so far with new contents).  Whatever the operator derived
  // from the old labels it redoes from state of its own, never from the caller's memory
  virtual int   set_labels(const double *y_dev)
  {
    y = y_dev;
    terms_changed();
    return refresh_ym();
  }
};

// Picking a kernel instance: f(std::integral_constant<int, v>()) for the run-time v in [0, N), so that the launch site names its kernel once, with
// decltype(V)::value as template arguments, and exactly the instances that can be picked are compiled
template <int N, class F>
static void svm_const(int v, F f)
{
  if constexpr (N > 1) {
    if (v == N - 1) return f(std::integral_constant<int, N - 1>());
    return svm_const<N - 1>(v, f);
  } else f(std::integral_constant<int, 0>());
}
// the type dense samples are stored in, as a picked constant: 0 double, 1 float (pmh_op_create_svm_dual_f32, pmh_svm_*_f32)
template <class V> using svm_sample_t = std::conditional_t<V::value != 0, float, double>;
// f(A, S, T): A::value the operator's form out of NAUG (SvmDualBase::aug_form(): 0 plain, 1 scalar shift, 2 diagonal; pass 1 knows 0 and 1 only), S::value 1 under
// a subset (the SUB = 1 instances, which read the masked labels), svm_sample_t<T> the samples' type
template <int NAUG, class F>
static void svm_pick(int form, bool sub, bool f32, F f)
{
  svm_const<NAUG>(form, [&](auto A) { svm_const<2>(sub, [&](auto S) { svm_const<2>(f32, [&](auto T) { f(A, S, T); }); }); });
}

struct SvmDualOp : SvmDualBase {
  const void   *X;       // n x d row-major, borrowed: doubles, or floats where f32
  int           f32 = 0; // the samples are stored in float32 (widened on arrival in the kernels; everything else stays fp64)
  double       *w, *part; // w: d; part: [nblocks][d]
  int           nblocks;
  int           mult(const double *a, double *Ha) override;
  // paired passes (d == 64, one GPU): see the block before k_svm_x64_grad
  int           mult_epi(const double *in, double *out, const pmh_vec_epi &e) override;
  int           spec_expansion_ready() override { return next_is == NEXT_XSPEC; }
  enum { NEXT_NONE = 0, NEXT_P, NEXT_XSPEC };
  // what part_next holds the partial sums of X'(y o v) for: the p of the last gradient split / the prepared expansion iterate
  int           next_is = NEXT_NONE;
  bool          next_aug = false; // the prepared sums carry the 65th column
  const double *next_p = nullptr;
  double       *part_next = nullptr, *feas_part = nullptr, *d_afeas = nullptr, *x_spec = nullptr;
  int           grid_epi = 0;
  // the augmented forms (SvmDualBase): s = sum_i y_i v_i is w[d] and one entry per workgroup beside part / part_next; template argument AUG = 0: the plain kernels
  double       *spart = nullptr, *spart_next = nullptr; // [nblocks] / [grid_epi] partial sums of s
  // the ||B u|| rider: sum_i y_i u_i taken where the rows' y_i are in registers anyway, finished by k_svm_aux_finish: Gu[0] = c sum, (c sum)^2 -> scalar slot.
  // One GPU only (the caller falls back to the projector's own dot otherwise)
  double       *aux_part = nullptr;
  int           aux_finish(int nb);
  // the two passes over X of one product, each with its launch counted and checked; aug: the AUG = 1 kernels (pass 1: + the 65th column sum and, where u is
  // given, sum_i y_i u_i -> upart)
  int           pass1(const double *v, bool aug, const double *u, double *upart);
  int           pass2(const double *a, double *out, bool aug);
  int           form_w(const double *a, const double **w_dev) override;
  void          terms_changed() override { next_is = NEXT_NONE; }
  ~SvmDualOp() override
  {
    pmh_free(ctx, w);
    pmh_free(ctx, part);
    if (part_next) pmh_free(ctx, part_next), pmh_free(ctx, feas_part), pmh_free(ctx, d_afeas), pmh_free(ctx, x_spec), pmh_free(ctx, spart_next);
    if (spart) pmh_free(ctx, spart);
    if (aux_part) pmh_free(ctx, aux_part);
  }
};


// the augmented row result: (y_i (x_i . w) + (sigma s) y_i) + shift a_i, in this order (s = w[d]); the diagonal form hands diag_i over as shift
static __device__ __forceinline__ double svm_aug_row(double yi, double dot, double sS, double shift, double ai) { return (yi * dot + sS * yi) + shift * ai; }

// w[c] = sum over the nblocks workgroups of part[b][c], c < d; spart != nullptr: w[d] = sum_b spart[b] too (k_svm_colsum: one wavefront per column, fixed order)
int pmh_svm_colsum(pmh_ctx ctx, int nblocks, int d, const double *part, double *w, const double *spart);

// The rules of a subset mask, checked in one place for pmh_op_svm_dual_set_subset and pmh_op_svr_dual_set_subset (who: the entry, for the messages): m_dev, n
// doubles on the device, must hold 0 / 1 only (else PMH_ERR_ARG with the count; a NaN is one) and at least one 1; both counts are summed over the communicator
// first, so every rank decides alike.  Nothing of the caller's is changed.  *ones: the ones of this rank, *first: the index of the first of them (0: none)
int pmh_svm_check_mask(pmh_ctx ctx, const char *who, int n, const double *m_dev, long long *ones, int *first);

// 1 (and c, with row = c y) if pf is a one-row projector whose row is a multiple of this operator's labels, entry by entry
int pmh_svm_op_row_is_labels(SvmDualBase *o, pmh_qppf pf, double *c);

// ---- svm_train.hip / svm_proba.hip: what the probability model shares across translation units (the sums and their finishing kernel: svm_front.h) ---------------------------------------------------------
// The Platt fit on scores[i * stride], i < n (column k of an n x K score matrix in place: scores + k, stride K).  The target of sample i is the positive one
// where y[i] == pos.  binary: every label must be +-1 (else PMH_ERR_ARG with the count); otherwise every label that is not pos is "the rest"
int pmh_svm_platt_fit_strided(pmh_ctx ctx, int n, const double *scores, int stride, const double *y, double pos, int binary, double *A, double *B, pmh_svm_platt_stats *st);

// the samples a binary handle was created on, as it borrows them, and its subset mask (svm_multi.hip scores its own rows over them): dense rows (*X, doubles
// unless *f32) or CSR (*Xcsr, then *X == nullptr); *msk: n doubles of 0 / 1 on the device, the operator's, valid until the next pmh_svm_set_subset; nullptr
// without a subset.  Any pointer may be NULL
void pmh_svm_own_samples(pmh_svm s, const void **X, int *f32, pmh_csr *Xcsr, const double **msk);

// ---- svm_csr.hip: samples in CSR --------------------------------------------------------------------------------------------------------------------
// dots[i] = x_i . w for the rows of X (one sweep over its stored entries, work divided by entries; w: X->ncols doubles, dots: X->nrows doubles, device)
int pmh_svm_csr_row_dots(pmh_csr X, const double *w, double *dots);
// the same for the operator's own samples, with the tables it already holds; counted as a pass
int pmh_svm_csr_op_row_dots(SvmDualBase *op, const double *w, double *dots);
// the test samples of the entry `who` (Xt, or dense rows: Xt == nullptr) against a model of d features: CSR of exactly d columns and fewer than 2^31 stored
// entries, dense only up to the sweeps' limit; else PMH_ERR_ARG in the name of who / who_csr
int pmh_svm_check_test_samples(const char *who, int d, pmh_csr Xt);
// Mapped samples (the *_rff entries): the features map(X) of n x map.d rows X of x_type (PMH_F64 / PMH_F32), which exist nowhere; their dot products with a
// model come from pmh_rffdots (rff_score.hip)
struct sv_mapped {
  pmh_rff     map;
  const void *X;
  int         x_type;
};
// the map's D must be the model's d (PMH_ERR_ARG naming both, in the name of who); n and X as the dense entries check them
int sv_check_mapped(const char *who, const sv_mapped &mp, int n, int d);
