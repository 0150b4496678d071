// The dense-row SVM dual operator (svm.hip) as the penalised operator (qppf.hip) and the SVM front end (svm_train.hip) see it.
#pragma once
#include "pmh_internal.h"

#define SVM_KMAX 4 // d <= 64 * SVM_KMAX
// a launch that streams X once (counted: pmh_op_svm_dual_passes)
#define SVM_PASS(...)                 \
  do {                                \
    npass++;                          \
    hipLaunchKernelGGL(__VA_ARGS__);  \
  } while (0)

struct SvmDualOp : pmh_op_s {
  int           d;
  const double *X, *y;
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
  long long     npass = 0; // passes over X so far
  // augmented Hessian H + shift I + (sigma + sigma_fold) y y' (L2 loss: shift = 1/C; the one-row equality y'a = 0 penalised: sigma_fold = rho c^2 for the
  // row c y, set by the penalised operator around each of its products, see qppf.hip).  s = sum_i y_i v_i travels with the column sums: w[d] (and one entry per
  // workgroup beside part / part_next).  All three zero: the kernels of the plain operator (template argument AUG = 0), the bits of the plain operator.
  double        shift = 0.0, sigma = 0.0, sigma_fold = 0.0;
  double       *spart = nullptr, *spart_next = nullptr; // [nblocks] / [grid_epi] partial sums of s
  bool          aug() const { return shift != 0.0 || sigma != 0.0 || sigma_fold != 0.0; }
  // ||B u|| of the one-row equality riding on the next product (the penalised operator arms it): sum_i y_i u_i taken where the rows' y_i are in registers
  // anyway, finished by k_svm_aux_finish: Gu[0] = c sum, (c sum)^2 -> scalar slot.  One GPU only (the caller falls back to the projector's own dot otherwise)
  const double *aux_u = nullptr;
  double       *aux_Gu = nullptr, *aux_part = nullptr;
  double        aux_c = 0.0;
  int           aux_slot = -1, aux_done = 0;
  int           aux_finish(int nb);
  ~SvmDualOp() override
  {
    pmh_free(ctx, w);
    pmh_free(ctx, part);
    if (part_next) pmh_free(ctx, part_next), pmh_free(ctx, feas_part), pmh_free(ctx, d_afeas), pmh_free(ctx, x_spec), pmh_free(ctx, spart_next);
    if (spart) pmh_free(ctx, spart);
    if (aux_part) pmh_free(ctx, aux_part);
  }
};


// svm.hip, for the front end: w = X'(y o a) into the operator's own w (d doubles, device; all-reduced under a communicator) by the pass-1 kernels
int pmh_svm_op_form_w(SvmDualOp *o, const double *a, const double **w_dev);
// 1 (and c, with row = c y) if pf is a one-row projector whose row is a multiple of this operator's labels, entry by entry
int pmh_svm_op_row_is_labels(SvmDualOp *o, pmh_qppf pf, double *c);
