// The regression dual operators (svr.hip) as the SVR front end (svr_train.hip) sees them.
#pragma once
#include "svm_internal.h"

// H^ = [Q + D, -Q; -Q, Q + D] on u = [p; q]: the classification dual on the doubled samples (SvmDualBase::doubled).  n = 2 nl; y = yy, the labels [+1; -1];
// shift / sigma / sigma_fold / diag as in SvmDualBase, diag being nl doubles used for both halves; form_w(u) gives w = X'(p - q)
// A sample subset (pmh_op_svr_dual_set_subset, a mask m of nl entries): H^_S = M^ H^ M^ + sigma e^ e^', M^ = diag([m; m]), e^ = [m; -m].  The masked labels of the
// doubled problem are ym = [m; -m] (2 nl doubles, +0 on a held-out sample in both halves: what pmh_svm_op_row_is_labels compares the equality's row with), and
// their first half IS the mask: msk points at ym, the kernels read ym[i], i < nl, as m_i.  n_sub: the samples of this rank in S, sub_first: the first of them
struct SvrDualBase : SvmDualBase {
  int     nl = 0;       // samples of this rank
  double *yy = nullptr; // [2 nl]
  bool    doubled() const override { return true; }
  int     set_labels(const double *) override { return pmh_set_error(PMH_ERR_SUP, "pmh_op_svm_dual_set_labels: the regression operator (pmh_op_create_svr_dual) has no labels to set"); }
  // CSR samples: dots[i] = x_i . w by the row sweep with the operator's tables, counted as a pass; dense rows: the front end sweeps X itself
  virtual int row_dots(const double *w_dev, double *dots) = 0;
  int         init_labels(); // yy = [+1; -1], y = yy
  // the checked mask m_dev (nullptr: all samples) becomes the operator's: ym = [m; -m], msk = ym.  CSR: the inner classification operator takes it first
  virtual int take_mask(const double *m_dev, long long ones, int first);
  // H^ 1 = D 1: all ones is an eigenvector of the SMALLEST eigenvalues (0 for L1, 1 / C for L2), and a power method started there stays there.  The largest
  // belong to vectors [v; -v]: the start is [1; 0], which has a component along them.  Under a subset it stays [1; 0]: the operator masks its operand, so the
  // first product sees [m; 0], which has a component along the top eigenvectors [v; -v] of H^_S (v supported on S)
  int         maxeig_start(double *v) override;
  ~SvrDualBase() override
  {
    if (yy) pmh_free(ctx, yy);
    if (ym) pmh_free(ctx, ym);
    msk = ym = nullptr; // (msk is ym: the base frees neither)
  }
};
