"""SVM front end (pmh_svm_*, csrc/svm_train.hip): train a linear SVM with L1 or L2 loss, with or without bias term, on the device; return the model; predict.

    L1: min 1/2 a'Ha - 1'a,          0 <= a <= C
    L2: min 1/2 a'(H + I/C)a - 1'a,  0 <= a
    bias: additionally y'a = 0 (SMALXE over a one-row projector; without bias MPGP alone)

H = diag(y) X X' diag(y).  Everything is computed by libpermonhip.so; there is no CPU fallback."""
import ctypes as ct

import numpy as np

from . import _lib
from ._lib import check
from .core import Vec


class SVM:
    def __init__(self, ctx, loss="L1", C=1.0, bias=True, options=""):
        """options: a PETSc-style option string for the solver (-qps_rtol 1e-6, -qps_mpgp_*, -qps_smalxe_*, -smalxe_qps_* ...) and -svm_loss_type / -svm_C /
        -svm_bias, which override the keyword arguments."""
        self.ctx, self.L = ctx, ctx.L
        o = _lib.SvmOpts()
        check(self.L.pmh_svm_default_opts(o))
        left = ct.create_string_buffer(4096)
        check(self.L.pmh_svm_set_from_options(("-svm_loss_type %s -svm_C %r -svm_bias %d %s" % (loss, float(C), int(bool(bias)), options)).encode(), o, left, len(left)))
        self.opts = o
        self.options_left = [k for k in left.value.decode().split() if k]
        self.h = None
        self._keep = None

    loss = property(lambda self: "L2" if self.opts.loss_type == 1 else "L1")
    C = property(lambda self: self.opts.C)
    bias = property(lambda self: bool(self.opts.bias))

    def _dev(self, a):
        return a if isinstance(a, Vec) else Vec.from_numpy(self.ctx, np.ascontiguousarray(a, dtype=np.float64).ravel())

    def create(self, X, y):
        """Set the training samples (X: (n, d) row-major, y: +-1) and build the solver without training."""
        self.destroy()
        X = np.ascontiguousarray(X, dtype=np.float64)
        self.n, self.d = X.shape
        Xd, yd = self._dev(X), self._dev(y)
        h = ct.c_void_p()
        try:
            check(self.L.pmh_svm_create(self.ctx.h, self.n, self.d, Xd.p, yd.p, self.opts, ct.byref(h)))
        except Exception:
            Xd.free(), yd.free()
            raise
        self.h, self._keep = h, (Xd, yd)
        return self

    def fit(self, X, y):
        self.create(X, y)
        check(self.L.pmh_svm_train(self.h))
        return self

    def _need(self):
        if self.h is None:
            raise RuntimeError("SVM: call fit first")

    @property
    def w(self):
        self._need()
        w = np.empty(self.d)
        check(self.L.pmh_svm_get_model(self.h, w.ctypes.data_as(ct.c_void_p), None))
        return w

    @property
    def b(self):
        self._need()
        b = ct.c_double()
        check(self.L.pmh_svm_get_model(self.h, None, ct.byref(b)))
        return b.value

    @property
    def alpha(self):
        self._need()
        v = Vec(self.ctx, self.n, zero=False)
        check(self.L.pmh_svm_get_dual(self.h, v.p))
        a = v.to_numpy()
        v.free()
        return a

    @property
    def stats(self):
        self._need()
        st = _lib.SvmStats()
        check(self.L.pmh_svm_get_stats(self.h, ct.byref(st)))
        return st

    def solver_handles(self):
        """(H, pf, mpgp, smalxe) as ctypes handles, borrowed (pmh_svm_get_solver); a solver not in use is None."""
        self._need()
        v = [ct.c_void_p() for _ in range(4)]
        check(self.L.pmh_svm_get_solver(self.h, *[ct.byref(x) for x in v]))
        return tuple(x if x.value else None for x in v)

    def _predict(self, X, want_scores, want_labels):
        self._need()
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError("SVM: X must be (n, %d)" % self.d)
        n = X.shape[0]
        Xd = self._dev(X)
        s = Vec(self.ctx, n, zero=False) if want_scores else None
        l = Vec(self.ctx, n, zero=False) if want_labels else None
        check(self.L.pmh_svm_predict(self.h, n, Xd.p, s.p if s else None, l.p if l else None))
        out = (s.to_numpy() if s else None, l.to_numpy() if l else None)
        for v in (Xd, s, l):
            if v is not None:
                v.free()
        return out

    def decision_function(self, X):
        return self._predict(X, True, False)[0]

    def predict(self, X):
        return self._predict(X, False, True)[1]

    def test(self, X, y):
        """Confusion counts of the predicted labels against y: dict(TP, FP, TN, FN, accuracy)."""
        self._need()
        X = np.ascontiguousarray(X, dtype=np.float64)
        n = X.shape[0]
        Xd, yd = self._dev(X), self._dev(y)
        cnt = (ct.c_longlong * 4)()
        check(self.L.pmh_svm_test(self.h, n, Xd.p, yd.p, cnt))
        Xd.free(), yd.free()
        tp, fp, tn, fn = (int(c) for c in cnt)
        return dict(TP=tp, FP=fp, TN=tn, FN=fn, accuracy=(tp + tn) / n if n else float("nan"))

    def destroy(self):
        if self.h is not None:
            self.L.pmh_svm_destroy(self.h)
            self.h = None
            for v in self._keep or ():
                v.free()
            self._keep = None
