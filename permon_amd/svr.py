"""SVR front end (pmh_svr_*, csrc/svr_train.hip): linear epsilon-insensitive support vector regression, trained and scored on the device.

    L1: primal 1/2 |w|^2 + sum C_i max(0, |x_i . w + b - t_i| - eps)
    L2: primal 1/2 |w|^2 + 1/2 sum C_i max(0, |x_i . w + b - t_i| - eps)^2,      C_i = C sample_weight_i
    dual in u = [p; q]: min 1/2 u'H^u - c^'u, H^ = [Q + D, -Q; -Q, Q + D] (MatCreateSVRDual), c^ = [t - eps; -t - eps], 0 <= u (L1: <= C_i)
    bias: additionally sum (p_i - q_i) = 0 (SMALXE over a one-row projector; without bias MPGP alone)

Model: w = X'(p - q), f(x) = x . w + b.  X is an (n, d) ndarray (d <= 256), a DeviceSamples (dense rows already on the device: RFFMap.transform) or a
scipy.sparse matrix of any width, kept ONCE on the device; predict and test also take a MappedSamples (RFFMap.lazy: the features are never stored).  Everything is
computed by libpermonhip.so; there is no CPU fallback.  set_subset trains on a part of the handle's samples with X staying where it is, predict_own / test_own
score the handle's own rows without an upload, and permon_amd.svm.cross_validate loops the three over k folds.  Not here: warm starts, a grid search (SVM has
them)."""
import ctypes as ct

import numpy as np

from . import _lib
from ._lib import check
from .core import Vec, sample_dtype_of
from .mat import is_sparse
from .svm import _Samples, _SVMHandle, _vecs


class SVR(_SVMHandle):
    """The handle, its keep-alive buffers and how a call is made on samples of either kind are _SVMHandle's; the options are pmh_svr_opts."""

    _who, _pre = "SVR", "pmh_svr_"

    def __init__(self, ctx, loss="L1", C=1.0, epsilon=0.1, bias=True, options="", sample_dtype=None):
        """options: a PETSc-style option string for the solver (-qps_rtol 1e-6, -qps_mpgp_*, -qps_smalxe_*, -smalxe_qps_* ...) and -svr_loss_type / -svr_C /
        -svr_epsilon / -svr_bias, which override the keyword arguments.  sample_dtype: as in SVM (numpy.float32 keeps dense samples in float32 on the device)."""
        self.ctx, self.L = ctx, ctx.L
        self.sample_dtype = sample_dtype_of(sample_dtype, False, "SVR")
        o = _lib.SvrOpts()
        check(self.L.pmh_svr_default_opts(o))
        if loss not in ("L1", "L2"):
            raise ValueError("SVR: loss must be \"L1\" or \"L2\"")
        o.loss_type, o.C, o.epsilon, o.bias = int(loss == "L2"), float(C), float(epsilon), int(bool(bias))  # (checked by pmh_svr_create)
        left = ct.create_string_buffer(4096)
        check(self.L.pmh_svr_set_from_options(options.encode(), o, left, len(left)))
        self.opts = o
        self.options_left = [k for k in left.value.decode().split() if k]
        self.h = None
        self._keep = None

    epsilon = property(lambda self: self.opts.epsilon)

    def create(self, X, t, sample_weight=None):
        """Set the training samples (X: (n, d) row-major ndarray or scipy.sparse matrix; t: n finite targets) and build the solver without training.  The handle
        borrows both for its lifetime.  sample_weight: n positive numbers that scale the samples' penalties (None: all 1)."""
        sample_dtype_of(self.sample_dtype, is_sparse(X), "SVR")  # (float32 with sparse samples is refused)
        self.destroy()
        if np.ndim(X) != 2:
            raise ValueError("SVR: X must be (n, d)")
        tn = np.ascontiguousarray(t, dtype=np.float64).ravel()
        if tn.size != np.shape(X)[0]:
            raise ValueError("SVR: t must have %d entries" % np.shape(X)[0])
        self._create_handle(X, tn)
        if sample_weight is not None:
            self.set_penalties(sample_weight=sample_weight)
        return self

    def set_penalties(self, C=None, sample_weight=None):
        """C_i = C sample_weight_i on the created handle (pmh_svr_set_penalties; None: the handle's C, all 1); the handle is untrained afterwards."""
        self._need()
        with self._lent(sample_weight) as wd:
            if wd is not None and wd.n != self.n:
                raise ValueError("SVR: sample_weight must have %d entries" % self.n)
            check(self.L.pmh_svr_set_penalties(self.h, float(self.C if C is None else C), wd.p if wd is not None else None))
        return self

    def set_epsilon(self, epsilon):
        """A new epsilon on the created handle (pmh_svr_set_epsilon): the right-hand side alone changes; the handle is untrained afterwards."""
        self._need()
        check(self.L.pmh_svr_set_epsilon(self.h, float(epsilon)))
        self.opts.epsilon = float(epsilon)
        return self

    def set_subset(self, mask):
        """Train on the samples where mask is true, X staying on the device (pmh_svr_set_subset): n booleans or 0 / 1 numbers; None: all samples again.  The
        handle is untrained afterwards; set_epsilon and set_penalties keep the subset.  After train() alpha is 0 on the held-out samples in both halves and the
        model is that of a fit on (X[mask], t[mask]); predict_own / test_own score the held-out samples without an upload."""
        self._need()
        if mask is None:
            check(self.L.pmh_svr_set_subset(self.h, None))
            return self
        m = np.asarray(mask)
        if m.dtype != np.bool_ and not (np.issubdtype(m.dtype, np.integer) or np.issubdtype(m.dtype, np.floating)):
            raise ValueError("SVR: the mask must hold booleans or 0 / 1 numbers, not %s" % m.dtype)
        m = np.ascontiguousarray(m, dtype=np.float64).ravel()
        if m.size != self.n:
            raise ValueError("SVR: the mask must have %d entries" % self.n)
        with self._lent(m) as md:
            check(self.L.pmh_svr_set_subset(self.h, md.p))
        return self

    @property
    def subset(self):
        """The training mask as n booleans (pmh_svr_get_subset), or None where all samples train."""
        self._need()
        with _vecs(self.ctx, self.n) as (v,):
            check(self.L.pmh_svr_get_subset(self.h, v.p, None))
            m = v.to_numpy() != 0.0
        return None if m.all() else m

    @property
    def n_subset(self):
        """The samples the problem is posed over (pmh_svr_get_subset): the subset's, or all."""
        self._need()
        k = ct.c_longlong()
        check(self.L.pmh_svr_get_subset(self.h, None, ct.byref(k)))
        return int(k.value)

    def train(self):
        """Train from u = 0 (pmh_svr_train)."""
        self._need()
        check(self.L.pmh_svr_train(self.h))
        return self

    def fit(self, X, t, sample_weight=None):
        return self.create(X, t, sample_weight).train()

    @property
    def w(self):
        self._need()
        w = np.empty(self.d)
        check(self.L.pmh_svr_get_model(self.h, w.ctypes.data_as(ct.c_void_p), None))
        return w

    @property
    def b(self):
        self._need()
        b = ct.c_double()
        check(self.L.pmh_svr_get_model(self.h, None, ct.byref(b)))
        return b.value

    @property
    def alpha(self):
        """(2 n,): the dual [p; q] (pmh_svr_get_dual)."""
        self._need()
        with _vecs(self.ctx, 2 * self.n) as (v,):
            check(self.L.pmh_svr_get_dual(self.h, v.p))
            return v.to_numpy()

    @property
    def beta(self):
        """(n,): p - q, the coefficients of w = X'beta."""
        u = self.alpha
        return u[:self.n] - u[self.n:]

    @property
    def stats(self):
        self._need()
        st = _lib.SvrStats()
        check(self.L.pmh_svr_get_stats(self.h, ct.byref(st)))
        return st

    def solver_handles(self):
        """(H, pf, mpgp, smalxe) as ctypes handles, borrowed (pmh_svr_get_solver); a solver not in use is None."""
        self._need()
        v = [ct.c_void_p() for _ in range(4)]
        check(self.L.pmh_svr_get_solver(self.h, *[ct.byref(x) for x in v]))
        return tuple(x if x.value else None for x in v)

    def _test_samples(self, X):
        """X for a scoring call: refused before any upload unless it is (n, d)."""
        self._need()
        S = _Samples(self.ctx, X, dtype=self.sample_dtype)
        if S.X.ndim != 2 or S.X.shape[1] != self.d:
            raise ValueError("SVR: X must be (n, %d)" % self.d)
        return S

    def predict(self, X):
        """(n,): f(x_i) = x_i . w + b in one pass over X (pmh_svr_predict)."""
        S = self._test_samples(X)
        with S as (n, xa), _vecs(self.ctx, n) as (f,):
            check(self._entry("predict", S)(self.h, *xa, f.p))
            return f.to_numpy()

    def test(self, X, t):
        """Scores X and reduces the residuals r = f(x) - t in the same pass (pmh_svr_test): dict(mse, mae, r2, max_abs, n_in_tube, n) and the sums they come
        from (sum_r, sum_r2, sum_abs_r, sum_t, sum_t2)."""
        S = self._test_samples(X)
        tn = np.ascontiguousarray(t, dtype=np.float64).ravel()
        if tn.size != S.X.shape[0]:
            raise ValueError("SVR: t must have %d entries" % S.X.shape[0])
        m = _lib.SvrMetrics()
        with S as (n, xa):
            td = Vec.from_numpy(self.ctx, tn)
            try:
                check(self._entry("test", S)(self.h, *xa, td.p, ct.byref(m)))
            finally:
                td.free()
        return {k: getattr(m, k) for k, _ in _lib.SvrMetrics._fields_}

    def predict_own(self):
        """(n,): f(x_i) of the samples the handle was created on, held-out ones included, without an upload (pmh_svr_predict_own): bit for bit predict(X)."""
        self._need()
        with _vecs(self.ctx, self.n) as (f,):
            check(self.L.pmh_svr_predict_own(self.h, f.p))
            return f.to_numpy()

    OWN = {"held_out": 0, "subset": 1, "all": 2}  # PMH_SVM_OWN_*

    def test_own(self, which="held_out"):
        """The metrics of the handle's own samples against its targets over the held-out samples, the subset or all of them (pmh_svr_test_own), nothing
        uploaded: the dict test returns; n is the number of selected samples."""
        self._need()
        if which not in self.OWN:
            raise ValueError("SVR: which must be one of %s" % ", ".join(sorted(self.OWN)))
        m = _lib.SvrMetrics()
        check(self.L.pmh_svr_test_own(self.h, self.OWN[which], ct.byref(m)))
        return {k: getattr(m, k) for k, _ in _lib.SvrMetrics._fields_}
