"""SVM front end (pmh_svm_*, csrc/svm_train.hip): train a linear SVM with L1 or L2 loss, with or without bias term, on the device; return the model; predict.

    L1: min 1/2 a'Ha - 1'a,          0 <= a <= C
    L2: min 1/2 a'(H + I/C)a - 1'a,  0 <= a
    penalties: C_i = (y_i > 0 ? C_pos : C_neg) sample_weight_i in place of C (L1: the bound of a_i; L2: the diagonal entry 1 / C_i)
    bias: additionally y'a = 0 (SMALXE over a one-row projector; without bias MPGP alone)

H = diag(y) X X' diag(y).  X is an (n, d) ndarray (d <= 256) or a scipy.sparse matrix of any width (kept in CSR on the device: 24 bytes per stored entry for
the two orderings the operator sweeps), or a DeviceSamples (core.py: dense rows already on the device, such as RFFMap.transform returns -- read where they are, in
the handle's sample_dtype).  Test samples may also be a MappedSamples (RFFMap.lazy: scored from the feature map's registers, the features never stored, through the
_rff entries; training refuses it).  Everything is computed by libpermonhip.so; there is no CPU fallback.

Probabilities: P(y = +1 | x) = 1 / (1 + exp(A s(x) + B)) by Platt scaling (csrc/svm_proba.hip: the Newton iteration of Lin, Lin and Weng, 2007).  calibrate(X, y)
fits A, B on the scores of samples the caller supplies -- held-out ones, or the training set with the bias that brings -- and predict_proba applies them in
the one pass over X that scoring takes."""
import contextlib
import ctypes as ct
import math

import numpy as np

from . import _lib
from ._lib import check
from .core import DeviceSamples, MappedSamples, Vec, VecF32, refuse_mapped, sample_array, sample_dtype_of
from .mat import csr_from_scipy, is_sparse


PLATT_REASONS = {0: "set", 1: "converged", 2: "max_it", 3: "line_search"}  # pmh_svm_platt_stats.reason (PMH_PLATT_*); 0: the pair was set, not fitted


def platt_fit(ctx, scores, y):
    """Fit P(y = +1 | s) = 1 / (1 + exp(A s + B)) to scores and labels +-1 on the device (pmh_svm_platt_fit) -> (A, B, stats); stats.reason indexes
    PLATT_REASONS.  scores, y: arrays or Vecs of one length."""
    sd = scores if isinstance(scores, Vec) else Vec.from_numpy(ctx, np.ascontiguousarray(scores, dtype=np.float64).ravel())
    yd = y if isinstance(y, Vec) else Vec.from_numpy(ctx, np.ascontiguousarray(y, dtype=np.float64).ravel())
    try:
        if sd.n != yd.n:
            raise ValueError("platt_fit: %d scores and %d labels" % (sd.n, yd.n))
        A, B, st = ct.c_double(), ct.c_double(), _lib.SvmPlattStats()
        check(ctx.L.pmh_svm_platt_fit(ctx.h, sd.n, sd.p, yd.p, ct.byref(A), ct.byref(B), ct.byref(st)))
        return A.value, B.value, st
    finally:
        if sd is not scores:
            sd.free()
        if yd is not y:
            yd.free()


class _Borrowed:
    """What a handle keeps of a DeviceSamples it was created on: a reference, so that the buffer outlives the handle's use of it; freeing it is the caller's."""

    def __init__(self, samples):
        self.samples = samples

    def free(self):
        self.samples = None


class _Samples:
    """Samples for one library call: X, a scipy.sparse matrix (csr_from_scipy) or anything else (a contiguous array of dtype: float64, or float32 for the
    _f32 entries), is put on the device on entry and taken off again on exit, whatever happened in between.  A DeviceSamples is on the device already:
    entering uploads nothing, leaving frees nothing, and its dtype must be `dtype` -- nothing is converted.  Entering gives n and the samples' arguments of
    the entry: (handle,) for CSR, (n, pointer) for dense rows -- with_d: (n, d, pointer), as the create entries take them.  X is the converted array (the
    DeviceSamples itself, which has shape and ndim): the shape checks are the caller's.  A MappedSamples (test samples only: with_d is a TypeError) is on the
    device as well, whatever its source's dtype: entering gives (map, n, pointer, type) for the _rff entries; its shape is (n, D).  suffix: the entries'."""

    def __init__(self, ctx, X, with_d=False, dtype=np.float64):
        self.ctx, self.sparse, self.with_d, self.dev = ctx, is_sparse(X), with_d, None
        self.mapped = isinstance(X, MappedSamples)
        if self.mapped and with_d:
            refuse_mapped(X, "SVM")
        self.device = isinstance(X, DeviceSamples)
        self.f32 = not self.sparse and not self.mapped and dtype is np.float32
        self.suffix = "_rff" if self.mapped else "_csr" if self.sparse else "_f32" if self.f32 else ""
        if self.device and X.dtype != np.dtype(dtype):
            raise ValueError("SVM: the DeviceSamples hold %s and the handle's sample_dtype is %s: nothing is converted on the device (transform with out_dtype = "
                             "the handle's sample_dtype)" % (X.dtype, np.dtype(dtype)))
        self.X = X if self.sparse or self.device or self.mapped else sample_array(X, dtype, "SVM")

    def __enter__(self):
        n = self.X.shape[0]
        if self.mapped:
            return n, self.X.entry_args()
        if self.device:
            return n, ((n, self.X.shape[1], self.X.p) if self.with_d else (n, self.X.p))
        if self.sparse:
            self.dev = csr_from_scipy(self.ctx, self.X)
            return n, (self.dev.h,)
        self.dev = (VecF32 if self.f32 else Vec).from_numpy(self.ctx, self.X.ravel())
        return n, ((n, self.X.shape[1], self.dev.p) if self.with_d else (n, self.dev.p))

    def keep(self):
        """The device copy, the caller's from now on (a DeviceSamples: a reference to it that frees nothing)."""
        if self.device:
            return _Borrowed(self.X)
        d, self.dev = self.dev, None
        return d

    def __exit__(self, *exc):
        if self.dev is not None:
            self.dev.destroy() if self.sparse else self.dev.free()


@contextlib.contextmanager
def _vecs(ctx, *sizes):
    """Uninitialised device vectors of the given lengths for the length of a call (None: no vector, None in its place)."""
    vs = []
    try:
        for m in sizes:
            vs.append(None if m is None else Vec(ctx, m, zero=False))
        yield vs
    finally:
        for v in vs:
            if v is not None:
                v.free()


class _SVMHandle:
    """What SVM and SVMMulticlass share: the options, the handle with the buffers it borrows, and how a call is made on samples of either kind."""

    _who, _pre = "SVM", "pmh_svm_"  # the class in messages, the prefix of its entries

    def __init__(self, ctx, loss, C, bias, options):
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

    @contextlib.contextmanager
    def _lent(self, a):
        """a (an array, a Vec or None) as a Vec for the length of a call; a Vec made here is freed afterwards, the caller's is not."""
        v = None if a is None else self._dev(a)
        try:
            yield v
        finally:
            if v is not None and v is not a:
                v.free()

    def _need(self):
        if self.h is None:
            raise RuntimeError("%s: call fit first" % self._who)

    sample_dtype = np.float64  # the type dense samples are stored in on the device (SVM: the sample_dtype argument)

    def _entry(self, name, S=None):
        """The entry `name` of the handle for the samples S (a _Samples: its suffix _csr, _f32, _rff or none)."""
        return getattr(self.L, self._pre + name + (S.suffix if S is not None else ""))

    def _create_handle(self, X, y, *more):
        """The handle on (X, y), which it borrows for its lifetime: both stay on the device in _keep."""
        self.destroy()
        S = _Samples(self.ctx, X, with_d=True, dtype=self.sample_dtype)
        self.n, self.d = S.X.shape
        h = ct.c_void_p()
        with S as (n, xa):
            yd = self._dev(y)
            try:
                check(self._entry("create", S)(self.ctx.h, *xa, yd.p, self.opts, *more, ct.byref(h)))
            except Exception:
                yd.free()
                raise
            self.h, self._keep = h, (S.keep(), yd)
        return self

    def destroy(self):
        if self.h is not None:
            self._entry("destroy")(self.h)
            self.h = None
            for v in self._keep or ():
                v.destroy() if hasattr(v, "destroy") else v.free()
            self._keep = None


class SVM(_SVMHandle):
    def __init__(self, ctx, loss="L1", C=1.0, bias=True, options="", C_pos=None, C_neg=None, sample_dtype=None):
        """options: a PETSc-style option string for the solver (-qps_rtol 1e-6, -qps_mpgp_*, -qps_smalxe_*, -smalxe_qps_* ...) and -svm_loss_type / -svm_C /
        -svm_bias, which override the keyword arguments.  C_pos / C_neg: the penalty of the samples with y = +1 / y = -1 (None: C).  sample_dtype: the type
        dense samples are stored in on the device, training and test samples alike -- None or numpy.float64: fp64, whatever X holds; numpy.float32: float32
        (pmh_svm_create_f32: half the memory and traffic of X; alpha, w, b and all arithmetic stay fp64; a float64 X is rounded, sparse samples are
        refused).  svm.sample_dtype reports it."""
        self.C_pos, self.C_neg = C_pos, C_neg
        self.sample_dtype = sample_dtype_of(sample_dtype, False, "SVM")
        super().__init__(ctx, loss, C, bias, options)

    def create(self, X, y, sample_weight=None):
        """Set the training samples (X: (n, d) row-major ndarray or scipy.sparse matrix, y: +-1) and build the solver without training.  sample_weight: n
        positive numbers that scale the samples' penalties (None: all 1)."""
        sample_dtype_of(self.sample_dtype, is_sparse(X), "SVM")  # (float32 with sparse samples is refused)
        self._create_handle(X, y)
        if self.C_pos is not None or self.C_neg is not None or sample_weight is not None:
            self.set_penalties(self.C_pos, self.C_neg, sample_weight)
        return self

    def set_penalties(self, C_pos=None, C_neg=None, sample_weight=None):
        """C_i = (y_i > 0 ? C_pos : C_neg) sample_weight_i on the created handle (pmh_svm_set_penalties; None: C, C, all 1); the handle is untrained afterwards."""
        self._need()
        with self._lent(sample_weight) as wd:
            if wd is not None and wd.n != self.n:
                raise ValueError("SVM: sample_weight must have %d entries" % self.n)
            check(self.L.pmh_svm_set_penalties(self.h, float(self.C if C_pos is None else C_pos), float(self.C if C_neg is None else C_neg), wd.p if wd is not None else None))
        return self

    def set_labels(self, y):
        """New labels (+-1) on the created handle, X staying on the device (pmh_svm_set_labels): no upload of X, no new column-ordered copy.  y: an array, or a
        Vec -- also the very Vec handed over before, overwritten in place.  The penalties go back to C (set them again afterwards: labels, then penalties) and
        the handle is untrained; train() then gives what a fresh fit on (X, y) gives, bit for bit."""
        self._need()
        yd = self._dev(y)
        if yd.n != self.n:
            if yd is not y:
                yd.free()
            raise ValueError("SVM: y must have %d entries" % self.n)
        try:
            check(self.L.pmh_svm_set_labels(self.h, yd.p))
        except Exception:
            # the handle may borrow either buffer now and has no solver (train raises): it is of no further use, so both buffers go with it
            self._keep = (self._keep[0], self._keep[1]) + ((yd,) if yd is not y and yd is not self._keep[1] else ())
            self.destroy()
            raise
        Xd, old = self._keep
        self._keep = (Xd, yd)
        if old is not yd and old is not y:
            old.free()
        return self

    def set_subset(self, mask):
        """Train on the samples where mask is true, X staying on the device (pmh_svm_set_subset): n booleans or 0 / 1 numbers; None: all samples again.  The
        handle is untrained and uncalibrated afterwards; set_labels and set_penalties keep the subset.  After train() alpha is 0 on the held-out samples and
        the model is that of a fit on (X[mask], y[mask]); decision_function_own / test_own score the held-out samples without an upload."""
        self._need()
        if mask is None:
            check(self.L.pmh_svm_set_subset(self.h, None))
            return self
        m = np.ascontiguousarray(mask, dtype=np.float64).ravel()
        if m.size != self.n:
            raise ValueError("SVM: the mask must have %d entries" % self.n)
        with self._lent(m) as md:
            check(self.L.pmh_svm_set_subset(self.h, md.p))
        return self

    @property
    def subset(self):
        """The training mask as n booleans (pmh_svm_get_subset), or None where all samples train."""
        self._need()
        k = ct.c_longlong()
        check(self.L.pmh_svm_get_subset(self.h, None, ct.byref(k)))
        m = self._get_vec(lambda h, p: self.L.pmh_svm_get_subset(h, p, None)) != 0.0
        return None if m.all() else m

    def train(self, warm_start=False, alpha_scale=1.0):
        """Train from alpha = 0 (pmh_svm_train).  warm_start: from warm_start_vector(alpha_scale) of the handle's last dual and, with a bias, from its last
        multiplier (pmh_svm_train_warm) -- after set_penalties (alpha_scale = C_new / C_old scales the dual with its bounds) or set_subset; not after set_labels."""
        self._need()
        check(self.L.pmh_svm_train_warm(self.h, float(alpha_scale)) if warm_start else self.L.pmh_svm_train(self.h))
        return self

    def warm_start_vector(self, alpha_scale=1.0):
        """(n,): the vector train(warm_start=True, alpha_scale) starts from (pmh_svm_warm_start_vector): min(max(alpha_scale alpha, 0), C_i) on the subset
        (L2: no upper bound), 0 on the held-out samples.  warm_start_counts then says how many entries the mask zeroed and how many the bound clipped."""
        return self._get_vec(lambda h, p: self.L.pmh_svm_warm_start_vector(h, float(alpha_scale), p))

    @property
    def warm_start_counts(self):
        """dict(masked, clipped) of the last start vector formed (pmh_svm_get_warm_start_counts)."""
        self._need()
        m, c = ct.c_longlong(), ct.c_longlong()
        check(self.L.pmh_svm_get_warm_start_counts(self.h, ct.byref(m), ct.byref(c)))
        return dict(masked=m.value, clipped=c.value)

    def _get_vec(self, entry):
        self._need()
        with _vecs(self.ctx, self.n) as (v,):
            check(entry(self.h, v.p))
            return v.to_numpy()

    @property
    def penalties(self):
        """The effective penalty C_i of every training sample (pmh_svm_get_penalties)."""
        return self._get_vec(self.L.pmh_svm_get_penalties)

    def fit(self, X, y, sample_weight=None):
        self.create(X, y, sample_weight)
        check(self.L.pmh_svm_train(self.h))
        return self

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
        return self._get_vec(self.L.pmh_svm_get_dual)

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

    def _test_samples(self, X):
        """X for a scoring call: refused before any upload unless it is (n, d)."""
        self._need()
        S = _Samples(self.ctx, X, dtype=self.sample_dtype)
        if S.X.ndim != 2 or S.X.shape[1] != self.d:
            raise ValueError("SVM: X must be (n, %d)" % self.d)
        return S

    def _predict(self, X, want_scores, want_labels):
        S = self._test_samples(X)
        with S as (n, xa), _vecs(self.ctx, n if want_scores else None, n if want_labels else None) as (s, l):
            check(self._entry("predict", S)(self.h, *xa, s.p if s else None, l.p if l else None))
            return (s.to_numpy() if s else None, l.to_numpy() if l else None)

    def decision_function(self, X):
        return self._predict(X, True, False)[0]

    def predict(self, X):
        return self._predict(X, False, True)[1]

    def calibrate(self, X, y):
        """Fit the probability model of the trained handle on the samples X with labels y = +-1 (pmh_svm_calibrate): exactly platt_fit of
        decision_function(X).  train, set_labels and set_penalties clear it."""
        self._need()
        with self._lent(y) as yd:
            S = _Samples(self.ctx, X, dtype=self.sample_dtype)
            if S.X.ndim != 2 or S.X.shape[1] != self.d or S.X.shape[0] != yd.n:
                raise ValueError("SVM: X must be (%d, %d)" % (yd.n, self.d))
            with S as (n, xa):
                check(self._entry("calibrate", S)(self.h, *xa, yd.p))
        return self

    def set_calibration(self, A, B):
        """A saved pair (A, B) in place of calibrate."""
        self._need()
        check(self.L.pmh_svm_set_calibration(self.h, float(A), float(B)))
        return self

    @property
    def calibration(self):
        """(A, B) of the probability model."""
        self._need()
        A, B = ct.c_double(), ct.c_double()
        check(self.L.pmh_svm_get_calibration(self.h, ct.byref(A), ct.byref(B), None))
        return A.value, B.value

    @property
    def calibration_stats(self):
        """pmh_svm_platt_stats of the fit behind calibration (reason 0: the pair was set)."""
        self._need()
        st = _lib.SvmPlattStats()
        check(self.L.pmh_svm_get_calibration(self.h, None, None, ct.byref(st)))
        return st

    def predict_proba(self, X):
        """(n,): P(y = +1 | x_i) = 1 / (1 + exp(A decision_function(x_i) + B)), in one pass over X (pmh_svm_predict_proba)."""
        S = self._test_samples(X)
        with S as (n, xa), _vecs(self.ctx, n) as (p,):
            check(self._entry("predict_proba", S)(self.h, *xa, p.p))
            return p.to_numpy()

    def decision_function_own(self):
        """(n,): the scores of the samples the handle was created on, held-out ones included, without an upload (pmh_svm_predict_own): bit for bit
        decision_function(X)."""
        return self._get_vec(lambda h, p: self.L.pmh_svm_predict_own(h, p, None))

    OWN = {"held_out": 0, "subset": 1, "all": 2}  # PMH_SVM_OWN_*

    def test_own(self, which="held_out"):
        """Confusion counts of the handle's own samples against its labels over the held-out samples, the subset or all of them (pmh_svm_test_own), as test
        returns them: dict(TP, FP, TN, FN, accuracy)."""
        self._need()
        if which not in self.OWN:
            raise ValueError("SVM: which must be one of %s" % ", ".join(sorted(self.OWN)))
        cnt = (ct.c_longlong * 4)()
        check(self.L.pmh_svm_test_own(self.h, self.OWN[which], cnt))
        tp, fp, tn, fn = (int(c) for c in cnt)
        n = tp + fp + tn + fn
        return dict(TP=tp, FP=fp, TN=tn, FN=fn, accuracy=(tp + tn) / n if n else float("nan"))

    def test(self, X, y):
        """Confusion counts of the predicted labels against y: dict(TP, FP, TN, FN, accuracy)."""
        self._need()
        cnt = (ct.c_longlong * 4)()
        S = _Samples(self.ctx, X, dtype=self.sample_dtype)
        with S as (n, xa):
            yd = self._dev(y)
            try:
                check(self._entry("test", S)(self.h, *xa, yd.p, cnt))
            finally:
                yd.free()  # (also the caller's own Vec)
        tp, fp, tn, fn = (int(c) for c in cnt)
        return dict(TP=tp, FP=fp, TN=tn, FN=fn, accuracy=(tp + tn) / n if n else float("nan"))


class SVMMulticlass(_SVMHandle):
    """One-vs-rest linear SVM for two or more classes (pmh_svm_multi_*, csrc/svm_multi.hip).  The classes are the distinct labels, ascending; class k is trained
    against the rest on ONE binary handle over X (uploaded once; in CSR the operator's column-ordered copy is built once), which gives W (K, d) and b (K).
    Two classes train two classifiers: SVM is there for that case.  balanced: class k is trained with C_pos = C n / (2 n_k), C_neg = C n / (2 (n - n_k)).
    decision_function / predict score all K classes in one pass over X per chunk of classes (SVMMulticlass.chunk); the label is the class of the greatest score,
    ties to the lowest class.  X: (n, d) ndarray (d <= 256) or scipy.sparse, as in SVM.  One GPU."""

    _who, _pre = "SVMMulticlass", "pmh_svm_multi_"

    def __init__(self, ctx, loss="L1", C=1.0, bias=True, options="", balanced=False):
        super().__init__(ctx, loss, C, bias, options)
        self.balanced = bool(balanced)

    @staticmethod
    def chunk(path):
        """Classes scored per pass over the test samples (pmh_svm_multi_chunk) on the kernel path "dense64" (d = 64), "dense" (any other d) or "csr"."""
        kc = ct.c_int()
        check(_lib.load().pmh_svm_multi_chunk(("dense64", "dense", "csr").index(path), ct.byref(kc)))
        return kc.value

    def create(self, X, labels):
        """Set the training samples and find the classes, without training (then fit's train, or set_model)."""
        self._create_handle(X, labels, int(self.balanced))
        k = ct.c_int()
        check(self.L.pmh_svm_multi_get_classes(self.h, ct.byref(k), None))
        self.K = k.value
        return self

    def train(self):
        self._need()
        check(self.L.pmh_svm_multi_train(self.h))
        return self

    def fit(self, X, labels):
        return self.create(X, labels).train()

    def set_subset(self, mask):
        """Train the K problems on the samples where mask is true, X staying on the device (pmh_svm_multi_set_subset): n booleans or 0 / 1 numbers; None: all
        samples again.  The classes stay those of all labels; a mask that leaves a class without a sample is refused (PMH_ERR_ARG) and the handle stays as it
        was.  The handle is untrained and uncalibrated afterwards; set_model keeps the subset.  balanced: the penalties follow the counts over the subset.
        decision_function_own / predict_own / test_own score the handle's own samples without an upload."""
        self._need()
        if mask is None:
            check(self.L.pmh_svm_multi_set_subset(self.h, None))
            return self
        m = np.ascontiguousarray(mask, dtype=np.float64).ravel()
        if m.size != self.n:
            raise ValueError("SVMMulticlass: the mask must have %d entries" % self.n)
        with self._lent(m) as md:
            check(self.L.pmh_svm_multi_set_subset(self.h, md.p))
        return self

    @property
    def subset(self):
        """The training mask as n booleans (pmh_svm_multi_get_subset), or None where all samples train."""
        self._need()
        with _vecs(self.ctx, self.n) as (v,):
            check(self.L.pmh_svm_multi_get_subset(self.h, v.p, None, None))
            m = v.to_numpy() != 0.0
        return None if m.all() else m

    @property
    def subset_class_counts(self):
        """(K,) int64: the samples of each class inside the subset; over all samples where no subset is set."""
        self._need()
        c = np.zeros(self.K, dtype=np.int64)
        check(self.L.pmh_svm_multi_get_subset(self.h, None, None, c.ctypes.data_as(ct.c_void_p)))
        return c

    @property
    def classes_(self):
        self._need()
        c = np.empty(self.K)
        check(self.L.pmh_svm_multi_get_classes(self.h, None, c.ctypes.data_as(ct.c_void_p)))
        return c

    @property
    def W(self):
        self._need()
        W = np.empty((self.K, self.d))
        check(self.L.pmh_svm_multi_get_model(self.h, W.ctypes.data_as(ct.c_void_p), None))
        return W

    @property
    def b(self):
        self._need()
        b = np.empty(self.K)
        check(self.L.pmh_svm_multi_get_model(self.h, None, b.ctypes.data_as(ct.c_void_p)))
        return b

    @property
    def stats(self):
        """The statistics of the K trainings, class by class (a list of pmh_svm_stats)."""
        self._need()
        out = []
        for k in range(self.K):
            st = _lib.SvmStats()
            check(self.L.pmh_svm_multi_get_stats(self.h, k, ct.byref(st), None, None))
            out.append(st)
        return out

    def class_penalties(self, k):
        """(C_pos, C_neg) class k is trained with."""
        self._need()
        cp, cn = ct.c_double(), ct.c_double()
        check(self.L.pmh_svm_multi_get_stats(self.h, int(k), None, ct.byref(cp), ct.byref(cn)))
        return cp.value, cn.value

    def set_model(self, W, b):
        """A saved model in place of training: W (K, d), b (K)."""
        self._need()
        W, b = np.ascontiguousarray(W, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64).ravel()
        if W.shape != (self.K, self.d) or b.shape != (self.K,):
            raise ValueError("SVMMulticlass: W must be (%d, %d) and b (%d,)" % (self.K, self.d, self.K))
        check(self.L.pmh_svm_multi_set_model(self.h, W.ctypes.data_as(ct.c_void_p), b.ctypes.data_as(ct.c_void_p)))
        return self

    def _run(self, X, want_scores, want_labels, labels_true=None):
        """predict (scores and / or labels) or, with labels_true, test: (scores, labels) or (confusion, n_unknown)."""
        self._need()
        S = _Samples(self.ctx, X)
        if S.X.ndim != 2:
            raise ValueError("SVMMulticlass: X must be (n, d)")
        with S as (n, xa), _vecs(self.ctx, n * self.K if want_scores else None, n if want_labels else None) as (s, l), self._lent(labels_true) as t:
            if t is not None and t.n != n:
                raise ValueError("SVMMulticlass: labels must have %d entries" % n)
            if not S.sparse and S.X.shape[1] != self.d:  # (a sparse X of another width is the library's to refuse)
                raise ValueError("SVMMulticlass: X must be (n, %d)" % self.d)
            if t is not None:
                conf, unk = np.zeros((self.K, self.K), dtype=np.int64), ct.c_longlong()
                check(self._entry("test", S)(self.h, *xa, t.p, conf.ctypes.data_as(ct.c_void_p), ct.byref(unk)))
                return conf, int(unk.value)
            check(self._entry("predict", S)(self.h, *xa, s.p if s else None, l.p if l else None))
            return (s.to_numpy().reshape(n, self.K) if s else None, l.to_numpy() if l else None)

    def calibrate(self, X, labels):
        """Fit the K probability models on the samples X with true labels (pmh_svm_multi_calibrate): model k is platt_fit of column k of decision_function(X)
        with "label == class k" as +1; a label that is no class counts among the rest.  train and set_model clear them."""
        self._need()
        S = _Samples(self.ctx, X)
        with self._lent(labels) as ld:
            if S.X.ndim != 2 or S.X.shape[1] != self.d or S.X.shape[0] != ld.n:
                raise ValueError("SVMMulticlass: X must be (%d, %d)" % (ld.n, self.d))
            with S as (n, xa):
                check(self._entry("calibrate", S)(self.h, *xa, ld.p))
        return self

    def set_calibration(self, A, B):
        """Saved pairs in place of calibrate: A (K), B (K)."""
        self._need()
        A, B = np.ascontiguousarray(A, dtype=np.float64).ravel(), np.ascontiguousarray(B, dtype=np.float64).ravel()
        if A.shape != (self.K,) or B.shape != (self.K,):
            raise ValueError("SVMMulticlass: A and B must have %d entries each" % self.K)
        check(self.L.pmh_svm_multi_set_calibration(self.h, A.ctypes.data_as(ct.c_void_p), B.ctypes.data_as(ct.c_void_p)))
        return self

    @property
    def calibration(self):
        """(A, B), two K-vectors: the classes' probability models."""
        self._need()
        A, B = np.empty(self.K), np.empty(self.K)
        check(self.L.pmh_svm_multi_get_calibration(self.h, A.ctypes.data_as(ct.c_void_p), B.ctypes.data_as(ct.c_void_p), None))
        return A, B

    @property
    def calibration_stats(self):
        """The K fits' pmh_svm_platt_stats, class by class."""
        self._need()
        st = (_lib.SvmPlattStats * self.K)()
        check(self.L.pmh_svm_multi_get_calibration(self.h, None, None, ct.cast(st, ct.c_void_p)))
        return list(st)

    def predict_proba(self, X):
        """(n, K): sigma_ik = 1 / (1 + exp(A_k score_ik + B_k)), every row divided by its sum (a row of zeros: 1 / K); one pass over X per chunk of classes."""
        self._need()
        S = _Samples(self.ctx, X)
        if S.X.ndim != 2 or S.X.shape[1] != self.d:
            raise ValueError("SVMMulticlass: X must be (n, %d)" % self.d)
        with S as (n, xa), _vecs(self.ctx, n * self.K) as (p,):
            check(self._entry("predict_proba", S)(self.h, *xa, p.p))
            return p.to_numpy().reshape(n, self.K)

    def decision_function(self, X):
        """(n, K): x_i . W_k + b_k."""
        return self._run(X, True, False)[0]

    def predict(self, X):
        return self._run(X, False, True)[1]

    def predict_both(self, X):
        """(scores (n, K), labels (n,)) from one call."""
        return self._run(X, True, True)

    def test(self, X, labels):
        """dict(accuracy, confusion, n_unknown): confusion[t, p] counts the samples of true class t predicted as class p; a true label that is no class is
        counted in n_unknown; accuracy = trace / n."""
        conf, unk = self._run(X, False, False, labels_true=labels)
        n = X.shape[0]
        return dict(accuracy=float(np.trace(conf)) / n if n else float("nan"), confusion=conf, n_unknown=unk)

    def _run_own(self, want_scores, want_labels):
        self._need()
        n = self.n
        with _vecs(self.ctx, n * self.K if want_scores else None, n if want_labels else None) as (s, l):
            check(self.L.pmh_svm_multi_predict_own(self.h, s.p if s else None, l.p if l else None))
            return (s.to_numpy().reshape(n, self.K) if s else None, l.to_numpy() if l else None)

    def decision_function_own(self):
        """(n, K): the scores of the samples the handle was created on, held-out ones included, without an upload (pmh_svm_multi_predict_own): bit for bit
        decision_function(X)."""
        return self._run_own(True, False)[0]

    def predict_own(self):
        """(n,): the labels of the handle's own samples, bit for bit predict(X)."""
        return self._run_own(False, True)[1]

    OWN = SVM.OWN  # PMH_SVM_OWN_*

    def test_own(self, which="held_out"):
        """The handle's own samples against its training labels over the held-out samples, the subset or all of them (pmh_svm_multi_test_own), nothing
        uploaded; dense samples that are not selected are not read.  -> dict(accuracy, confusion, n): confusion as test returns it, n the samples counted,
        accuracy = trace / n."""
        self._need()
        if which not in self.OWN:
            raise ValueError("SVMMulticlass: which must be one of %s" % ", ".join(sorted(self.OWN)))
        conf, n = np.zeros((self.K, self.K), dtype=np.int64), ct.c_longlong()
        check(self.L.pmh_svm_multi_test_own(self.h, self.OWN[which], conf.ctypes.data_as(ct.c_void_p), ct.byref(n)))
        n = int(n.value)
        return dict(accuracy=float(np.trace(conf)) / n if n else float("nan"), confusion=conf, n=n)


def kfold(y, k, seed=0, stratified=True):
    """k boolean training masks over the samples of y whose complements (the folds) partition them.  One seeded shuffle, then the samples are dealt to the
    folds round-robin -- stratified: class by class (classes ascending), the deal going on where the previous class stopped, so every fold's share of a class
    and of the whole differs from another fold's by at most one sample.  A class of fewer than k samples leaves some folds without it.  Host only."""
    y = np.asarray(y).ravel()
    n, k = y.size, int(k)
    if k < 2 or k > n:
        raise ValueError("kfold: k = %d, need 2 <= k <= n = %d" % (k, n))
    perm = np.random.default_rng(seed).permutation(n)
    if stratified:
        order = np.concatenate([perm[y[perm] == c] for c in np.unique(y)])
    else:
        order = perm
    fold = np.empty(n, dtype=np.int64)
    fold[order] = np.arange(n) % k
    return [fold != f for f in range(k)]


def cross_validate(svm, k=5, seed=0, stratified=True):
    """k-fold cross-validation on a created SVM handle, X uploaded once (CSR: one column-ordered copy): for every mask of kfold(y, k, seed, stratified)
    set_subset, train, test_own("held_out").  -> dict(folds: the k dicts of test_own, accuracy: their mean accuracy, masks).  The handle gets back the subset
    it had and is left untrained.  An SVMMulticlass handle is cross-validated the same way, the masks stratified over its K classes, and the result has
    confusion, the sum of the folds' K x K matrices, as well; a class of one sample leaves one fold's training set without it, and set_subset's PMH_ERR_ARG
    comes through (the subset is still restored).
    An SVR handle is cross-validated the same way.  Its targets are continuous, so `stratified` does not apply to it: the masks are kfold(t, k, seed,
    stratified=False) whatever is passed.  -> dict(folds: the k dicts of test_own, masks, and the metrics pooled over the k held-out sets by pooled_metrics: mse,
    mae, r2, n from the folds' summed sum_r2, sum_abs_r, sum_t, sum_t2, n; max_abs: the maximum over the folds)."""
    svm._need()
    before = svm.subset
    y = svm._keep[1].to_numpy()
    regression = svm._who == "SVR"
    masks = kfold(y, k, seed, stratified and not regression)
    folds = []
    try:
        for m in masks:
            folds.append(svm.set_subset(m).train().test_own("held_out"))
    finally:
        svm.set_subset(before)
    if regression:
        return dict(folds=folds, masks=masks, **pooled_metrics(folds))
    out = dict(folds=folds, accuracy=float(np.mean([f["accuracy"] for f in folds])), masks=masks)
    if isinstance(svm, SVMMulticlass):
        out["confusion"] = sum(f["confusion"] for f in folds)
    return out


def pooled_metrics(folds):
    """The regression metrics over the union of the folds' samples from the sums SVR.test / test_own return: dict(n, mse = sum_r2 / n, mae = sum_abs_r / n,
    r2 = 1 - sum_r2 / (sum_t2 - sum_t^2 / n), max_abs = the largest of the folds'), each sum added over the folds in their order.  nan where n is 0, r2 also
    where the pooled targets are constant.  Host arithmetic."""
    tot = {key: sum(f[key] for f in folds) for key in ("sum_r2", "sum_abs_r", "sum_t", "sum_t2", "n")}
    n = int(tot["n"])
    nan = float("nan")
    sst = tot["sum_t2"] - tot["sum_t"] ** 2 / n if n else 0.0
    return dict(n=n, mse=tot["sum_r2"] / n if n else nan, mae=tot["sum_abs_r"] / n if n else nan, r2=1.0 - tot["sum_r2"] / sst if n and sst > 0.0 else nan,
                max_abs=max((f["max_abs"] for f in folds), default=0.0))


SCORES = ("accuracy", "precision", "recall", "specificity", "f1", "balanced_accuracy", "mcc")


def scores(counts):
    """The scores of confusion counts: dict(TP, FP, TN, FN) as test / test_own return it, or a list of such dicts (summed) -> dict of SCORES.  A score whose
    denominator is 0 is nan, except mcc, which is 0 there.  Host arithmetic."""
    if isinstance(counts, dict):
        counts = [counts]
    tp, fp, tn, fn = (sum(int(c[k]) for c in counts) for k in ("TP", "FP", "TN", "FN"))
    div = lambda a, b: a / b if b else float("nan")
    prec, rec, spec = div(tp, tp + fp), div(tp, tp + fn), div(tn, tn + fp)
    den = (tp + fp) * (tp + fn) * (tn + fp) * (tn + fn)  # (Python integers: exact)
    return dict(accuracy=div(tp + tn, tp + fp + tn + fn), precision=prec, recall=rec, specificity=spec, f1=div(2 * tp, 2 * tp + fp + fn),
                balanced_accuracy=(rec + spec) / 2, mcc=(tp * tn - fp * fn) / math.sqrt(den) if den else 0.0)


def select_C(Cs, score):
    """(C, its index in Cs) of the highest score; among equal scores the smallest C; a nan never wins; all nan: ValueError.  Cs in any order.  Host only."""
    best = None
    for g in np.argsort(np.asarray(Cs, dtype=np.float64), kind="stable"):
        if not np.isnan(score[g]) and (best is None or score[g] > score[best]):
            best = int(g)
    if best is None:
        raise ValueError("grid_search: every score is nan")
    return float(Cs[best]), best


def _grid(Cs, score):
    """Cs as an ascending list of floats; ValueError for an empty list, a value that is not positive and finite, or an unknown score."""
    if score not in SCORES:
        raise ValueError("grid_search: score must be one of %s" % ", ".join(SCORES))
    Cs = sorted(float(c) for c in np.asarray(Cs, dtype=np.float64).ravel())
    if not Cs:
        raise ValueError("grid_search: Cs is empty")
    if not all(c > 0.0 and np.isfinite(c) for c in Cs):
        raise ValueError("grid_search: every C must be positive and finite")
    return Cs


def grid_search(svm, Cs, k=5, seed=0, stratified=True, score="accuracy", warm_start=True, sample_weight=None, refit=True, return_models=False):
    """Choose C by k-fold cross-validation on a created SVM handle, X uploaded once.  Cs: absolute values of C, sorted ascending here; C_pos and C_neg keep the
    ratio to C they were constructed with (C_pos_g = C_g C_pos / C) and sample_weight goes to set_penalties at every grid point.  For every mask of
    kfold(y, k, seed, stratified) set_subset once, then C ascending: set_penalties, train, test_own("held_out") -- the first C of a fold from zero, every later
    one with warm_start from the previous C's solution (alpha_scale = C_g / C_{g-1}); warm_start=False: all from zero, which gives exactly what the same loop
    written by hand gives.
    -> dict(Cs, counts[g][f] (test_own's dicts), score[g] (`score` of the counts summed over the folds; any of SCORES), nmv[g][f], passes_X[g][f], best_index,
    best_C (the highest score, the smallest C among equals, a nan never), masks; return_models: W[g][f], b[g][f]).
    The handle gets back the subset it had.  refit: it is left with best_C's penalties and trained on that subset; else with the penalties it was constructed
    with (and sample_weight), untrained.  SVM only: SVMMulticlass is not covered."""
    svm._need()
    Cs = _grid(Cs, score)
    ratio = lambda c: 1.0 if c is None else float(c) / svm.C
    pen = lambda C: svm.set_penalties(C * ratio(svm.C_pos), C * ratio(svm.C_neg), sample_weight)
    before = svm.subset
    masks = kfold(svm._keep[1].to_numpy(), k, seed, stratified)
    cell = lambda: [[None] * len(masks) for _ in Cs]
    counts, nmv, passes, W, b = cell(), cell(), cell(), cell(), cell()
    try:
        for f, m in enumerate(masks):
            svm.set_subset(m)
            for g, C in enumerate(Cs):
                pen(C)
                if warm_start and g > 0:
                    svm.train(warm_start=True, alpha_scale=C / Cs[g - 1])
                else:
                    svm.train()
                t = svm.test_own("held_out")
                st = svm.stats
                counts[g][f], nmv[g][f], passes[g][f] = t, st.nmv, st.passes_X
                if return_models:
                    W[g][f], b[g][f] = svm.w, svm.b
    finally:
        svm.set_subset(before)
    sc = [scores(row)[score] for row in counts]
    best_C, best = select_C(Cs, sc)
    out = dict(Cs=Cs, counts=counts, score=sc, nmv=nmv, passes_X=passes, best_index=best, best_C=best_C, masks=masks)
    if return_models:
        out.update(W=W, b=b)
    if refit:
        pen(best_C)
        svm.train()
    else:
        svm.set_penalties(svm.C_pos, svm.C_neg, sample_weight)
    return out


def load_svmlight(path, n_features=None, zero_based="auto", multiclass=False):
    """Read a file in the svmlight / libsvm text format, `label idx:val idx:val ...` per sample, into (X, y): X a scipy.sparse CSR matrix (fp64, int32, sorted
    indices, duplicates summed), y in {-1, +1}.  Text after `#` is a comment; `qid:` tokens are ignored; a sample may have no feature.  The labels must take
    exactly two distinct values: the smaller becomes -1, the larger +1; multiclass=True: y is the labels as read, two or more distinct values (SVMMulticlass).  zero_based: True / False, or "auto" (one-based unless an index 0 occurs).
    n_features: the width of X (default: the largest index + 1 after the shift); an index beyond it is an error."""
    import scipy.sparse as sp

    labels, indptr, idx, val = [], [0], [], []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            t = line.split("#", 1)[0].split()
            if not t:
                continue
            try:
                labels.append(float(t[0]))
                for tok in t[1:]:
                    k, v = tok.split(":", 1)
                    if k == "qid":
                        continue
                    idx.append(int(k))
                    val.append(float(v))
            except ValueError:
                raise ValueError("%s:%d: not in the svmlight format: %r" % (path, ln, line.strip())) from None
            indptr.append(len(idx))
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size and idx.min() < 0:
        raise ValueError("%s: negative feature index" % path)
    if zero_based == "auto":
        zero_based = bool(idx.size and idx.min() == 0)
    if not zero_based:
        if idx.size and idx.min() < 1:
            raise ValueError("%s: feature index 0 in a one-based file" % path)
        idx = idx - 1
    d = int(idx.max()) + 1 if idx.size else 0
    if n_features is not None:
        if d > n_features:
            raise ValueError("%s: feature index %d with n_features = %d" % (path, d - 1, n_features))
        d = int(n_features)
    lab = np.asarray(labels, dtype=np.float64)
    u = np.unique(lab)
    if multiclass:
        if u.size < 2:
            raise ValueError("%s: %d distinct labels, a classifier needs at least two" % (path, u.size))
        y = lab
    else:
        if u.size != 2:
            raise ValueError("%s: %d distinct labels, a binary classifier needs exactly two" % (path, u.size))
        y = np.where(lab == u[1], 1.0, -1.0)
    X = sp.csr_matrix((np.asarray(val, dtype=np.float64), idx.astype(np.int32), np.asarray(indptr, dtype=np.int32)), shape=(lab.size, d))
    X.sum_duplicates()
    X.sort_indices()
    return X, y
