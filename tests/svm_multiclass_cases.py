"""Inputs and bounds shared by tests/test_gpu_svm_multiclass.py and tests/test_svm_multiclass_host.py (no test in here): the scoring cases -- a model
W ~ N(0,1), b ~ N(0,1) and test samples from a seed -- with numpy's scores, the entrywise bound on a score and the rows whose arg-max the bound leaves open."""
import numpy as np

EPS = np.finfo(float).eps
DENSE_D = (1, 63, 64, 65, 256)
DENSE_N = (1, 2, 67, 1025)
CSR_D = 5000
SPAN = 2048  # SVC_SPAN of csrc/svm_csr_seg.h: stored entries per workgroup


def chunk_Ks(KC):
    """The class counts of the scoring tests: one chunk exactly, one more, two classes, one short of three chunks."""
    return (KC, KC + 1, 2, 3 * KC - 1)


def model(d, K, seed=0):
    rng = np.random.default_rng(1000 * d + K + seed)
    return rng.standard_normal((K, d)), rng.standard_normal(K)


def dense_samples(n, d):
    return np.random.default_rng(7919 * d + n).standard_normal((n, d))


def csr_samples(which):
    """"many": 49 samples, among them samples without entries, with one entry, with 3000 and 2100 (each begins in one span and ends in the next) and with 4500
    (a whole span lies inside it), the rest short, so that one span holds many samples; "one": a single sample of 3000 entries."""
    import scipy.sparse as sp

    rng = np.random.default_rng(11 if which == "many" else 12)
    lens = [3000] if which == "one" else [5, 0, 1, 17, 3000, 0, 9, 1, 60, 2100, 4500] + [int(v) for v in rng.integers(0, 40, 37)] + [0]
    assert max(lens) > SPAN
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.concatenate([np.sort(rng.choice(CSR_D, size=m, replace=False)) for m in lens]).astype(np.int32)
    val = rng.standard_normal(idx.size)
    return sp.csr_matrix((val, idx, indptr), shape=(len(lens), CSR_D))


def reference(X, W, b):
    """numpy's scores X W' + b, the entrywise bound 4 (m + 2) eps (|X| |W|' + |b|) with m = d (dense) or the sample's number of entries (CSR: the standard
    bound of a recursive sum of m products and one addition, with margin for the tree order), and the rows whose label the bound leaves open: top-two gap <=
    twice the row's largest bound."""
    if hasattr(X, "tocsr"):
        m = np.diff(X.indptr).astype(np.float64)[:, None]
        S = np.asarray(X @ W.T) + b
        A = np.asarray(abs(X) @ np.abs(W).T) + np.abs(b)
    else:
        m = float(X.shape[1])
        S = X @ W.T + b
        A = np.abs(X) @ np.abs(W).T + np.abs(b)
    bound = 4.0 * (m + 2.0) * EPS * A
    if W.shape[0] > 1:
        top = np.sort(S, axis=1)
        open_rows = (top[:, -1] - top[:, -2]) <= 2.0 * bound.max(axis=1)
    else:
        open_rows = np.zeros(S.shape[0], dtype=bool)
    return S, bound, open_rows
