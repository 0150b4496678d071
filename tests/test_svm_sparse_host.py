"""Host-side pieces of the SVM on sparse samples: the svmlight reader and the sparse problem generator (no GPU)."""
import numpy as np
import pytest
import scipy.sparse as sp

from permon_amd import problems as P
from permon_amd.svm import load_svmlight


def _write(path, X, labels, one_based, qid=False, comment=True):
    X = X.tocsr()
    with open(path, "w") as fh:
        if comment:
            fh.write("# written by the test\n")
        for i in range(X.shape[0]):
            k0, k1 = X.indptr[i], X.indptr[i + 1]
            tok = ["%d:%r" % (c + (1 if one_based else 0), float(v)) for c, v in zip(X.indices[k0:k1], X.data[k0:k1])]
            if qid:
                tok.insert(0, "qid:%d" % (i % 3))
            fh.write(" ".join([repr(labels[i])] + tok) + ("  # sample %d\n" % i if i % 2 else "\n"))


@pytest.mark.parametrize("one_based", [True, False])
def test_load_svmlight_round_trip(tmp_path, one_based):
    rng = np.random.default_rng(3)
    X = sp.random(40, 25, density=0.2, random_state=5, format="lil")
    X[0, 0] = 1.5  # the smallest index occurs, so "auto" can tell the two conventions apart
    X.rows[7], X.data[7] = [], []  # an empty sample
    X = X.tocsr()
    lab = np.where(rng.random(40) < 0.5, 3, 8)  # two distinct values, neither +-1
    path = str(tmp_path / "data.svm")
    _write(path, X, lab.tolist(), one_based, qid=True)
    for zb in ("auto", not one_based):
        Y, y = load_svmlight(path, zero_based=zb)
        assert Y.shape == (40, int(X.indices.max()) + 1) and Y.dtype == np.float64 and Y.indices.dtype == np.int32 and Y.has_sorted_indices
        assert np.array_equal(Y.indptr, X.indptr) and np.array_equal(Y.indices, X.indices) and np.array_equal(Y.data, X.data)  # repr round-trips fp64
        assert np.array_equal(y, np.where(lab == 8, 1.0, -1.0))
        assert Y.indptr[8] == Y.indptr[7]
    Y, _ = load_svmlight(path, n_features=60)
    assert Y.shape == (40, 60) and Y.nnz == X.nnz
    with pytest.raises(ValueError):
        load_svmlight(path, n_features=3)


def test_load_svmlight_rejects_what_it_cannot_read(tmp_path):
    p = str(tmp_path / "bad.svm")
    open(p, "w").write("1 1:2.0\n2 2:1.0\n3 1:1.0\n")
    with pytest.raises(ValueError, match="distinct labels"):
        load_svmlight(p)
    open(p, "w").write("1 1:2.0\n-1 oops\n")
    with pytest.raises(ValueError, match="svmlight"):
        load_svmlight(p)
    open(p, "w").write("1 0:2.0\n-1 2:1.0\n")
    with pytest.raises(ValueError, match="one-based"):
        load_svmlight(p, zero_based=False)
    open(p, "w").write("+1 3:1 1:2 3:4\n-1\n")  # unsorted and repeated indices: sorted, summed
    X, y = load_svmlight(p)
    assert X.shape == (2, 3) and np.array_equal(X.toarray(), [[2.0, 0.0, 5.0], [0.0, 0.0, 0.0]]) and np.array_equal(y, [1.0, -1.0])


@pytest.mark.parametrize("args,nnz,cmax,cmed,cempty", [((4000, 5000, 30, 1.0, 0.5, 1.0), 100477, 3880, 6, 76), ((4000, 300, 12, 1.2, 0.5, 1.0), 34795, 3875, 31, 0),
                                                      ((3000, 20000, 40, 0.8, 0.5, 10.0), 115765, 2137, 3, 2091)])
def test_svm_sparse_statistics_and_determinism(args, nnz, cmax, cmed, cempty):
    p = P.svm_sparse(*args, N_test=50)
    X, y = p["X"], p["y"]
    cc = np.bincount(X.indices, minlength=args[1])
    assert (X.nnz, int(cc.max()), int(np.median(cc)), int((cc == 0).sum())) == (nnz, cmax, cmed, cempty)
    assert sp.issparse(X) and X.format == "csr" and X.has_sorted_indices and X.shape == (args[0], args[1])
    nr = np.sqrt(np.asarray(X.multiply(X).sum(axis=1)).ravel())
    assert np.allclose(nr[nr > 0], 1.0, rtol=1e-14, atol=0) and set(np.unique(y)) <= {-1.0, 1.0}
    assert set(p) >= {"n", "d", "X", "y", "C", "offset", "w_star", "b", "lb", "ub", "x0", "X_test", "y_test"} and p["C"] == args[5] and p["X_test"].shape == (50, args[1])
    q = P.svm_sparse(*args, N_test=50)
    assert np.array_equal(q["X"].indptr, X.indptr) and np.array_equal(q["X"].indices, X.indices) and np.array_equal(q["X"].data, X.data) and np.array_equal(q["y"], y)
    assert np.array_equal(q["X_test"].data, p["X_test"].data) and np.array_equal(q["y_test"], p["y_test"])
    r = P.svm_sparse(*args[:6], seed=8)
    assert r["X"].nnz != X.nnz or not np.array_equal(r["X"].indices, X.indices)
