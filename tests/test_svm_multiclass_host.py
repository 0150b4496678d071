"""The multiclass SVM without a GPU: the ABI (the entries are declared, listed and exported), load_svmlight(multiclass=True), problems.svm_blobs, and that numpy
alone leaves no label of the GPU scoring tests' cases open."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import svm_multiclass_cases as MC
from permon_amd import _lib
from permon_amd import problems as P
from permon_amd.svm import load_svmlight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["pmh_op_svm_dual_set_labels", "pmh_svm_set_labels", "pmh_svm_multi_chunk", "pmh_svm_multi_create", "pmh_svm_multi_create_csr", "pmh_svm_multi_train",
           "pmh_svm_multi_get_classes", "pmh_svm_multi_get_model", "pmh_svm_multi_set_model", "pmh_svm_multi_get_stats", "pmh_svm_multi_predict",
           "pmh_svm_multi_predict_csr", "pmh_svm_multi_test", "pmh_svm_multi_test_csr", "pmh_svm_multi_destroy"]


def _chunk(path):
    """pmh_svm_multi_chunk of path 0 (dense d = 64), 1 (dense, any other d), 2 (CSR)."""
    lib = C.CDLL(_lib.LIB_PATH)
    kc = C.c_int(0)
    assert lib.pmh_svm_multi_chunk(path, C.byref(kc)) == 0
    return kc.value


@pytest.mark.parametrize("name", ENTRIES)
def test_multiclass_entries_are_declared_listed_and_exported(name):
    header = open(os.path.join(ROOT, "include", "permon_hip.h")).read()
    assert re.search(r"^int %s\(" % name, header, re.M), "%s is not declared in permon_hip.h" % name
    assert name in _lib.EXPORTED
    lib = C.CDLL(_lib.LIB_PATH)  # (loading needs no GPU)
    assert hasattr(lib, name), "libpermonhip.so does not export %s" % name


def test_chunk_getter_needs_no_gpu():
    for path in range(3):
        kc = _chunk(path)
        assert kc >= 2 and kc & (kc - 1) == 0


def test_load_svmlight_multiclass(tmp_path):
    f = tmp_path / "three.svm"
    f.write_text("3 1:0.5 4:-2\n1 2:1.5  # a comment\n7\n3 1:1 3:2\n1 4:4\n")
    X, y = load_svmlight(str(f), multiclass=True)
    assert np.array_equal(y, [3.0, 1.0, 7.0, 3.0, 1.0])
    assert X.shape == (5, 4) and X.nnz == 6
    assert np.array_equal(X.toarray()[0], [0.5, 0.0, 0.0, -2.0]) and np.array_equal(X.toarray()[2], np.zeros(4))
    # the default keeps refusing more than two labels
    with pytest.raises(ValueError, match="3 distinct labels"):
        load_svmlight(str(f))
    # and two labels read as before, whichever way
    g = tmp_path / "two.svm"
    g.write_text("3 1:0.5\n1 2:1.5\n")
    assert np.array_equal(load_svmlight(str(g))[1], [1.0, -1.0])
    assert np.array_equal(load_svmlight(str(g), multiclass=True)[1], [3.0, 1.0])
    one = tmp_path / "one.svm"
    one.write_text("2 1:1\n2 2:1\n")
    with pytest.raises(ValueError, match="at least two"):
        load_svmlight(str(one), multiclass=True)


def test_svm_blobs_shapes_and_determinism():
    p = P.svm_blobs(50, 20, 5, 4.0, 3, N_test=11)
    assert p["X"].shape == (50, 20) and p["X_csr"].shape == (50, 20) and p["labels"].shape == (50,)
    assert p["X_test"].shape == (11, 20) and p["labels_test"].shape == (11,)
    assert np.array_equal(np.unique(p["labels"]), np.arange(5.0))
    assert np.array_equal(p["X_csr"].toarray(), p["X"])
    q = P.svm_blobs(50, 20, 5, 4.0, 3, N_test=11)
    assert np.array_equal(p["X"], q["X"]) and np.array_equal(p["X_test"], q["X_test"]) and np.array_equal(p["labels"], q["labels"])
    assert not np.array_equal(p["X"], P.svm_blobs(50, 20, 5, 4.0, 4)["X"])
    # the centre of class k is sep e_k: the class means stand out in their own column
    for k in range(5):
        assert abs(p["X"][p["labels"] == k, k].mean() - 4.0) < 1.5
    s = P.svm_blobs(40, 300, 4, 4.0, 3, sparse=10)
    assert s["X_csr"].shape == (40, 300) and s["X_csr"].has_sorted_indices
    assert (np.diff(s["X_csr"].indptr) <= 11).all() and (np.diff(s["X_csr"].indptr) >= 10).all()
    assert np.array_equal(s["X_csr"].toarray(), s["X"])
    with pytest.raises(ValueError):
        P.svm_blobs(10, 3, 4, 1.0, 0)


def test_numpy_leaves_no_label_of_the_scoring_cases_open():
    """The share of rows the GPU test may exclude from its arg-max comparison is, by numpy alone, 0 for every case: Gaussian scores do not tie to a few eps."""
    for d in MC.DENSE_D:
        for K in MC.chunk_Ks(_chunk(0 if d == 64 else 1)):
            W, b = MC.model(d, K)
            for n in MC.DENSE_N:
                assert not MC.reference(MC.dense_samples(n, d), W, b)[2].any(), (d, n, K)
    for K in MC.chunk_Ks(_chunk(2)):
        W, b = MC.model(MC.CSR_D, K)
        for which in ("many", "one"):
            assert not MC.reference(MC.csr_samples(which), W, b)[2].any(), (which, K)
