"""float32 samples without a GPU: the six new entries are declared in the header, listed in _lib.py, exported by the built library and named in
INTEGRATION.md; pmh_svm_opts keeps its six fields; what the Python front end refuses before anything reaches the device (sparse samples with float32, a finite
value that float32 cannot hold, a sample_dtype that is neither float32 nor float64); SVMMulticlass takes no sample_dtype."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import scipy.sparse as sp

from permon_amd import _lib
from permon_amd.core import sample_array
from permon_amd.mat import MatCreateSVMDual
from permon_amd.svm import SVM, SVMMulticlass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["pmh_op_create_svm_dual_f32", "pmh_svm_create_f32", "pmh_svm_predict_f32", "pmh_svm_test_f32", "pmh_svm_predict_proba_f32", "pmh_svm_calibrate_f32"]


@pytest.mark.parametrize("name", ENTRIES)
def test_f32_entries_are_declared_listed_and_exported(name):
    header = open(os.path.join(ROOT, "include", "permon_hip.h")).read()
    m = re.search(r"\bint %s\(([^)]*)\)" % name, header)
    assert m, name + " is not declared in include/permon_hip.h"
    assert "const float *X_dev" in m.group(1)
    assert name in _lib.EXPORTED, name + " is not declared in permon_amd/_lib.py"
    assert hasattr(_lib.load(), name), name + " is not exported by libpermonhip.so"
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_svm_opts_fields_are_unchanged():
    assert [name for name, _ in _lib.SvmOpts._fields_] == ["loss_type", "C", "bias", "qps", "mpgp", "smalxe"]
    body = re.search(r"typedef struct \{([^}]*)\} pmh_svm_opts;", open(os.path.join(ROOT, "include", "permon_hip.h")).read()).group(1)
    assert re.findall(r"(\w+);", body) == ["loss_type", "C", "bias", "qps", "mpgp", "smalxe"]


def _host_ctx():
    """What SVM's constructor needs of a context: the library (its option entries run on the host) and a handle no test here reaches."""
    return types.SimpleNamespace(L=_lib.load(), h=None)


def test_sample_dtype_is_reported_and_checked():
    assert SVM(_host_ctx()).sample_dtype is np.float64
    assert SVM(_host_ctx(), sample_dtype=np.float64).sample_dtype is np.float64
    assert SVM(_host_ctx(), sample_dtype=np.float32).sample_dtype is np.float32
    assert SVM(_host_ctx(), sample_dtype="float32").sample_dtype is np.float32
    for bad in (np.float16, np.int32, "no such type"):
        with pytest.raises(ValueError, match="sample_dtype"):
            SVM(_host_ctx(), sample_dtype=bad)
        with pytest.raises(ValueError, match="sample_dtype"):
            MatCreateSVMDual(None, np.zeros((3, 2)), np.ones(3), sample_dtype=bad)


def test_sparse_samples_with_float32_are_refused():
    X = sp.random(20, 30, density=0.2, format="csr", random_state=0)
    y = np.where(np.arange(20) % 2 == 0, 1.0, -1.0)
    with pytest.raises(ValueError, match="sparse"):
        SVM(_host_ctx(), sample_dtype=np.float32).create(X, y)
    with pytest.raises(ValueError, match="sparse"):
        SVM(_host_ctx(), sample_dtype=np.float32).fit(X, y)
    with pytest.raises(ValueError, match="sparse"):
        MatCreateSVMDual(None, X, y, sample_dtype=np.float32)


def test_overflow_on_rounding_is_refused():
    X = np.random.default_rng(0).standard_normal((10, 5))
    y = np.where(np.arange(10) % 2 == 0, 1.0, -1.0)
    X[3, 2], X[7, 0] = 1e300, -4e38  # finite in fp64, infinite in float32
    with pytest.raises(ValueError, match="2 finite values"):
        SVM(_host_ctx(), sample_dtype=np.float32).create(X, y)
    with pytest.raises(ValueError, match="2 finite values"):
        MatCreateSVMDual(None, X, y, sample_dtype=np.float32)
    # what rounds to a finite float32 goes through, rounded to nearest; an infinity that was one stays; float32 in is float32 out, untouched
    X[3, 2], X[7, 0] = 3.0e38, np.inf
    X32 = sample_array(X, np.float32, "t")
    assert X32.dtype == np.float32 and X32.flags.c_contiguous and np.array_equal(X32, X.astype(np.float32))
    assert sample_array(X32, np.float32, "t") is X32
    # without the argument a float32 array is widened, as ever
    assert sample_array(X32, np.float64, "t").dtype == np.float64


def test_multiclass_takes_no_sample_dtype():
    assert "sample_dtype" not in inspect.signature(SVMMulticlass.__init__).parameters
    with pytest.raises(TypeError):
        SVMMulticlass(_host_ctx(), sample_dtype=np.float32)
    assert SVMMulticlass(_host_ctx()).sample_dtype is np.float64
