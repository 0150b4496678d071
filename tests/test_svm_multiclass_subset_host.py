"""Subsets on SVMMulticlass without a GPU: the four new entries are declared in the header, listed in _lib.py, exported by the built library and named in
INTEGRATION.md; kfold's masks on labels of 3 and 5 classes whose sizes are no multiples of k; a mask of the wrong length is refused before anything reaches
the device."""
import os
import re
import types

import numpy as np
import pytest

from permon_amd import _lib
from permon_amd.svm import SVMMulticlass, kfold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["pmh_svm_multi_set_subset", "pmh_svm_multi_get_subset", "pmh_svm_multi_predict_own", "pmh_svm_multi_test_own"]


@pytest.mark.parametrize("name", ENTRIES)
def test_multiclass_subset_entries_are_declared_listed_and_exported(name):
    header = open(os.path.join(ROOT, "include", "permon_hip.h")).read()
    assert re.search(r"\bint %s\(pmh_svm_multi svm" % name, header), name + " is not declared in include/permon_hip.h"
    assert name in _lib.EXPORTED, name + " is not declared in permon_amd/_lib.py"
    assert hasattr(_lib.load(), name), name + " is not exported by libpermonhip.so"
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _labels(sizes, seed):
    """Class values 10 k - 7 with the given class sizes, shuffled."""
    y = np.concatenate([np.full(s, 10.0 * k - 7.0) for k, s in enumerate(sizes)])
    return np.random.default_rng(seed).permutation(y)


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("sizes", [(41, 33, 29), (23, 17, 13, 7, 2), (52, 1, 31), (11, 12, 13, 14, 1)])
def test_kfold_on_multiclass_labels(sizes, k):
    y = _labels(sizes, 5)
    assert any(s % k for s in sizes)
    masks = kfold(y, k, seed=1, stratified=True)
    assert len(masks) == k and all(m.dtype == bool and m.shape == y.shape for m in masks)
    # the complements partition the samples
    assert (sum((~m).astype(int) for m in masks) == 1).all()
    for c, size in zip(np.unique(y), sizes):
        share = [int(((~m) & (y == c)).sum()) for m in masks]
        assert sum(share) == size and max(share) - min(share) <= 1, (c, share)
        # a class of at least 2 samples is in every training mask (k >= 2: no fold holds all of it)
        if size >= 2:
            assert all((m & (y == c)).any() for m in masks), c
        else:
            assert sum(not (m & (y == c)).any() for m in masks) == 1


def _host_ctx():
    """What the constructor needs of a context: the library (its option entries run on the host) and a handle no test here reaches."""
    return types.SimpleNamespace(L=_lib.load(), h=None)


def test_a_mask_of_the_wrong_length_is_refused_on_the_host():
    m = SVMMulticlass(_host_ctx())
    with pytest.raises(RuntimeError):
        m.set_subset(np.ones(10))  # no handle yet
    m.h, m.n, m.K = object(), 10, 3  # (a handle that must not be reached)
    for bad in (np.ones(9), np.ones(11), np.ones((2, 10))):
        with pytest.raises(ValueError, match="10 entries"):
            m.set_subset(bad)
    with pytest.raises(ValueError, match="which"):
        m.test_own("no such selection")
    m.h = None
