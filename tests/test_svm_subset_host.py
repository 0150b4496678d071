"""Sample subsets without a GPU: the new entries are declared in the header, listed in _lib.py and exported by the built library; pmh_svm_opts keeps its six
fields; the PMH_SVM_OWN_* selectors have the values svm.py uses; kfold's masks."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from permon_amd.svm import SVM, kfold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["pmh_op_svm_dual_set_subset", "pmh_svm_set_subset", "pmh_svm_get_subset", "pmh_svm_predict_own", "pmh_svm_test_own"]


@pytest.mark.parametrize("name", ENTRIES)
def test_subset_entries_are_declared_listed_and_exported(name):
    from permon_amd import _lib

    header = open(os.path.join(ROOT, "include", "permon_hip.h")).read()
    assert re.search(r"\bint %s\(" % name, header), name + " is not declared in include/permon_hip.h"
    assert name in _lib.EXPORTED, name + " is not declared in permon_amd/_lib.py"
    assert hasattr(_lib.load(), name), name + " is not exported by libpermonhip.so"
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_svm_opts_fields_are_unchanged():
    from permon_amd import _lib

    assert [name for name, _ in _lib.SvmOpts._fields_] == ["loss_type", "C", "bias", "qps", "mpgp", "smalxe"]
    body = re.search(r"typedef struct \{([^}]*)\} pmh_svm_opts;", open(os.path.join(ROOT, "include", "permon_hip.h")).read()).group(1)
    assert re.findall(r"(\w+);", body) == ["loss_type", "C", "bias", "qps", "mpgp", "smalxe"]


def test_own_selectors_match_the_header():
    src = '#include <stdio.h>\n#include "permon_hip.h"\nint main(void){ printf("%d %d %d", PMH_SVM_OWN_HELD_OUT, PMH_SVM_OWN_SUBSET, PMH_SVM_OWN_ALL); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = list(map(int, subprocess.check_output([exe]).split()))
    assert got == [SVM.OWN["held_out"], SVM.OWN["subset"], SVM.OWN["all"]]


def _labels(n, seed, rare=0):
    y = np.where(np.random.default_rng(seed).random(n) < 0.3, 1.0, -1.0)
    y[:rare] = 2.0  # a third class of `rare` samples
    return y


@pytest.mark.parametrize("stratified", [True, False])
@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("n,rare", [(103, 0), (103, 3), (1000, 1)])
def test_kfold(n, rare, k, stratified):
    y = _labels(n, 4, rare)
    masks = kfold(y, k, seed=3, stratified=stratified)
    assert len(masks) == k and all(m.dtype == bool and m.shape == (n,) for m in masks)
    # the complements partition range(n), in folds whose sizes differ by at most one
    assert (sum((~m).astype(int) for m in masks) == 1).all()
    sizes = [int((~m).sum()) for m in masks]
    assert max(sizes) - min(sizes) <= 1
    if stratified:
        for c in np.unique(y):
            share = [int(((~m) & (y == c)).sum()) for m in masks]
            assert max(share) - min(share) <= 1, (c, share)
            assert sum(share) == int((y == c).sum())
    # the same seed gives the same masks, another seed other ones
    again = kfold(y, k, seed=3, stratified=stratified)
    assert all(np.array_equal(a, b) for a, b in zip(masks, again))
    other = kfold(y, k, seed=4, stratified=stratified)
    assert any(not np.array_equal(a, b) for a, b in zip(masks, other))


def test_kfold_refuses_a_bad_k():
    with pytest.raises(ValueError):
        kfold(np.ones(10), 1)
    with pytest.raises(ValueError):
        kfold(np.ones(3), 5)
