"""The dense SVM path computes, bit for bit, what tests/golden/svm_dense_bits.json recorded: the operator's products in every form with and without a sample
subset, fixed runs of MPGP on the paired and on the separate passes (iterate, step string, pass count) and trainings with and without bias (alpha, w, b, every
statistic).  The other SVM tests compare with numpy inside rounding bounds and one GPU path with another; neither sees a change that reassociates a sum on both
paths.  The cases and how they are recorded: tests/golden/make_svm_dense_bits.py, which this test runs again."""
import importlib.util
import json
import os

import numpy as np
import pytest

from test_gpu_svm_subset import train_mask

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_dense_svm_bits_equal_the_recorded_ones():
    spec = importlib.util.spec_from_file_location("make_svm_dense_bits", os.path.join(GOLDEN, "make_svm_dense_bits.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for n, _, _ in gen.SHAPES:  # (the generator's copy of the held-out set is the subset tests')
        assert np.array_equal(gen.train_mask(n), train_mask(n))
    with open(gen.JSON) as f:
        rec = json.load(f)
    got = json.loads(json.dumps(gen.compute()))  # (tuples and ints as JSON holds them)
    want = rec["cases"]
    assert rec["meta"]["mpgp_iters"] == gen.MPGP_ITERS
    assert sorted(got) == sorted(want)
    bad = [k for k in sorted(want) if got[k] != want[k]]
    for k in bad:
        print(k, "recorded", want[k], "now", got[k])
    assert not bad, ("%d of %d entries differ from the bits recorded at %s with %s; if the toolchain or the intended arithmetic changed, record them again with "
                     "tests/golden/make_svm_dense_bits.py: %s" % (len(bad), len(want), rec["meta"]["commit"][:12], rec["meta"]["hipcc"], bad[:8]))
