"""The SVM and SVR front ends compute, bit for bit, what tests/golden/svm_front_bits.json recorded: SVR trainings (dense fp64 and float32, CSR; both losses, with
and without sample weights and bias), its scores and metrics, set_epsilon / set_penalties / a second training on one handle; SVM on CSR samples and with
per-sample upper bounds; scores, labels, counts, test_own, probabilities and the Platt fit; warm starts.  The other SVM and SVR tests compare with numpy inside
rounding bounds and would pass a reassociated sum.  The cases and how they are recorded: tests/golden/make_svm_front_bits.py, which this test runs again."""
import importlib.util
import json
import os

import numpy as np
import pytest

from test_gpu_svm_sparse import _zero_rows
from test_gpu_svm_subset import train_mask

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_svm_front_bits_equal_the_recorded_ones():
    spec = importlib.util.spec_from_file_location("make_svm_front_bits", os.path.join(GOLDEN, "make_svm_front_bits.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for n in [s[0] for s in gen.SHAPES] + [gen.CSR[0]]:  # (the generator's copy of the held-out set is the subset tests')
        assert np.array_equal(gen.train_mask(n), train_mask(n))
    import scipy.sparse as sp

    X = sp.random(50, 20, 0.3, random_state=1, format="csr")  # (and its copy of the row emptying is the sparse tests')
    assert (gen.zero_rows(X, 0.2, 3) != _zero_rows(X, 0.2, 3)).nnz == 0
    with open(gen.JSON) as f:
        rec = json.load(f)
    got = json.loads(json.dumps(gen.compute()))  # (tuples and ints as JSON holds them)
    want = rec["cases"]
    assert sorted(got) == sorted(want)
    bad = [k for k in sorted(want) if got[k] != want[k]]
    for k in bad:
        print(k, "recorded", want[k], "now", got[k])
    assert not bad, ("%d of %d entries differ from the bits recorded at %s with %s; if the toolchain or the intended arithmetic changed, record them again with "
                     "tests/golden/make_svm_front_bits.py: %s" % (len(bad), len(want), rec["meta"]["commit"][:12], rec["meta"]["hipcc"], bad[:8]))
