"""The host-only parts of the grid search over C (permon_amd.svm.scores, select_C, the checks of the grid) and numpy's restatement of the warm start vector,
which the GPU tests compare the kernel against: hand-computed values throughout."""
import math

import numpy as np
import pytest

from permon_amd.svm import SCORES, _grid, scores, select_C
from svm_warm_cases import projected_gradient_norm, start_vector_np

NAN = float("nan")


def test_scores_by_hand():
    s = scores(dict(TP=3, FP=1, TN=4, FN=2))
    assert set(s) == set(SCORES)
    assert s["accuracy"] == 7 / 10 and s["precision"] == 3 / 4 and s["recall"] == 3 / 5 and s["specificity"] == 4 / 5
    assert s["f1"] == 6 / 9 and s["balanced_accuracy"] == (3 / 5 + 4 / 5) / 2
    assert s["mcc"] == (3 * 4 - 1 * 2) / math.sqrt(4 * 5 * 5 * 6)
    assert all(type(v) is float for v in s.values())
    # the dict of test / test_own carries an accuracy of its own, which is not read
    assert scores(dict(TP=3, FP=1, TN=4, FN=2, accuracy=-1.0)) == s


def test_scores_of_a_list_are_those_of_the_sum():
    parts = [dict(TP=1, FP=0, TN=3, FN=2), dict(TP=2, FP=1, TN=0, FN=0), dict(TP=0, FP=0, TN=1, FN=0)]
    assert scores(parts) == scores(dict(TP=3, FP=1, TN=4, FN=2))
    assert scores([parts[0]]) == scores(parts[0])


def test_scores_with_zero_denominators():
    s = scores(dict(TP=0, FP=0, TN=4, FN=0))  # nothing positive, nothing predicted positive
    assert s["accuracy"] == 1.0 and s["specificity"] == 1.0 and s["mcc"] == 0.0
    assert all(math.isnan(s[k]) for k in ("precision", "recall", "f1", "balanced_accuracy"))
    s = scores(dict(TP=0, FP=0, TN=0, FN=0))
    assert s["mcc"] == 0.0 and all(math.isnan(v) for k, v in s.items() if k != "mcc")
    s = scores(dict(TP=2, FP=3, TN=0, FN=0))  # everything predicted positive: no negative prediction, mcc's denominator is 0
    assert s["precision"] == 2 / 5 and s["recall"] == 1.0 and s["specificity"] == 0.0 and s["mcc"] == 0.0 and s["f1"] == 4 / 7
    s = scores(dict(TP=5, FP=0, TN=0, FN=0))
    assert s["accuracy"] == 1.0 and math.isnan(s["specificity"]) and s["mcc"] == 0.0


def test_select_C():
    assert select_C([1.0, 2.0, 4.0], [0.5, 0.9, 0.7]) == (2.0, 1)
    # a tie: the smallest C
    assert select_C([1.0, 2.0, 4.0], [0.5, 0.9, 0.9]) == (2.0, 1)
    assert select_C([1.0, 2.0, 4.0], [0.9, 0.9, 0.9]) == (1.0, 0)
    # a nan never wins, wherever it stands
    assert select_C([1.0, 2.0, 4.0], [NAN, 0.2, 0.1]) == (2.0, 1)
    assert select_C([1.0, 2.0, 4.0], [0.1, NAN, 0.1]) == (1.0, 0)
    assert select_C([1.0, 2.0], [NAN, -1.0]) == (2.0, 1)
    with pytest.raises(ValueError):
        select_C([1.0, 2.0], [NAN, NAN])
    # Cs in any order: the tie still goes to the smallest C, the index is the one in Cs as given
    assert select_C([4.0, 1.0, 2.0], [0.9, 0.5, 0.9]) == (2.0, 2)
    assert select_C([4.0, 2.0, 1.0], [0.9, 0.9, 0.9]) == (1.0, 2)
    assert select_C([4.0, 2.0, 1.0], [0.9, 0.9, NAN]) == (2.0, 1)


def test_grid_is_sorted_and_checked():
    assert _grid([4, 0.25, 1], "accuracy") == [0.25, 1.0, 4.0]
    assert _grid(np.array([2.0]), "mcc") == [2.0]
    for bad in ([], [1.0, 0.0], [1.0, -2.0], [1.0, float("inf")], [NAN, 1.0]):
        with pytest.raises(ValueError):
            _grid(bad, "accuracy")
    with pytest.raises(ValueError):
        _grid([1.0], "auc")


def test_start_vector_restatement_by_hand():
    a = np.array([0.0, 0.5, 1.0, 2.0, 0.25, 0.0])
    m = np.array([True, True, True, True, False, False])
    ub = np.array([1.0, 1.0, 1.5, 3.0, 1.0, 1.0])
    v, masked, clipped = start_vector_np(a, 2.0, m, ub)
    assert v.tolist() == [0.0, 1.0, 1.5, 3.0, 0.0, 0.0] and (masked, clipped) == (1, 2)  # (1.0 is AT its bound, not clipped; 2.0 -> 1.5 and 4.0 -> 3.0 are)
    v, masked, clipped = start_vector_np(a, 2.0, None, None)
    assert v.tolist() == [0.0, 1.0, 2.0, 4.0, 0.5, 0.0] and (masked, clipped) == (0, 0)
    v, masked, clipped = start_vector_np(np.array([-1.0, 3.0]), 0.5, None, np.array([1.0, 1.0]))
    assert v.tolist() == [0.0, 1.0] and (masked, clipped) == (0, 1)


def test_projected_gradient_by_hand():
    H = np.diag([1.0, 2.0, 4.0])
    rhs = np.ones(3)
    # the minimiser over 0 <= a <= 0.3: (0.3, 0.3, 0.25) -- the first two at the bound with g < 0, the third free with g = 0
    assert projected_gradient_norm(H, rhs, np.array([0.3, 0.3, 0.25]), np.full(3, 0.3)) == 0.0
    # at the lower bound g = -1 points into the box: it counts; at the upper bound a g > 0 would
    assert projected_gradient_norm(H, rhs, np.zeros(3), np.full(3, 0.3)) == math.sqrt(3.0)
    assert projected_gradient_norm(H, rhs, np.array([2.0, 0.5, 0.25]), np.array([2.0, 1.0, 1.0])) == 1.0
    assert projected_gradient_norm(H, rhs, np.array([2.0, 0.5, 0.25]), None) == 1.0
