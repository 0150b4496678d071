"""What tests/test_svm_grid_host.py and tests/test_gpu_svm_warm.py share (no test in here): numpy's restatement of the warm start vector, the solver's stopping
quantity recomputed on the host, the instances of the grid search and the loop grid_search stands for, written by hand over the existing API."""
import numpy as np

from permon_amd import problems as P
from permon_amd.svm import kfold
from svm_train_cases import ASTOL

GRID_CS = [2.0 ** e for e in (-4, 0, 4)]
GRID_K = 3


def start_vector_np(alpha, scale, m, ub):
    """a0_i = m_i ? min(max(scale alpha_i, 0), ub_i) : 0 -- one multiplication, then max, then min -- with the two counts: entries the mask zeroed that were
    not zero, entries clipped at ub.  m: booleans or None (all ones); ub: the bounds or None (no upper bound)."""
    m = np.ones(alpha.size, dtype=bool) if m is None else np.asarray(m, dtype=bool)
    v = np.maximum(scale * alpha, 0.0)
    clipped = np.zeros(alpha.size, dtype=bool)
    if ub is not None:
        clipped = m & (v > ub)
        v = np.minimum(v, ub)
    return np.where(m, v, 0.0), int((~m & (alpha != 0.0)).sum()), int(clipped.sum())


def dual_hessian(X, y, diag=None):
    """H = diag(y) X X' diag(y) (+ diag) as a dense matrix; X an ndarray or a scipy.sparse matrix."""
    Z = X.toarray() if hasattr(X, "toarray") else np.asarray(X, dtype=np.float64)
    Z = y[:, None] * Z
    H = Z @ Z.T
    if diag is not None:
        H[np.diag_indices_from(H)] += diag
    return H


def projected_gradient_norm(H, rhs, a, ub):
    """MPGP's stopping quantity |gP| at a for min 1/2 a'Ha - rhs'a over 0 <= a <= ub (ub None: no upper bound): g = Ha - rhs; where a_i is at a bound (within
    astol, the lower bound asked first) the part of g_i that points into the box, min(g_i, 0) at 0 and max(g_i, 0) at ub_i; g_i elsewhere."""
    g = H @ a - rhs
    at_lb = np.abs(a) <= ASTOL
    at_ub = ~at_lb & (np.abs(a - ub) <= ASTOL) if ub is not None else np.zeros(a.size, dtype=bool)
    gP = np.where(at_lb, np.minimum(g, 0.0), np.where(at_ub, np.maximum(g, 0.0), g))
    return float(np.linalg.norm(gP))


_GRID = {}


def grid_data(kind):
    """"dense": 240 x 8, two overlapping blobs (svm_blobs with K = 2, separation 1: the classes' centres are sqrt(2) apart under unit noise), labels -1 / +1;
    "csr": svm_sparse 300 x 200 with 12 entries per row.  -> (X, y), drawn once."""
    if kind not in _GRID:
        if kind == "dense":
            p = P.svm_blobs(240, 8, 2, 1.0, 1)
            _GRID[kind] = (p["X"], 2.0 * p["labels"] - 1.0)
        else:
            p = P.svm_sparse(300, 200, 12, 1.2, 0.5, 1.0)
            _GRID[kind] = (p["X"], p["y"])
    return _GRID[kind]


def hand_grid(svm, y, Cs, k, ratio_pos=1.0, ratio_neg=1.0, sample_weight=None):
    """counts[g][f] of the loop over the existing entries alone: for every fold set_subset, for every C ascending set_penalties, train, test_own."""
    Cs = sorted(Cs)
    masks = kfold(y, k, 0, True)
    counts = [[None] * k for _ in Cs]
    for f, m in enumerate(masks):
        svm.set_subset(m)
        for g, C in enumerate(Cs):
            svm.set_penalties(C * ratio_pos, C * ratio_neg, sample_weight)
            counts[g][f] = svm.train().test_own("held_out")
    return counts
