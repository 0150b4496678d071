"""Helpers shared by tests/test_gpu_svm.py, test_gpu_svm_train.py, test_gpu_svm_sparse.py and test_gpu_svm_penalties.py (no test in here): the rounding bound
of a dot product, the plain MPGP solve of an SVM dual, the oracle's biased training, numpy's model of a dual solution and the check of the confusion counts."""
import numpy as np

import permon_amd as pa

EPS = np.finfo(float).eps
ASTOL = 10 * EPS  # qpc.c:28


def gamma(k):
    """Higham's gamma_k = k eps / (1 - k eps): |fl(sum of k products) - exact| <= gamma_k sum |a_i v_i| for ANY order of summation of a k-term fp64 dot product."""
    return k * EPS / (1.0 - k * EPS)


def solve(ctx, p, rtol=1e-6, distributed=False):
    H = pa.MatCreateSVMDual(ctx, p["X"], p["y"])
    qp = pa.QP(ctx)
    qp.SetOperator(H)
    qp.SetRhs(ctx.vec_from(p["b"]))
    x = ctx.vec_from(p["x0"])
    qp.SetInitialVector(x)
    qp.SetBox(None, ctx.vec_from(p["lb"]), ctx.vec_from(p["ub"]))
    qps = pa.QPS(ctx)
    qps.SetQP(qp)
    qps.SetType("mpgp")
    qps.SetTolerances(rtol=rtol)
    qps.MPGPSetDistributed(distributed)
    st = qps.Solve()
    return H, st, x.to_numpy()


def oracle_train(oracle, p, loss):
    X, y, n = p["X"], p["y"], p["n"]
    Xt = X.T.tocsr() if hasattr(X, "tocsr") else X.T  # (dense samples: X.T as it is)
    sh = 0.0 if loss == "L1" else 1.0 / p["C"]
    op = oracle.Op(n, fn=lambda a: y * (X @ (Xt @ (y * a))) + sh * a)
    pf = oracle.Qppf(oracle.Csr(1, n, [0, n], np.arange(n), y / np.sqrt(n)), orthonormal=True)
    box = oracle.Box(n, lb=p["lb"], ub=p["ub"] if loss == "L1" else None)
    return oracle.smalxe(op, p["b"], p["x0"], box, pf, rtol=1e-6, max_it=100)


def np_model(p, a, loss, Ci=None):
    """w, b and the free support vectors of the dual solution a: free means astol < a_i and, for L1, a_i < C_i - astol (Ci: the bound of every sample; None: C)."""
    X, y = p["X"], p["y"]
    w = X.T @ (y * a)
    free = (a > ASTOL) & ((a < (p["C"] if Ci is None else Ci) - ASTOL) if loss == "L1" else True)
    return w, float(np.mean(y[free] - X[free] @ w)), free


def check_counts(t, sc_np, yt, sure):
    """The four counts against numpy's on the samples whose label the score decides beyond rounding: each library count lies between numpy's count on those samples
    and that plus the number left out (equality where none is left out)."""
    l_np = np.where(sc_np >= 0, 1.0, -1.0)
    out = int((~sure).sum())
    ref = dict(TP=(l_np > 0) & (yt > 0), FP=(l_np > 0) & (yt < 0), TN=(l_np < 0) & (yt < 0), FN=(l_np < 0) & (yt > 0))
    assert t["TP"] + t["FP"] + t["TN"] + t["FN"] == yt.size
    for k, m in ref.items():
        c = int((m & sure).sum())
        assert c <= t[k] <= c + out, (k, t[k], c, out)
