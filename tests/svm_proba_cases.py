"""Inputs and references shared by tests/test_gpu_svm_proba.py and tests/test_svm_proba_host.py (no test in here): a numpy restatement of the Platt fit of
csrc/svm_proba.hip (Lin, Lin and Weng, 2007: the same formulas, constants and control flow; numpy's summation order), the score generator of the fit's
instances, the models and samples of the predict_proba tests."""
import numpy as np

EPS = 2.0 ** -52
CONVERGED, MAX_IT, LINE_SEARCH = 1, 2, 3  # PMH_PLATT_*
# (n, frac, seed): one wavefront; one workgroup and a ragged tail; several workgroups; unbalanced.  Checked on the CPU: the restatement's iterations and the
# smallest eigenvalue of the final Hessian (rounded down), the strong-convexity modulus the GPU comparison rests on
INSTANCES = [(64, 0.3, 3), (257, 0.5, 1), (1000, 0.5, 0), (2000, 0.1, 2)]
ITERATIONS = {(64, 0.3, 3): 4, (257, 0.5, 1): 5, (1000, 0.5, 0): 5, (2000, 0.1, 2): 5}
LAMBDA_MIN = {(64, 0.3, 3): 9.9, (257, 0.5, 1): 43.8, (1000, 0.5, 0): 174.0, (2000, 0.1, 2): 102.0}


def scores(n, frac, seed):
    """Overlapping scores: y = +-1 with P(+1) = frac, f = y + 1.5 N(0,1)."""
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(n) < frac, 1.0, -1.0)
    f = 1.0 * y + 1.5 * rng.standard_normal(n)
    return f, y


def separable_scores(n=200, seed=4):
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    return y * (1.0 + np.abs(rng.standard_normal(n))), y


def sigma(z):
    """1 / (1 + e^z) in the two branches the kernels use."""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0.0, e / (1.0 + e), 1.0 / (1.0 + e))


def targets(y):
    n_pos, n_neg = int((y > 0).sum()), int((y <= 0).sum())
    return np.where(y > 0, (n_pos + 1.0) / (n_pos + 2.0), 1.0 / (n_neg + 2.0)), n_pos, n_neg


def sums(f, t, A, B):
    """(F, g1, g2, h11, h22, h21) at (A, B)."""
    z = A * f + B
    e = np.exp(-np.abs(z))
    p = np.where(z >= 0.0, e / (1.0 + e), 1.0 / (1.0 + e))
    F = np.where(z >= 0.0, t * z, (t - 1.0) * z) + np.log1p(e)
    q, r = p * (1.0 - p), t - p
    return np.array([F.sum(), (f * r).sum(), r.sum(), (f * f * q).sum(), q.sum(), (f * q).sum()])


def platt_np(f, y):
    """The fit: dict(A, B, reason, iterations, evaluations, fval, g1, g2, lambda_min)."""
    t, n_pos, n_neg = targets(y)
    A, B = 0.0, np.log((n_neg + 1.0) / (n_pos + 1.0))
    h = sums(f, t, A, B)
    ev, reason, it = 1, MAX_IT, 0
    with np.errstate(all="ignore"):
        while it < 100:
            g1, g2, h11, h22, h21 = h[1], h[2], h[3] + 1e-12, h[4] + 1e-12, h[5]
            if abs(g1) < 1e-5 and abs(g2) < 1e-5:
                reason = CONVERGED
                break
            det = h11 * h22 - h21 * h21
            dA, dB = -(h22 * g1 - h21 * g2) / det, -(-h21 * g1 + h11 * g2) / det
            gd = g1 * dA + g2 * dB
            step = 1.0
            while step >= 1e-10:
                hn = sums(f, t, A + step * dA, B + step * dB)
                ev += 1
                if hn[0] < h[0] + 1e-4 * step * gd:
                    A, B, h = A + step * dA, B + step * dB, hn
                    break
                step /= 2.0
            if step < 1e-10:
                reason = LINE_SEARCH
                break
            it += 1
    lam = float(np.linalg.eigvalsh(np.array([[h[3], h[5]], [h[5], h[4]]]))[0])
    return dict(A=float(A), B=float(B), reason=reason, iterations=it, evaluations=ev, fval=float(h[0]), g1=float(h[1]), g2=float(h[2]), lambda_min=lam, n_pos=n_pos, n_neg=n_neg)


# ---- predict_proba: samples with two labellings (the generator of the multiclass tests' re-labelling cases, restated) -----------------------------------------
SHAPES = [(300, 64), (257, 37), (130, 130), "csr"]


def samples(shape):
    """(X, y): dense (n, d), or the CSR case 400 x 3000 with 12 entries per sample and one sample without entries."""
    import scipy.sparse as sp

    from permon_amd import problems as P

    if shape == "csr":
        p = P.svm_sparse(400, 3000, 12, 1.0, 0.5)
        keep = np.ones(400)
        keep[123] = 0.0
        X = (sp.diags(keep) @ p["X"]).tocsr()
        X.eliminate_zeros()
        X.sort_indices()
        assert X.indptr[124] == X.indptr[123]
        return X, p["y"]
    p = P.svm_offset(*shape)
    return p["X"], p["y"]


# ---- multiclass: overlapping blobs, so that no class is separable from the rest ------------------------------------------------------------------------------
MULTI = [(3, 64, None), (5, 64, None), (3, 37, None), (5, 37, None), (3, 300, 10), (5, 300, 10)]  # (K, d, sparse)
MULTI_N = 150


def multi_case(K, d, sparse):
    """(X (ndarray or CSR), labels, W, b): blobs with separation 1.5 against unit noise and the model W_k = e_k - mean, b = -0.4: scores that overlap."""
    from permon_amd import problems as P

    p = P.svm_blobs(MULTI_N, d, K, 1.5, 7, sparse=sparse)
    W = np.zeros((K, d))
    W[np.arange(K), np.arange(K)] = 1.0
    W[:, :K] -= 1.0 / K
    W += 0.01 * np.random.default_rng(K + d).standard_normal((K, d))
    b = np.full(K, -0.4) + 0.05 * np.arange(K)
    return (p["X_csr"] if sparse else p["X"]), p["labels"], W, b
