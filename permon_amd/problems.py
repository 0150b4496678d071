"""Synthetic QP generators for the PERMON QPS hot path (numpy, host side).

Each generator restates the *problem definition* of one of the reference's tutorials (cited per
function; paths relative to /root/reference) or one of BASELINE.json's configs, and returns plain
CSR arrays (int32 indices, fp64 values) + vectors.  No solver code lives here.
"""
import numpy as np

__all__ = ["ex1", "ex2", "ex3_primal", "jbearing2", "laplace2d_box", "laplace2d_csr", "svm_dual", "svm_sparse"]


def _fobst(i, n):
    # src/tutorials/ex1.c:42-46
    h = 1.0 / (n - 1)
    return np.sin(4 * np.pi * i * h - np.pi / 6.0) / 2 - 2


def _tridiag_dirichlet(n):
    """CSR of ex1's Hessian: tridiag(-1,2,-1) with identity first/last rows and the couplings to
    them dropped (src/tutorials/ex1.c:74-100)."""
    rowptr = np.zeros(n + 1, dtype=np.int32)
    col, val = [], []
    for i in range(n):
        if i == 0 or i == n - 1:
            col.append(i)
            val.append(1.0)
        else:
            if i != 1:
                col.append(i - 1)
                val.append(-1.0)
            col.append(i)
            val.append(2.0)
            if i != n - 2:
                col.append(i + 1)
                val.append(-1.0)
        rowptr[i + 1] = len(col)
    return rowptr, np.asarray(col, dtype=np.int32), np.asarray(val, dtype=np.float64)


def ex1(n=100):
    """String-contact QP of src/tutorials/ex1.c:58-157: min 1/2 x'Ax - x'b s.t. x >= c.

    Returns dict(n, rowptr, col, val, b, lb, x0).  b_i = -15 h^2 * 2 (ex1.c:98), lb_i = fobst(i) for
    interior i and 0 at both ends (vector c is zero-initialised, ex1.c:71,99), x0 = 0.
    """
    h = 1.0 / (n - 1)
    rowptr, col, val = _tridiag_dirichlet(n)
    b = np.full(n, -15 * h * h * 2)
    b[0] = b[-1] = 0.0
    i = np.arange(n)
    lb = _fobst(i, n)
    lb[0] = lb[-1] = 0.0
    return dict(n=n, rowptr=rowptr, col=col, val=val, b=b, lb=lb, ub=None, x0=np.zeros(n))


def ex2(n=100, infinite=False):
    """src/tutorials/ex2.c:32-140: as ex1 but the bound acts on the first half of the unknowns only,
    either through an index set (is = [0, n/2), lb of length n/2) or through -inf bounds."""
    p = ex1(n)
    i = np.arange(n)
    if infinite:
        lb = np.where(i < n // 2, _fobst(i, n), -np.inf)
        lb[0] = 0.0
        lb[-1] = 0.0  # rows 0 and n-1 are never set (ex2.c:88-103) -> 0
        p.update(lb=lb, is_=None)
    else:
        lb = _fobst(np.arange(n // 2), n)
        lb[0] = 0.0
        p.update(lb=lb, is_=np.arange(n // 2, dtype=np.int32))
    return p


def ex3_primal(n=100):
    """src/tutorials/ex3.c:32-150: ex1's QP with the bound written as the inequality -I x <= -c
    (B = -I, cI = -c, ex3.c:118-120).  Returned in primal form; dualisation is the caller's job
    (QPTDualize, src/qp/interface/qptransform.c:909-1197)."""
    p = ex1(n)
    c = p.pop("lb")
    p.update(BI_diag=-np.ones(n), cI=-c)
    return p


def jbearing2(nx, ny, ecc=0.1, b=10.0):
    """Journal-bearing QP (MINPACK-2 DPJB) of src/tutorials/jbearing2.c: Hessian FormHessian :349-482,
    linear term ComputeB :191-232, QP set-up :511-514 (QPSetRhsPlus => rhs = -B), bounds 0 <= x <= 1000
    (:151-152), x0 = 0.  Natural ordering row = j*nx + i (single-rank DMDA)."""
    hx = 2.0 * (4.0 * np.arctan(1.0)) / (nx + 1.0)
    hy = 2.0 * b / (ny + 1.0)
    hxhy = hx * hy
    hxhx = 1.0 / (hx * hx)
    hyhy = 1.0 / (hy * hy)

    def p(xi):
        t = 1.0 + ecc * np.cos(xi)
        return t * t * t

    n = nx * ny
    rowptr = np.zeros(n + 1, dtype=np.int32)
    col, val = [], []
    six = 6.0
    rows = {}
    for i in range(nx):
        xi = (i + 1) * hx
        trule1 = hxhy * (p(xi) + p(xi + hx) + p(xi)) / six
        trule2 = hxhy * (p(xi) + p(xi - hx) + p(xi)) / six
        trule3 = hxhy * (p(xi) + p(xi + hx) + p(xi + hx)) / six
        trule4 = hxhy * (p(xi) + p(xi - hx) + p(xi - hx)) / six
        trule5 = trule1
        trule6 = trule2
        vdown = -(trule5 + trule2) * hyhy
        vleft = -hxhx * (trule2 + trule4)
        vright = -hxhx * (trule1 + trule3)
        vup = -hyhy * (trule1 + trule6)
        vmiddle = hxhx * (trule1 + trule2 + trule3 + trule4) + hyhy * (trule1 + trule2 + trule5 + trule6)
        for j in range(ny):
            row = j * nx + i
            c, v = [], []
            if j > 0:
                c.append(row - nx)
                v.append(vdown)
            if i > 0:
                c.append(row - 1)
                v.append(vleft)
            c.append(row)
            v.append(vmiddle)
            if i + 1 < nx:
                c.append(row + 1)
                v.append(vright)
            if j + 1 < ny:
                c.append(row + nx)
                v.append(vup)
            rows[row] = (c, v)
    for r in range(n):
        c, v = rows[r]
        col.extend(c)
        val.extend(v)
        rowptr[r + 1] = len(col)
    ehxhy = ecc * hx * hy
    B = np.empty(n)
    for i in range(nx):
        temp = np.sin((i + 1) * hx)
        for j in range(ny):
            B[nx * j + i] = -ehxhy * temp
    return dict(n=n, rowptr=rowptr, col=np.asarray(col, dtype=np.int32), val=np.asarray(val, dtype=np.float64), b=-B,
                lb=np.zeros(n), ub=np.full(n, 1000.0), x0=np.zeros(n))


def laplace2d_csr(nx, ny):
    """5-point Laplacian (4 on the diagonal, -1 off) on an nx x ny interior grid with homogeneous
    Dirichlet boundary eliminated (SPD).  Row r = j*nx + i; columns ascending.  Vectorised: fits the
    10 M-row config of BASELINE.json configs[1] (nx = ny = 3162 -> n = 9 998 244, nnz = 49 978 572)."""
    n = nx * ny
    r = np.arange(n, dtype=np.int64)
    i = r % nx
    j = r // nx
    has = [j > 0, i > 0, np.ones(n, dtype=bool), i < nx - 1, j < ny - 1]
    offs = [-nx, -1, 0, 1, nx]
    vals = [-1.0, -1.0, 4.0, -1.0, -1.0]
    cnt = np.zeros(n, dtype=np.int64)
    for h in has:
        cnt += h
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(cnt, out=rowptr[1:])
    nnz = int(rowptr[-1])
    col = np.empty(nnz, dtype=np.int32)
    val = np.empty(nnz, dtype=np.float64)
    pos = rowptr[:-1].copy()
    for h, o, v in zip(has, offs, vals):
        idx = pos[h]
        col[idx] = (r[h] + o).astype(np.int32)
        val[idx] = v
        pos[h] += 1
    return rowptr.astype(np.int32), col, val


def laplace2d_box(nx, ny, variant="obstacle", seed=20260515):
    """BASELINE.json configs[1]: synthetic SPD 5-pt Laplacian QP with box constraints.

    variant "obstacle": b = -15 h^2 * 2 (ex1's load scaled the same way), lb = sin(4 pi x - pi/6) *
    sin(4 pi y - pi/6)/2 - 2 (2-D analogue of ex1's obstacle), ub = +inf (None).
    variant "twosided": lb = -1, ub = +1, b standard normal (numpy default_rng(seed)) - exercises both bounds.
    """
    n = nx * ny
    rowptr, col, val = laplace2d_csr(nx, ny)
    hx, hy = 1.0 / (nx + 1), 1.0 / (ny + 1)
    r = np.arange(n, dtype=np.int64)
    x = ((r % nx) + 1) * hx
    y = ((r // nx) + 1) * hy
    if variant == "obstacle":
        b = np.full(n, -15.0 * hx * hy * 2)
        lb = np.sin(4 * np.pi * x - np.pi / 6.0) * np.sin(4 * np.pi * y - np.pi / 6.0) / 2 - 2
        ub = None
    elif variant == "twosided":
        rng = np.random.default_rng(seed)
        b = rng.standard_normal(n)
        lb = np.full(n, -1.0)
        ub = np.full(n, 1.0)
    else:
        raise ValueError(variant)
    return dict(n=n, rowptr=rowptr, col=col, val=val, b=b, lb=lb, ub=ub, x0=np.zeros(n))


def svm_dual(N, d=64, C=1.0, seed_x=7, seed_w=8):
    """BASELINE.json configs[4]: PermonSVM-style hinge-loss dual without bias term,
    min 1/2 a'Ha - 1'a, 0 <= a <= C, H = diag(y) X X' diag(y) applied matrix-free.
    X in R^{N x d} i.i.d. N(0,1) (default_rng(seed_x)), w* ~ N(0,1) (default_rng(seed_w)), y = sign(X w* + 0.1 N(0,1))."""
    rng = np.random.default_rng(seed_x)
    X = rng.standard_normal((N, d))
    w = np.random.default_rng(seed_w).standard_normal(d)
    y = np.sign(X @ w + 0.1 * rng.standard_normal(N))
    y[y == 0] = 1.0
    return dict(n=N, d=d, X=X, y=y, b=np.ones(N), lb=np.zeros(N), ub=np.full(N, float(C)), x0=np.zeros(N))


def svm_offset(N, d=64, offset=3.0, C=1.0, seed_x=7, seed_w=8, seed_test=None, N_test=0):
    """The data of svm_dual with an offset planted in the labels, y = sign(X w* + offset + 0.1 N(0,1)): a separating plane that does not pass through the
    origin, so a classifier needs the bias term.  Same draws as svm_dual (X, then the noise, from default_rng(seed_x); w* from default_rng(seed_w)).
    N_test > 0: a held-out draw (X_test, y_test) of the same model from default_rng(seed_test or seed_x + 1000)."""
    rng = np.random.default_rng(seed_x)
    X = rng.standard_normal((N, d))
    w = np.random.default_rng(seed_w).standard_normal(d)
    y = np.sign(X @ w + offset + 0.1 * rng.standard_normal(N))
    y[y == 0] = 1.0
    out = dict(n=N, d=d, X=X, y=y, C=float(C), offset=float(offset), w_star=w, b=np.ones(N), lb=np.zeros(N), ub=np.full(N, float(C)), x0=np.zeros(N))
    if N_test > 0:
        rt = np.random.default_rng(seed_x + 1000 if seed_test is None else seed_test)
        Xt = rt.standard_normal((N_test, d))
        yt = np.sign(Xt @ w + offset + 0.1 * rt.standard_normal(N_test))
        yt[yt == 0] = 1.0
        out.update(X_test=Xt, y_test=yt)
    return out


def svm_sparse(N, d, nnz_row, skew, offset, C=1.0, seed=7, N_test=0):
    """Sparse, wide samples with skewed feature popularity (text / click data): per sample nnz_row feature draws with probability proportional to
    1 / rank^skew, values N(0,1), duplicates summed, rows scaled to unit length (default_rng(seed)); w* ~ N(0,1) from default_rng(seed + 1);
    y = sign(X w* + offset + 0.1 N(0,1)).  N_test > 0: a held-out draw from default_rng(seed + 1000).  The keys of svm_offset, X (and X_test) scipy CSR."""
    import scipy.sparse as sp

    p = 1.0 / np.arange(1, d + 1) ** skew
    p /= p.sum()

    def draw(r, n):
        cols = r.choice(d, size=(n, nnz_row), p=p)
        vals = r.standard_normal((n, nnz_row))
        X = sp.csr_matrix((vals.ravel(), (np.repeat(np.arange(n), nnz_row), cols.ravel())), shape=(n, d))
        X.sum_duplicates()
        X.sort_indices()
        nr = np.sqrt(np.asarray(X.multiply(X).sum(axis=1)).ravel())
        nr[nr == 0] = 1.0
        X = (sp.diags(1.0 / nr) @ X).tocsr()
        X.sort_indices()  # (the product does not promise them sorted; the values are the same either way)
        return X

    rng = np.random.default_rng(seed)
    X = draw(rng, N)
    w = np.random.default_rng(seed + 1).standard_normal(d)
    y = np.sign(X @ w + offset + 0.1 * rng.standard_normal(N))
    y[y == 0] = 1.0
    out = dict(n=N, d=d, X=X, y=y, C=float(C), offset=float(offset), w_star=w, b=np.ones(N), lb=np.zeros(N), ub=np.full(N, float(C)), x0=np.zeros(N))
    if N_test > 0:
        rt = np.random.default_rng(seed + 1000)
        Xt = draw(rt, N_test)
        yt = np.sign(Xt @ w + offset + 0.1 * rt.standard_normal(N_test))
        yt[yt == 0] = 1.0
        out.update(X_test=Xt, y_test=yt)
    return out


def svr_linear(n, d, noise, seed, sparse=None, b_true=3.0, eps=0.1, C=1.0, n_test=0):
    """Linear regression data for SVR: t = X w* + b* + noise N(0,1), w* ~ N(0,1) / sqrt(d) so that the targets' spread does not grow with d.
    sparse=None: X i.i.d. N(0,1), dense.  sparse=(nnz_row, skew): X scipy CSR drawn in the style of svm_sparse -- nnz_row feature draws per sample with
    probability proportional to 1 / rank^skew, values N(0,1), duplicates summed, rows scaled to unit length.  X, then the noise, from default_rng(seed); w* from
    default_rng(seed + 1).  Returns dict(n, d, X, t, w_true, b_true, eps, C) and, for the QP-level tests on MatCreateSVRDual, the vectors of the dual in
    u = [p; q]: c = [t - eps; -t - eps], lb = 0, ub = C (the L1 box), x0 = 0.  n_test > 0: a held-out draw (X_test, t_test) from default_rng(seed + 1000)."""
    import scipy.sparse as sp

    def draw(r, m):
        if sparse is None:
            return r.standard_normal((m, d))
        nnz_row, skew = sparse
        p = 1.0 / np.arange(1, d + 1) ** skew
        p /= p.sum()
        cols = r.choice(d, size=(m, nnz_row), p=p)
        vals = r.standard_normal((m, nnz_row))
        X = sp.csr_matrix((vals.ravel(), (np.repeat(np.arange(m), nnz_row), cols.ravel())), shape=(m, d))
        X.sum_duplicates()
        nr = np.sqrt(np.asarray(X.multiply(X).sum(axis=1)).ravel())
        nr[nr == 0] = 1.0
        X = (sp.diags(1.0 / nr) @ X).tocsr()
        X.sort_indices()
        return X

    rng = np.random.default_rng(seed)
    X = draw(rng, n)
    w = np.random.default_rng(seed + 1).standard_normal(d) / np.sqrt(d)
    t = X @ w + b_true + noise * rng.standard_normal(n)
    out = dict(n=n, d=d, X=X, t=t, w_true=w, b_true=float(b_true), eps=float(eps), C=float(C),
               c=np.concatenate([t - eps, -t - eps]), lb=np.zeros(2 * n), ub=np.full(2 * n, float(C)), x0=np.zeros(2 * n))
    if n_test > 0:
        rt = np.random.default_rng(seed + 1000)
        Xt = draw(rt, n_test)
        out.update(X_test=Xt, t_test=Xt @ w + b_true + noise * rt.standard_normal(n_test))
    return out


def svm_blobs(N, d, K, sep, seed, N_test=0, sparse=None):
    """K classes for SVMMulticlass, K <= d.  Sample i has the label i mod K (as a float) and x_i = sep e_label + noise, all draws from default_rng(seed).
    sparse=None: N(0,1) noise in every entry.  sparse=m: N(0,1) noise in m distinct columns per sample, chosen uniformly; sep is then added in the column of the
    label, which may or may not be one of the m, so a sample stores m or m + 1 entries.  Returns dict(n, d, K, X (ndarray), X_csr (scipy CSR of the same
    values), labels); N_test > 0: a held-out draw (X_test, X_test_csr, labels_test) from default_rng(seed + 1000)."""
    import scipy.sparse as sp

    if K > d:
        raise ValueError("svm_blobs: K = %d classes need d >= K" % K)

    def draw(r, n):
        lab = (np.arange(n) % K).astype(np.float64)
        if sparse is None:
            X = r.standard_normal((n, d))
        else:
            X = np.zeros((n, d))
            cols = np.argsort(r.random((n, d)), axis=1)[:, :sparse]
            X[np.repeat(np.arange(n), sparse), cols.ravel()] = r.standard_normal(n * sparse)
        X[np.arange(n), lab.astype(int)] += sep
        Xs = sp.csr_matrix(X)
        Xs.sort_indices()
        return X, Xs, lab

    X, Xs, lab = draw(np.random.default_rng(seed), N)
    out = dict(n=N, d=d, K=K, X=X, X_csr=Xs, labels=lab)
    if N_test > 0:
        Xt, Xts, lt = draw(np.random.default_rng(seed + 1000), N_test)
        out.update(X_test=Xt, X_test_csr=Xts, labels_test=lt)
    return out


def write_contact_problem(path, f):
    """A CubeFeti contact problem (permon_amd.feti.CubeFeti) in the binary layout examples/contact_tfeti.c reads:
    everything pmh_feti_contact_solve takes -- block-diagonal K, f, B as leaves (equality rows first), c, R, the node boxes."""
    K = f.K.tocsr()
    K.sort_indices()
    nn = f.nel + 1
    with open(path, "wb") as fh:
        np.array([0x504D4831, f.nsub, f.N, K.nnz, f.n_lambda, f.n_eq, f.leaves_row.size, f.kdim], dtype=np.int32).tofile(fh)
        np.array([f.ndof], dtype=np.int32).tofile(fh)
        np.array([nn, nn, nn] * f.nsub, dtype=np.int32).tofile(fh)
        for a in (f.block_rowstart, K.indptr, K.indices, f.leaves_row, f.leaves_root):
            np.ascontiguousarray(a, dtype=np.int32).tofile(fh)
        for a in (K.data, f.f, f.leaves_sign, f.c, f.R):
            np.ascontiguousarray(a, dtype=np.float64).tofile(fh)
