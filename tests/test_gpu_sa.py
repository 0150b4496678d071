"""K^+ for subdomains that are NOT boxes (round 6): the algebraic hierarchy built inside the library (pmh_mg_create_sa, csrc/mgsa.hip: smoothed aggregation with the
block's kernel as near-kernel) as the PC of MATINV's inner CG -- the reference factorises ANY block (src/mat/impls/inv/matinv.c:481-580, apply :734-743) and inverts it
explicitly column block by column block (:640-730); here that is the V-cycle-preconditioned block CG and the multi-right-hand-side assembly of the explicit local dual
operators, with no box, no symmetry, no congruent partner and no caller-supplied P.

Decompositions: the (2 n)^3-element cube of configs[2]'s generator re-cut into 8 staircase-bounded / L-shaped subdomains (permon_amd.feti.irregular_partition,
MeshFeti: local numbering = nodes in ascending global order, gluing through pmh_feti_gluing_from_l2g).  Checked: the hierarchy against its scipy restatement
(feti.sa_mg_hierarchy + oracle.mg_host.vcycle), K^+ against numpy.linalg.pinv, F against B pinv(K) B' to 1e-10, the CG iteration counts (<= 25), and the contact
solution of the irregular decomposition against the SAME mesh cut into boxes (one body, two decompositions: the same displacement field)."""
import numpy as np
import pytest
import scipy.sparse as sp

import permon_amd as pa
from permon_amd import feti
from permon_amd.chain import FetiDualQP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    c.close()


def _local(f):
    return f.subset(range(f.nsub))


def test_sa_cycle_matches_scipy_restatement(ctx):
    """One V-cycle of the C++-built hierarchy (fp64) on three staircase blocks against oracle.mg_host.vcycle on feti.sa_mg_hierarchy: same aggregates, same
    Gram-Schmidt, same smoothing => the same linear operator to rounding.  (The long-row transfer kernels this hierarchy takes are compared with == in
    tests/test_gpu_mg_paths.py, case long_rows; this test stays for the hierarchy BUILDER.)"""
    from oracle import mg_host

    f = feti.MeshFeti(feti.irregular_partition(6, "staircase"), contact=False)
    sel = [0, 3, 7]
    rs = f.block_rowstart
    blocks = [f.blocks[s] for s in sel]
    nns = [f.R[:, rs[s]:rs[s + 1]] for s in sel]
    K = feti.csr_block_diag(blocks)
    brs = np.concatenate([[0], np.cumsum([b.shape[0] for b in blocks])]).astype(np.int32)
    R = np.concatenate(nns, axis=1)
    H = feti.sa_mg_hierarchy(blocks, nns, ndof=3, max_coarse=200, theta=0.08)
    assert len(H["A"]) >= 2
    Kd = pa.MatBlockDiag.from_scipy(ctx, brs, K)
    Mi = pa.MatInv(Kd, rtol=1e-12, nullspace=R)
    mg = Mi.set_pc_mg_sa(K, 3, R=R, max_coarse=200, theta=0.08, precision="fp64")
    V = mg_host.vcycle(H, 2)
    rng = np.random.default_rng(3)
    for _ in range(2):
        b = rng.standard_normal(K.shape[0])
        x = ctx.vec(K.shape[0])
        mg.apply(ctx.vec_from(b), x)
        ref = V(b)
        assert np.linalg.norm(x.to_numpy() - ref) <= 1e-9 * np.linalg.norm(ref)
    Mi.destroy()
    Kd.destroy()


@pytest.mark.parametrize("kind,precision", [("staircase", "fp64"), ("staircase", "fp16"), ("lshape", "fp32")])
def test_sa_kplus_on_irregular_blocks_vs_pinv(ctx, kind, precision):
    """pmh_matinv_mult with the algebraic V-cycle on 8 blocks that are not boxes: K^+ f = pinv(K) f, and the CG needs <= 25 iterations at rtol 1e-12 (Jacobi: hundreds)."""
    f = feti.MeshFeti(feti.irregular_partition(6, kind), contact=False)
    loc = _local(f)
    K = loc["K"]
    Kd = pa.MatBlockDiag.from_scipy(ctx, loc["block_rowstart"], K)
    Mi = pa.MatInv(Kd, rtol=1e-12, nullspace=loc["R"])
    if precision != "fp64":
        Mi.enable_bsr3()
    Mi.set_pc_mg_sa(K, 3, R=loc["R"], max_coarse=300, precision=precision)
    rng = np.random.default_rng(4)
    rhs = rng.standard_normal(f.N)
    u = ctx.vec(f.N)
    Mi.mult(ctx.vec_from(rhs), u)
    its, _ = Mi.last_iterations()
    assert its <= 25, its
    got = u.to_numpy()
    rs = f.block_rowstart
    for s in range(f.nsub):
        ref = np.linalg.pinv(f.blocks[s].toarray(), rcond=1e-10, hermitian=True) @ rhs[rs[s]:rs[s + 1]]
        assert np.linalg.norm(got[rs[s]:rs[s + 1]] - ref) <= 1e-9 * np.linalg.norm(ref)
    # Jacobi-preconditioned CG on the same blocks for scale
    Mj = pa.MatInv(Kd, rtol=1e-12, nullspace=loc["R"], jacobi=True)
    Mj.mult(ctx.vec_from(rhs), u)
    assert Mj.last_iterations()[0] > 4 * its
    Mj.destroy()
    Mi.destroy()
    Kd.destroy()


def test_sa_non_singular_blocks_default_near_kernel(ctx):
    """Blocks with Dirichlet conditions eliminated IN the matrix (identity rows: non-singular, no kernel handed over): the near-kernel defaults to the three translations
    (or the caller's rigid-body modes, `nns`), isolated dofs become singleton aggregates with dead coarse dofs; K^{-1} f against a direct solve."""
    f = feti.MeshFeti(feti.irregular_partition(5, "lshape"), contact=False)
    rs = f.block_rowstart
    blocks, rb = [], []
    for s in (0, 2):
        Kb = f.blocks[s].tolil()
        X = f.coords[s]
        fix = np.nonzero(X[:, 0] == X[:, 0].min())[0]
        dd = (fix[:, None] * 3 + np.arange(3)[None, :]).ravel()
        keep = np.ones(Kb.shape[0])
        keep[dd] = 0.0
        D = sp.diags(keep)
        Kb = (D @ f.blocks[s] @ D + sp.diags(1.0 - keep)).tocsr()
        Kb.eliminate_zeros()
        Kb.sort_indices()
        blocks.append(Kb)
        Q = np.zeros((6, Kb.shape[0]))  # rigid-body modes from the coordinates as the caller's near-kernel
        Q[0, 0::3] = Q[1, 1::3] = Q[2, 2::3] = 1.0
        Q[3, 0::3], Q[3, 1::3] = -X[:, 1], X[:, 0]
        Q[4, 1::3], Q[4, 2::3] = -X[:, 2], X[:, 1]
        Q[5, 0::3], Q[5, 2::3] = X[:, 2], -X[:, 0]
        rb.append(Q)
    K = feti.csr_block_diag(blocks)
    brs = np.concatenate([[0], np.cumsum([b.shape[0] for b in blocks])]).astype(np.int32)
    Kd = pa.MatBlockDiag.from_scipy(ctx, brs, K)
    rhs = np.random.default_rng(8).standard_normal(K.shape[0])
    from scipy.sparse.linalg import spsolve

    ref = spsolve(K.tocsc(), rhs)
    counts = []
    for nns in (None, np.concatenate(rb, axis=1)):
        Mi = pa.MatInv(Kd, rtol=1e-11, nullspace=None)
        Mi.set_pc_mg_sa(K, 3, R=None, nns=nns, max_coarse=200, precision="fp64")
        u = ctx.vec(K.shape[0])
        Mi.mult(ctx.vec_from(rhs), u)
        counts.append(Mi.last_iterations()[0])
        assert np.linalg.norm(u.to_numpy() - ref) <= 1e-8 * np.linalg.norm(ref)
        Mi.destroy()
    assert counts[1] <= counts[0] and counts[1] <= 25, counts  # the rotations in the near-kernel pay
    Kd.destroy()


@pytest.fixture(scope="module")
def staircase(ctx):
    n = 6
    f = feti.MeshFeti(feti.irregular_partition(n, "staircase"), contact=True)
    G, e = f.coarse(orthonormalize=True)
    loc = _local(f)
    q = FetiDualQP(ctx, loc, G, e, f.c, f.lb, kplus_rtol=1e-12, mg_sa=dict(ndof=3, max_coarse=300), mg_precision="fp16", bsr3=True, explicit=dict(rtol=1e-13, storage="auto"))
    return f, loc, G, e, q


def test_irregular_partition_explicit_F_vs_dense(ctx, staircase):
    """The verdict's acceptance test: an irregular partition, no P from the caller, the explicit operators assembled 8 columns per block at a time on the algebraic
    hierarchy, F = B pinv(K) B' to 1e-10."""
    f, loc, G, e, q = staircase
    cls = pa.csr_block_classes(loc["block_rowstart"], loc["K"])
    assert sorted(cls.tolist()) == list(range(8))  # no two blocks are congruent
    assert q.explicit_storage == "sym" and q.explicit_multi_rhs  # per-block symmetric tiles (k_fx_symv), set up by the multi-right-hand-side K^+
    Bd = f.B.toarray()
    rs = f.block_rowstart
    Fd = np.zeros((f.n_lambda, f.n_lambda))
    for s in range(f.nsub):
        Bs = Bd[:, rs[s]:rs[s + 1]]
        Fd += Bs @ np.linalg.pinv(f.blocks[s].toarray(), rcond=1e-10, hermitian=True) @ Bs.T
    rng = np.random.default_rng(6)
    for _ in range(2):
        lam = rng.standard_normal(f.n_lambda)
        y = ctx.vec(f.n_lambda)
        q.F.mult(ctx.vec_from(lam), y)
        ref = Fd @ lam
        assert np.linalg.norm(y.to_numpy() - ref) <= 1e-10 * np.linalg.norm(ref)
    n_solves, _ = q.E.assemble_stats()
    assert n_solves == int(q.E.n_gamma.sum())


def test_irregular_partition_contact_solution_equals_box_decomposition(ctx, staircase):
    """One body, two decompositions: the staircase cut (algebraic hierarchy, per-block explicit operators) and the 2 x 2 x 2 boxes (box hierarchy, the orbit storage of the
    headline) of the SAME mesh, load, Dirichlet face and obstacle, both through the one-call solve pmh_feti_contact_solve (dims = NULL: pmh_mg_create_sa).  SMALXE + MPGP
    converge on both, the recovered displacement fields agree at every global node, the contact multipliers are feasible and complementary; and the staircase solve
    through the Python-assembled chain (the fixture) gives the same multipliers."""
    from permon_amd.chain import FETIContactSolve

    f, loc, G, e, q = staircase

    def assemble(fm, uloc):
        nglob = int(max(g.max() for g in fm.l2g)) + 1
        out, cnt = np.zeros(nglob), np.zeros(nglob)
        rs = fm.block_rowstart
        for s, g in enumerate(fm.l2g):
            np.add.at(out, g, uloc[rs[s]:rs[s + 1]])
            np.add.at(cnt, g, 1.0)
        return out / cnt

    u, lam, st = FETIContactSolve(ctx, f, rtol=1e-7, kplus_rtol=1e-11, mg_min_nodes=100, dims=None)
    assert st.smalxe.reason > 0 and st.explicit_symmetries <= 1
    assert st.explicit_solves == int(np.unique(f.leaves_row).size)  # one K^+ column per touched dof: nothing shared, nothing found by symmetry
    lamI = lam[f.n_eq:]
    assert lamI.min() >= -1e-12 and (lamI > 0).sum() > 0
    Bu = f.B @ u
    assert np.abs(Bu[:f.n_eq]).max() <= 1e-5 * np.abs(u).max()  # glued and fixed
    gap = Bu[f.n_eq:] - f.c[f.n_eq:]
    assert gap.max() <= 1e-5 * np.abs(u).max() and np.abs(gap[lamI > 0]).max() <= 1e-5 * np.abs(u).max()  # no penetration; multipliers only where the gap is closed
    fb = feti.MeshFeti(feti.irregular_partition(6, "cubes"), contact=True)
    ub, lamb, sb = FETIContactSolve(ctx, fb, rtol=1e-7, kplus_rtol=1e-11, mg_min_nodes=27, dims=[(7, 7, 7)] * 8, explicit_storage="class_orbit")
    assert sb.smalxe.reason > 0 and sb.explicit_symmetries == 48
    ug, ubg = assemble(f, u), assemble(fb, ub)
    assert np.linalg.norm(ug - ubg) <= 2e-5 * np.linalg.norm(ubg)
    # the chain assembled from Python on the same decomposition: same dual solution
    sq = q.solve_smalxe(rtol=1e-7)
    assert sq.reason > 0
    lq = q.dual_solution()
    assert np.linalg.norm(lq - lam) <= 1e-4 * np.linalg.norm(lam)


@pytest.mark.parametrize("regularize", [None, True, False])
def test_kspfeti_on_an_irregular_partition_with_the_algebraic_pc(ctx, regularize):
    """KSPFETI (src/ksp/impls/feti/feti.c:71-156) on a decomposition into subdomains that are not boxes, `-dual_mat_inv_pc_type gamg`: MATINV's inner KSP preconditioned by the
    algebraic V-cycle, on each of the three generalised inverses (the left inverse K^- P_R that KSPFETI takes by itself, K_reg^{-1}, the Moore-Penrose form).  The outer CG
    count (to +-1) and u as with the Jacobi-preconditioned inner KSP, u equal to the direct solve of the assembled problem."""
    from scipy.sparse.linalg import spsolve

    from permon_amd.chain import KSPFETISolve

    f = feti.MeshFeti(feti.irregular_partition(5, "staircase"), contact=False)
    l2g = np.concatenate(f.l2g).astype(np.int32)
    rs = f.block_rowstart
    GX = f.elem_sub.shape[2] + 1
    dl = np.concatenate([(np.nonzero(g % GX == 0)[0][:, None] * 3 + np.arange(3)[None, :]).ravel() + rs[s] for s, g in enumerate(f.gnodes)]).astype(np.int32)
    res = {}
    for pc in ("jacobi", "gamg"):
        u, lam, st = KSPFETISolve(ctx, rs, f.K, f.f, l2g, dirichlet_local=dl, R=f.R, regularize=regularize, rtol=1e-8, kplus_rtol=1e-12, kplus_pc=pc)
        assert st.reason > 0
        res[pc] = (u, st.iteration)
    assert abs(res["jacobi"][1] - res["gamg"][1]) <= 1  # (two inner solvers at rtol 1e-12: the outer count may move by one at the stopping iteration)
    assert np.linalg.norm(res["jacobi"][0] - res["gamg"][0]) <= 1e-6 * np.linalg.norm(res["jacobi"][0])
    # the assembled problem: K_glob u = f_glob with u = 0 on x = 0
    nglob = int(l2g.max()) + 1
    A = sp.csr_matrix((np.ones(f.N), (np.arange(f.N), l2g)), shape=(f.N, nglob))
    Kg = (A.T @ f.K @ A).tocsr()
    fg = A.T @ f.f
    fixed = np.zeros(nglob, dtype=bool)
    fixed[np.unique(l2g[dl])] = True
    free = np.nonzero(~fixed)[0]
    ug = np.zeros(nglob)
    ug[free] = spsolve(Kg[free][:, free].tocsc(), fg[free])
    ua = np.zeros(nglob)
    ua[l2g] = res["gamg"][0]  # (INSERT_VALUES assembly of the copies, as QPTPostSolve_QPTMatISToBlockDiag)
    assert np.linalg.norm(ua - ug) <= 1e-5 * np.linalg.norm(ug)
    # and through the options database key
    u2, _, st2 = KSPFETISolve(ctx, rs, f.K, f.f, l2g, dirichlet_local=dl, R=f.R, regularize=regularize, rtol=1e-8, kplus_rtol=1e-12, options="-dual_mat_inv_pc_type gamg")
    assert st2.iteration == res["gamg"][1] and np.array_equal(u2, res["gamg"][0])


def test_sa_scalar_problem_poisson_blocks(ctx):
    """The same builder on a SCALAR problem (Poisson, one dof per node, kernel = the constant): aggregates of nodes, one coarse dof each, fp64 cycle on the CSR kernels (no 3 x 3
    blocks anywhere) -- K^+ = pinv(K) on the 8 staircase blocks, and the one-call contact solve (obstacle under the z = 0 face) takes the same path."""
    from permon_amd.chain import FETIContactSolve

    f = feti.MeshFeti(feti.irregular_partition(6, "staircase"), physics="poisson", contact=True)
    assert f.ndof == 1 and f.kdim == 1
    loc = _local(f)
    Kd = pa.MatBlockDiag.from_scipy(ctx, loc["block_rowstart"], loc["K"])
    Mi = pa.MatInv(Kd, rtol=1e-12, nullspace=loc["R"])
    Mi.set_pc_mg_sa(loc["K"], 1, R=loc["R"], max_coarse=60, precision="fp64")
    rhs = np.random.default_rng(9).standard_normal(f.N)
    u = ctx.vec(f.N)
    Mi.mult(ctx.vec_from(rhs), u)
    assert Mi.last_iterations()[0] <= 25
    rs = f.block_rowstart
    for s in range(f.nsub):
        ref = np.linalg.pinv(f.blocks[s].toarray(), rcond=1e-10, hermitian=True) @ rhs[rs[s]:rs[s + 1]]
        assert np.linalg.norm(u.to_numpy()[rs[s]:rs[s + 1]] - ref) <= 1e-9 * np.linalg.norm(ref)
    Mi.destroy()
    Kd.destroy()
    uu, lam, st = FETIContactSolve(ctx, f, rtol=1e-7, kplus_rtol=1e-11, mg_min_nodes=20, dims=None)
    assert st.smalxe.reason > 0
    Bu = f.B @ uu
    assert np.abs(Bu[:f.n_eq]).max() <= 1e-5 * np.abs(uu).max() and (Bu[f.n_eq:] - f.c[f.n_eq:]).max() <= 1e-5 * np.abs(uu).max()


def test_sa_on_congruent_blocks_is_built_once_and_falls_back_politely(ctx):
    """8 congruent cubes through the ALGEBRAIC builder: one class, its hierarchy built once and replicated; pmh_matinv_mult's 8-columns-of-one-block mode needs a node-wise P
    for congruent blocks and is refused without an error (the one-column cycle with the scalar transfers runs); K^+ = pinv(K), and the 8-column set-up solver applies."""
    f = pa.CubeFeti((2, 2, 2), 6, contact=False)
    loc = f.subset(range(8))
    Kd = pa.MatBlockDiag.from_scipy(ctx, loc["block_rowstart"], loc["K"])
    Mi = pa.MatInv(Kd, rtol=1e-12, nullspace=loc["R"])
    Mi.enable_bsr3()
    Mi.set_pc_mg_sa(loc["K"], 3, R=loc["R"], max_coarse=150, precision="fp16")
    assert Mi.bsr3_replicas() == 8 and not Mi.multi_rhs_active()
    rhs = np.random.default_rng(10).standard_normal(f.N)
    u = ctx.vec(f.N)
    Mi.mult(ctx.vec_from(rhs), u)
    assert Mi.last_iterations()[0] <= 20
    Kp = np.linalg.pinv(f.Ki.toarray(), rcond=1e-10, hermitian=True)
    got = u.to_numpy()
    for s in range(8):
        ref = Kp @ rhs[s * f.n_i:(s + 1) * f.n_i]
        assert np.linalg.norm(got[s * f.n_i:(s + 1) * f.n_i] - ref) <= 1e-9 * np.linalg.norm(ref)
    F8, U8 = ctx.vec_from(np.random.default_rng(11).standard_normal(8 * f.N)), ctx.vec(8 * f.N)
    assert Mi.mult_multi(F8, U8) <= 20
    X = U8.to_numpy().reshape(f.N, 8)
    B8 = F8.to_numpy().reshape(f.N, 8)
    ref = Kp @ B8[:f.n_i, 3]
    assert np.linalg.norm(X[:f.n_i, 3] - ref) <= 1e-9 * np.linalg.norm(ref)
    Mi.destroy()
    Kd.destroy()
