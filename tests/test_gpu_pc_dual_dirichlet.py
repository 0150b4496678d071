"""PCDUAL dirichlet (pmh_op_create_pc_dual_dirichlet, csrc/pcdual.hip): M = B S B', S_b = K_GG - K_GI K_II^-1 K_IG on the dofs B touches.
The blocks and the apply against numpy, the preconditioned CG on P F through the Python chain and through pmh_kspfeti_solve, and the set-up counters."""
import ctypes as C

import numpy as np
import pytest

import permon_amd as pa
from permon_amd import _lib
from permon_amd.chain import FetiDualQP
from permon_amd.feti import DmdaFeti

pytestmark = pytest.mark.gpu

CUBE = ((12, 12, 12), 8, "elasticity", "full")  # 8 blocks of 7^3 nodes: 381 dofs on Gamma_b, 648 interior
SLABS = ((8, 6, 4), 7, "elasticity")            # ex71_2: four of the seven slabs have no interior


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def probs():
    return {"cube": DmdaFeti(*CUBE), "slabs": DmdaFeti(*SLABS)}


def _gammas(prob):
    rs = prob.block_rowstart
    tr = np.unique(prob.leaves_row)
    return [tr[(tr >= rs[b]) & (tr < rs[b + 1])] for b in range(prob.nsub)]


def _schur(prob):
    """numpy: (Gamma_b as rank-local dofs, S_b = K_GG - K_GI solve(K_II, K_IG), n_I) for every block."""
    rs, K, out = prob.block_rowstart, prob.K.tocsr(), []
    for b, g in enumerate(_gammas(prob)):
        Kb = K[rs[b]:rs[b + 1], rs[b]:rs[b + 1]].toarray()
        G = g - rs[b]
        I = np.setdiff1d(np.arange(Kb.shape[0]), G)
        S = Kb[np.ix_(G, G)]
        if I.size:
            S = S - Kb[np.ix_(G, I)] @ np.linalg.solve(Kb[np.ix_(I, I)], Kb[np.ix_(I, G)])
        out.append((g, S, I.size))
    return out


def _operators(ctx, prob):
    B = pa.MatGluing(ctx, prob.N, prob.n_lambda, prob.leaves_row, prob.leaves_root, prob.leaves_sign)
    K = pa.MatBlockDiag.from_scipy(ctx, prob.block_rowstart, prob.K)
    return B, K


@pytest.mark.parametrize("name", ["cube", "slabs"])
@pytest.mark.parametrize("storage", ["sym", "full"])
def test_blocks_apply_and_stats_against_numpy(ctx, probs, name, storage):
    prob = probs[name]
    ref = _schur(prob)
    B, K = _operators(ctx, prob)
    M = pa.PCDualDirichletOp(B, K, storage=storage, rtol=1e-12)
    for b, (g, S, nI) in enumerate(ref):
        Sg, gg = M.block(b)
        assert np.array_equal(gg, g)
        assert np.array_equal(Sg, Sg.T)  # exactly symmetric, as stored
        err = np.linalg.norm(Sg - S) / np.linalg.norm(S)
        assert err <= 1e-9, (b, nI, err)
    # y = B S B' lambda
    Bd = prob.B.tocsc()
    lam = np.random.default_rng(7).standard_normal(prob.n_lambda)
    yref = np.zeros(prob.n_lambda)
    for g, S, _ in ref:
        Bg = Bd[:, g]
        yref += Bg @ (S @ (Bg.T @ lam))
    x, y = ctx.vec_from(lam), ctx.vec(prob.n_lambda)
    M.mult(x, y)
    assert np.linalg.norm(y.to_numpy() - yref) <= 1e-9 * np.linalg.norm(yref)
    # one interior solve per column of every block that has an interior; the dense bytes of a pmh_fexplicit of that storage
    n_solves, seconds, dense_bytes = M.stats()
    assert n_solves == sum(len(g) for g, _, nI in ref if nI > 0)
    assert n_solves == ({"cube": 8 * 381, "slabs": 105 + 210 + 105}[name])
    E = pa.MatExplicitDual(B, K, storage=storage)
    assert dense_bytes == E.dense_bytes and dense_bytes >= (4 if storage == "sym" else 8) * sum(len(g) ** 2 for g, _, _ in ref)
    assert seconds > 0.0
    E.destroy()
    M.destroy()


def test_storage_and_arguments_refused(ctx, probs):
    prob = probs["slabs"]
    B, K = _operators(ctx, prob)
    for storage in (2, 3, 4):  # class-shared storage: not built, said so
        with pytest.raises(pa.PermonHipError) as ex:
            h = C.c_void_p()
            _lib.check(ctx.L.pmh_op_create_pc_dual_dirichlet(B.h, K.h, storage, 1e-12, 1000, C.byref(h)))
        assert ex.value.code == 4
    with pytest.raises(pa.PermonHipError):
        pa.PCDualDirichletOp(B, K, rtol=1e-12, max_it=1)  # an interior solve that cannot converge is an error, not an inexact S
    with pytest.raises(ValueError):
        FetiDualQP(ctx, prob.local(), *prob.coarse(), prob.c, prob.lb, orthonormal=False).solve_ksp(pc_type="neumann")


def _coarse_correct(prob, dq):
    u, Fl = dq.primal_solution(None)
    G, _ = prob.coarse()
    alpha = -np.linalg.solve((G @ G.T).toarray(), G @ Fl)  # G' alpha = d - F lambda
    Rm = np.zeros((G.shape[0], prob.N))
    r0 = 0
    for s, R in enumerate(prob.Rblocks):
        Rm[r0:r0 + R.shape[0], prob.block_rowstart[s]:prob.block_rowstart[s + 1]] = R
        r0 += R.shape[0]
    return u - Rm.T @ alpha


def _solve(ctx, prob, pc_type, rtol):
    G, e = prob.coarse()
    dq = FetiDualQP(ctx, prob.local(), G, e, prob.c, prob.lb, orthonormal=False, kplus_rtol=1e-13)
    st = dq.solve_ksp(rtol=rtol, pc_type=pc_type)
    return dq, st


def test_iterations_cube(ctx, probs):
    prob = probs["cube"]
    its = {pc: _solve(ctx, prob, pc, 1e-6)[1] for pc in ("none", "lumped", "dirichlet")}
    print("12^3 elasticity, rtol 1e-6: " + ", ".join("%s %d" % (k, v.iteration) for k, v in its.items()))
    assert all(st.reason == 2 for st in its.values())
    assert abs(its["dirichlet"].iteration - 12) <= 1
    assert its["lumped"].iteration - its["dirichlet"].iteration >= 3
    # `lumped=True` keeps its meaning and agrees with pc_type="lumped"
    assert _solve(ctx, prob, None, 1e-6)[1].iteration == its["none"].iteration
    G, e = prob.coarse()
    dq = FetiDualQP(ctx, prob.local(), G, e, prob.c, prob.lb, orthonormal=False, kplus_rtol=1e-13)
    assert dq.solve_ksp(rtol=1e-6, lumped=True).iteration == its["lumped"].iteration


def test_iterations_slabs(ctx, probs):
    dq, st = _solve(ctx, probs["slabs"], "dirichlet", 1e-6)
    print("ex71_2 slabs, rtol 1e-6: dirichlet %d" % st.iteration)
    assert st.reason == 2 and abs(st.iteration - 24) <= 2


def test_same_answer_as_unpreconditioned(ctx, probs):
    prob = probs["cube"]
    rtol = 1e-9
    dn, sn = _solve(ctx, prob, "none", rtol)
    dd, sd = _solve(ctx, prob, "dirichlet", rtol)
    assert sn.reason == sd.reason == 2 and sd.iteration < sn.iteration
    ln, ld = dn.dual_solution(), dd.dual_solution()
    un, ud = _coarse_correct(prob, dn), _coarse_correct(prob, dd)
    print("12^3: |lambda_d - lambda_n| / |lambda_n| = %.2e, |u_d - u_n| / |u_n| = %.2e" % (np.linalg.norm(ld - ln) / np.linalg.norm(ln), np.linalg.norm(ud - un) / np.linalg.norm(un)))
    assert np.linalg.norm(ld - ln) <= 1e-6 * np.linalg.norm(ln)
    assert np.linalg.norm(ud - un) <= 1e-6 * np.linalg.norm(un)
    res = prob.K @ ud - prob.f + prob.B.T @ ld  # the primal equations of the Dirichlet-preconditioned solve
    assert np.linalg.norm(res) <= 1e-6 * np.linalg.norm(prob.f)


def _l2g(prob):
    nd = prob.ndof
    return np.concatenate([(np.asarray(g)[:, None] * nd + np.arange(nd)[None, :]).ravel() for g in prob.gids]).astype(np.int32)


def test_kspfeti_front_end(ctx, probs):
    """-dual_pc_dual_type dirichlet from the options string: the count of the Python path on the same chain (the Moore-Penrose K^+, -qpt_dualize_Kplus_mp);
    the keyword gives the same; -project 0 refuses it as it refuses lumped."""
    prob = probs["cube"]
    py = _solve(ctx, prob, "dirichlet", 1e-6)[1].iteration
    args = (ctx, prob.block_rowstart, prob.K, prob.f, _l2g(prob))
    u, lam, st = pa.KSPFETISolve(*args, R=prob.R, kplus_rtol=1e-13, options="-pde_type Elasticity -dim 3 -qps_rtol 1e-6 -qpt_dualize_Kplus_mp -dual_pc_dual_type dirichlet")
    print("12^3 through pmh_kspfeti_solve: dirichlet %d (Python path %d)" % (st.iteration, py))
    assert st.reason == 2 and st.iteration == py
    assert np.linalg.norm(prob.B @ u) <= 1e-4 * np.linalg.norm(u)
    u2, _, st2 = pa.KSPFETISolve(*args, R=prob.R, kplus_rtol=1e-13, regularize=False, rtol=1e-6, pc_dual_type="dirichlet")
    assert st2.iteration == st.iteration and np.linalg.norm(u2 - u) <= 1e-12 * np.linalg.norm(u)
    with pytest.raises(pa.PermonHipError) as ex:
        pa.KSPFETISolve(*args, R=prob.R, options="-project 0 -dual_pc_dual_type dirichlet")
    assert ex.value.code == 4 and "dirichlet" in str(ex.value)
