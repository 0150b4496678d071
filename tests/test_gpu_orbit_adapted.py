"""GPU tests of the orbit storage applied in the cube group's symmetry-adapted basis (fshared_adapted.h): W_c = (+)_i (W^_i (x) I_d) over the ten irreps of the 48
signed coordinate permutations -- forward transform, ten block products, inverse transform in place of the orbit GEMM and its finishing kernel."""
import ctypes as C

import numpy as np
import pytest

import permon_amd as pa
from permon_amd._lib import check
from permon_amd.chain import FetiDualQP
from permon_amd.feti import box_symmetries

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    check(c.L.pmh_set_knob(b"orbit_adapted", 1)), check(c.L.pmh_set_knob(b"orbit_adapted_spoil", 0))
    c.close()


def _knob(ctx, name):
    v = C.c_int()
    check(ctx.L.pmh_get_knob(name.encode(), C.byref(v)))
    return v.value


def _set(ctx, name, value):
    check(ctx.L.pmh_set_knob(name.encode(), int(value)))


_cache = {}


def _problem(ctx, sub, nel):
    """One operator per shape, shared by the tests: assembled with the adapted form on; the knob then switches between it and the GEMM per application."""
    key = (sub, nel)
    if key not in _cache:
        _set(ctx, "orbit_adapted", 1)
        f = pa.CubeFeti(sub, nel, contact=True)
        G, e = f.coarse()
        nn = nel + 1
        q = FetiDualQP(ctx, f.subset(range(f.nsub)), G, e, f.c, f.lb, kplus_rtol=1e-13, explicit=dict(rtol=1e-13, storage="class_orbit", symmetry=dict(dims=(nn, nn, nn), ndof=3)))
        assert q.explicit_storage == "class_orbit" and q.explicit_symmetries == 48
        _cache[key] = (f, q)
    return _cache[key]


def _dense_F(f):
    Kp = np.linalg.pinv(f.Ki.toarray(), rcond=1e-10, hermitian=True)
    B = f.B.tocsr()
    F = np.zeros((f.n_lambda, f.n_lambda))
    for s in range(f.nsub):
        Bs = B[:, s * f.n_i:(s + 1) * f.n_i].toarray()
        F += Bs @ Kp @ Bs.T
    return F


SHAPES = [((2, 2, 2), 4), ((2, 2, 2), 5), ((4, 4, 4), 4)]


@pytest.mark.parametrize("sub,nel", SHAPES)
def test_adapted_dense_apply_against_longdouble(ctx, sub, nel):
    """(a), (d): Y = blockdiag(W_b) X on a random multivector (zero off every block's touched set) through the adapted form and through the GEMM (knob off), both judged
    against a numpy.longdouble product with the dense blocks of get_block.  Three sums in sequence instead of one, each no longer than the GEMM's, plus one spare factor:
    the adapted form's normwise error may be at most 4 x the GEMM's in the same test, and the GEMM's own error meets the bound derived for a sum of n_c terms
    ((n_c + 8) 2^-53 || |W| |x| || / || ref ||), so that the yardstick has a checked base.  Two applications give the same bits.
    Measured (adapted / GEMM): see docs/LAB_NOTEBOOK.md, entry "Orbit operator in the symmetry-adapted basis"."""
    f, q = _problem(ctx, sub, nel)
    E = q.E
    assert E.orbit_adapted(0)
    ngroups = (f.nsub + 7) // 8
    ntot, _ = E.compressed_size()
    ld = ntot // (8 * ngroups)
    urel = E.class_union(0)
    rng = np.random.default_rng(100 + nel)
    x, ref, mag = np.zeros(ntot), np.zeros(ntot, dtype=np.longdouble), np.zeros(ntot, dtype=np.longdouble)
    touched = np.zeros(ntot, dtype=bool)
    for b in range(f.nsub):
        W, g = E.block(b)
        idx = (b // 8) * ld * 8 + np.searchsorted(urel, g - b * f.n_i) * 8 + b % 8
        x[idx] = rng.standard_normal(idx.size)
        ref[idx] = W.astype(np.longdouble) @ x[idx].astype(np.longdouble)
        mag[idx] = np.abs(W).astype(np.longdouble) @ np.abs(x[idx]).astype(np.longdouble)
        touched[idx] = True
    xv = ctx.vec_from(x)
    ya, ya2, yg = ctx.vec(ntot), ctx.vec(ntot), ctx.vec(ntot)
    E.dense_mult(xv, ya)
    E.dense_mult(xv, ya2)
    _set(ctx, "orbit_adapted", 0)
    try:
        assert not E.orbit_adapted(0)
        E.dense_mult(xv, yg)
    finally:
        _set(ctx, "orbit_adapted", 1)
    ya, ya2, yg = ya.to_numpy(), ya2.to_numpy(), yg.to_numpy()
    assert np.array_equal(ya, ya2)
    nrm = float(np.linalg.norm(ref[touched]))
    err_a = float(np.linalg.norm((ya[touched] - ref[touched]).astype(np.float64))) / nrm
    err_g = float(np.linalg.norm((yg[touched] - ref[touched]).astype(np.float64))) / nrm
    print("orbit_adapted dense apply %s nel %d: adapted %.3e, GEMM %.3e (normwise, against longdouble)" % (sub, nel, err_a, err_g))
    assert not np.any(ya[~touched])  # nothing written off the touched set
    # the yardstick itself: a sum of n_c fused terms in any order is within (n_c + 8) 2^-53 (|W| |x|)_i of the exact one, hence normwise (tests/orbit_cases.py)
    bound_g = (urel.size + 8) * 2.0 ** -53 * float(np.linalg.norm(mag[touched])) / nrm
    print("orbit GEMM dense apply %s nel %d: %.3e against the derived bound %.3e" % (sub, nel, err_g, bound_g))
    assert err_g <= bound_g
    assert err_a <= 4.0 * err_g


@pytest.mark.parametrize("sub,nel", SHAPES[:2])
def test_adapted_F_against_dense_pinv(ctx, sub, nel):
    """(b), (d): F lambda through the adapted form against B pinv(K) B', at the tolerance of test_gpu_explicit.py; bitwise reproducible."""
    f, q = _problem(ctx, sub, nel)
    assert q.E.orbit_adapted(0)
    Fref = _dense_F(f)
    lam = np.random.default_rng(6).standard_normal(f.n_lambda)
    lv, y, y2 = ctx.vec_from(lam), ctx.vec(f.n_lambda), ctx.vec(f.n_lambda)
    q.F.mult(lv, y)
    q.F.mult(lv, y2)
    assert np.array_equal(y.to_numpy(), y2.to_numpy())
    assert np.linalg.norm(y.to_numpy() - Fref @ lam) <= 1e-10 * np.linalg.norm(Fref @ lam)


def test_adapted_F_eight_groups(ctx):
    """(b) for 64 blocks (8 groups: further columns of the same products): F lambda against the inner-Krylov K^+ and against the GEMM."""
    f, q = _problem(ctx, (4, 4, 4), 4)
    assert q.E.orbit_adapted(0)
    G, e = f.coarse()
    q0 = FetiDualQP(ctx, f.subset(range(f.nsub)), G, e, f.c, f.lb, kplus_rtol=1e-13)
    lam = np.random.default_rng(7).standard_normal(f.n_lambda)
    lv, y, y0, yg = ctx.vec_from(lam), ctx.vec(f.n_lambda), ctx.vec(f.n_lambda), ctx.vec(f.n_lambda)
    q.F.mult(lv, y)
    q0.F.mult(lv, y0)
    _set(ctx, "orbit_adapted", 0)
    try:
        q.F.mult(lv, yg)
    finally:
        _set(ctx, "orbit_adapted", 1)
    assert np.linalg.norm(y.to_numpy() - y0.to_numpy()) <= 1e-9 * np.linalg.norm(y0.to_numpy())
    assert np.linalg.norm(y.to_numpy() - yg.to_numpy()) <= 1e-12 * np.linalg.norm(yg.to_numpy())


def test_adapted_contact_solve_same_counts(ctx):
    """(c): the small contact solve with the knob on and off: the same SMALXE / MPGP counters, the same solution."""
    res = []
    for on in (1, 0):
        _set(ctx, "orbit_adapted", on)
        try:
            f = pa.CubeFeti((2, 2, 2), 5, contact=True)
            G, e = f.coarse()
            q = FetiDualQP(ctx, f.subset(range(f.nsub)), G, e, f.c, f.lb, kplus_rtol=1e-12, explicit=dict(rtol=1e-13, storage="class_orbit", symmetry=dict(dims=(6, 6, 6), ndof=3)))
            assert q.E.orbit_adapted(0) == bool(on)
            st = q.solve_smalxe(rtol=1e-6)
            res.append(((st.iteration, st.inner_iter_accu, st.inner.ncg, st.inner.nexp, st.reason), q.dual_solution()))
        finally:
            _set(ctx, "orbit_adapted", 1)
    assert res[0][0] == res[1][0]
    assert np.linalg.norm(res[0][1] - res[1][1]) <= 1e-7 * np.linalg.norm(res[1][1])


def test_adapted_fallbacks(ctx):
    """(e): a class with a 16-operation subgroup, a class whose symmetries came through set_class_symmetry, and a class whose basis was spoilt on purpose (the set-up's
    self-check against the GEMM trips) all keep the GEMM -- and F is right in each."""
    nel = 4
    nn = nel + 1
    f, _ = _problem(ctx, (2, 2, 2), nel)
    G, e = f.coarse()
    loc = f.subset(range(f.nsub))
    Fref = _dense_F(f)
    lam = np.random.default_rng(8).standard_normal(f.n_lambda)
    lv = ctx.vec_from(lam)
    cls = np.zeros(f.nsub, dtype=np.int32)

    def right(E):
        y = ctx.vec(f.n_lambda)
        E.mult(lv, y)
        return np.linalg.norm(y.to_numpy() - Fref @ lam) <= 1e-10 * np.linalg.norm(Fref @ lam)

    q = FetiDualQP(ctx, loc, G, e, f.c, f.lb, kplus_rtol=1e-13)
    # 16 operations: the symmetries are looked for in a matrix whose z components are stiffer, so the swaps with z are dropped (true symmetries of K all the same)
    Kc = f.Ki.tocsr().copy()
    d = np.zeros(f.n_i)
    d[2::3] = 1e-3 * Kc.diagonal().max()
    import scipy.sparse as sp

    E = pa.MatExplicitDual(q.B, q.K, storage="class_orbit", block_class=cls)
    assert E.set_box_symmetry(0, (nn, nn, nn), 3, Kc + sp.diags(d)) == 16
    E.assemble(q.Kplus, slot_class=cls, block_class=cls, rtol=1e-13)
    assert not E.orbit_adapted(0) and right(E)
    E.destroy()
    # all 48, but handed over as bare signed permutations: no operations to build the irreps from
    perm, sign = box_symmetries((nn, nn, nn), 3, f.Ki)
    E = pa.MatExplicitDual(q.B, q.K, storage="class_orbit", block_class=cls)
    assert E.set_class_symmetry(0, perm, sign) == 48
    E.assemble(q.Kplus, slot_class=cls, block_class=cls, rtol=1e-13)
    assert not E.orbit_adapted(0) and right(E)
    E.destroy()
    # a wrong table
    n_fb, n_ok = _knob(ctx, "orbit_adapted_fallbacks"), _knob(ctx, "orbit_adapted_classes")
    _set(ctx, "orbit_adapted_spoil", 1)
    E = pa.MatExplicitDual(q.B, q.K, storage="class_orbit", block_class=cls)
    assert E.set_box_symmetry(0, (nn, nn, nn), 3, f.Ki) == 48
    E.assemble(q.Kplus, slot_class=cls, block_class=cls, rtol=1e-13)
    assert _knob(ctx, "orbit_adapted_fallbacks") == n_fb + 1 and _knob(ctx, "orbit_adapted_classes") == n_ok and _knob(ctx, "orbit_adapted_spoil") == 0
    assert not E.orbit_adapted(0) and right(E)
    E.destroy()
    # and the same class unspoilt takes the adapted form
    E = pa.MatExplicitDual(q.B, q.K, storage="class_orbit", block_class=cls)
    assert E.set_box_symmetry(0, (nn, nn, nn), 3, f.Ki) == 48
    E.assemble(q.Kplus, slot_class=cls, block_class=cls, rtol=1e-13)
    assert _knob(ctx, "orbit_adapted_classes") == n_ok + 1 and E.orbit_adapted(0) and right(E)
    E.destroy()
