"""The transforms of the orbit operator's symmetry-adapted form for multivectors of at most 16 columns (k_fxa_narrow, csrc/fshared_adapted.h) against the wide
kernels (k_fxa_transform, knob orbit_narrow = 0 at the assembly) bit for bit, and each transform alone (pmh_fexplicit_orbit_adapted_transform) against
numpy.longdouble products with the host tables of permon_amd.mat.orbit_basis.  The problems are those of tests/golden/make_orbit_adapted_bits.py::problem.

  2x2x2 of 4^3   5 nodes per edge: nodes on the symmetry planes, orbits of sizes that are no multiple of 4 (asserted)
  2x2x2 of 5^3   even node count: no node on a symmetry plane
  4x2x2          16 blocks, NC = 16: two groups of columns (the smallest nel >= 4 at which the class takes the adapted form)
  4x4x4 of 4^3   NC = 64: the wide kernels stay"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import permon_amd as pa
from permon_amd._lib import check
from permon_amd.mat import orbit_basis

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_orbit_adapted_bits", os.path.join(HERE, "golden", "make_orbit_adapted_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    check(c.L.pmh_set_knob(b"orbit_narrow", 1))
    c.close()


_cache = {}


def _problem(ctx, sub, nel, narrow):
    """One operator per (shape, orbit_narrow at its assembly), shared by the tests and left unchanged"""
    key = (sub, nel, narrow)
    if key not in _cache:
        check(ctx.L.pmh_set_knob(b"orbit_narrow", int(narrow)))
        try:
            _cache[key] = gen.problem(ctx, sub, nel)
        finally:
            check(ctx.L.pmh_set_knob(b"orbit_narrow", 1))
    return _cache[key]


_nel16 = []


def _nel_two_groups(ctx):
    """4x2x2: the smallest nel >= 4 at which class 0 takes the adapted form (gen.problem asserts that it does)"""
    if not _nel16:
        for nel in range(4, 9):
            try:
                _problem(ctx, (4, 2, 2), nel, 1)
            except AssertionError:
                continue
            _nel16.append(nel)
            break
    assert _nel16, "4x2x2: no nel in 4 .. 8 takes the symmetry-adapted form"
    return _nel16[0]


def _shape(ctx, name):
    return {"2x2x2/nel4": ((2, 2, 2), 4), "2x2x2/nel5": ((2, 2, 2), 5)}[name] if name != "4x2x2" else ((4, 2, 2), _nel_two_groups(ctx))


def _layout(ctx, f, q):
    E = q.E
    ngroups = (f.nsub + 7) // 8
    ntot, _ = E.compressed_size()
    ld = ntot // (8 * ngroups)
    urel = E.class_union(0)
    touched = np.zeros(ntot, dtype=bool)
    for b in range(f.nsub):
        g = np.zeros(int(E.n_gamma[b]), dtype=np.int32)
        check(ctx.L.pmh_fexplicit_get_block(E.h, b, None, g.ctypes.data_as(C.c_void_p)))
        touched[(b // 8) * ld * 8 + np.searchsorted(urel, g - b * f.n_i) * 8 + b % 8] = True
    return ngroups, ntot, ld, urel, touched


def _seeded(ntot, touched, seed):
    x = np.zeros(ntot)
    x[touched] = np.random.default_rng(seed).standard_normal(int(touched.sum()))
    return x


@pytest.mark.parametrize("name", ["2x2x2/nel4", "2x2x2/nel5", "4x2x2"])
def test_transform_bits(ctx, name):
    """dense_mult on a seeded multivector that is zero off the touched sets: the narrow kernels (orbit_narrow = 1) and the wide ones (= 0) give the same bits, and two
    applications of either do"""
    sub, nel = _shape(ctx, name)
    fn, qn = _problem(ctx, sub, nel, 1)
    fw, qw = _problem(ctx, sub, nel, 0)
    info_n, info_w = qn.E.orbit_adapted_info(0), qw.E.orbit_adapted_info(0)
    assert all(i["narrow"] for i in info_n) and not any(i["narrow"] for i in info_w)
    ngroups, ntot, ld, urel, touched = _layout(ctx, fn, qn)
    assert ngroups == (2 if name == "4x2x2" else 1)
    x = _seeded(ntot, touched, 7 + nel)
    out = []
    for q in (qn, qw):
        xv, y, y2 = ctx.vec_from(x), ctx.vec(ntot), ctx.vec(ntot)
        q.E.dense_mult(xv, y)
        q.E.dense_mult(xv, y2)
        y, y2 = y.to_numpy(), y2.to_numpy()
        assert np.array_equal(y, y2) and np.any(y)
        out.append(y)
    assert np.array_equal(out[0], out[1])
    assert not np.any(out[0][~touched])
    lam = np.random.default_rng(6).standard_normal(fn.n_lambda)
    z = []
    for q in (qn, qw):
        lv, zz = ctx.vec_from(lam), ctx.vec(fn.n_lambda)
        q.F.mult(lv, zz)
        z.append(zz.to_numpy())
    assert np.array_equal(z[0], z[1]) and np.any(z[0])


def test_wide_kernels_stay_for_64_columns(ctx):
    """4x4x4 of 4^3 (NC = 64) with orbit_narrow = 1: the class keeps k_fxa_transform"""
    f, q = _problem(ctx, (4, 4, 4), 4, 1)
    assert (f.nsub + 7) // 8 == 8
    assert not any(i["narrow"] for i in q.E.orbit_adapted_info(0))


def _host_tables(nel, urel):
    nn = nel + 1
    B = orbit_basis((nn, nn, nn), 3, urel)
    tbase = np.concatenate(([0], np.cumsum(B["orb_size"])))
    return B, tbase


@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("name", ["2x2x2/nel4", "2x2x2/nel5"])
def test_transforms_alone_against_longdouble(ctx, name, narrow):
    """X^ = U' X, Y = U Y^ and the round trip against numpy.longdouble with the host tables.  Per entry |error| <= 48 * 2^-53 * sum |T| |x|: every output is four
    interleaved chains of at most 12 fused terms and two additions, inside the bound of ONE chain of 48 fused terms (derived, not tuned).  Round trip: the inverse's
    bound on the computed X^, the forward errors carried through |T'|, and the tables' own defect |T' T - I| |X| as longdouble measures it."""
    sub, nel = _shape(ctx, name)
    f, q = _problem(ctx, sub, nel, narrow)
    E = q.E
    assert all(i["narrow"] == bool(narrow) for i in E.orbit_adapted_info(0))
    ngroups, ntot, ld, urel, touched = _layout(ctx, f, q)
    NC, nc = 8 * ngroups, urel.size
    B, tbase = _host_tables(nel, urel)
    if name == "2x2x2/nel4":
        assert any(s % 4 for s in B["orb_size"])  # the zero padding of the sums in fours is exercised
    L = np.longdouble
    x = _seeded(ntot, touched, 11 + nel)
    X = x.reshape(ngroups, ld, 8)[:, :nc, :].transpose(1, 0, 2).reshape(nc, NC)  # (position, column)
    xh, xh_mag = np.zeros((nc, NC), dtype=L), np.zeros((nc, NC), dtype=L)
    tabs = []
    for o, s in enumerate(B["orb_size"]):
        r0 = tbase[o]
        T, pos = B["table"][r0:r0 + s, :s].astype(L), B["orb_pos"][r0:r0 + s]
        tabs.append((r0, s, T, pos))
        xh[r0:r0 + s] = T @ X[pos].astype(L)
        xh_mag[r0:r0 + s] = np.abs(T) @ np.abs(X[pos]).astype(L)
    xv, xhv = ctx.vec_from(x), ctx.vec(nc * NC)
    E.orbit_adapted_transform(0, False, xv, xhv)
    got = xhv.to_numpy().reshape(nc, NC)
    err = np.abs(got.astype(L) - xh)
    print("forward transform %s narrow %d: max error / bound %.3f" % (name, narrow, float(np.max(err / np.maximum(48 * U * xh_mag, np.finfo(float).tiny)))))
    assert np.all(err <= 48 * U * xh_mag) and np.any(got)

    yh = np.random.default_rng(13 + nel).standard_normal((nc, NC))
    Y, Ymag, back, back_b = (np.zeros((nc, NC), dtype=L) for _ in range(4))
    for r0, s, T, pos in tabs:
        Y[pos] = T.T @ yh[r0:r0 + s].astype(L)
        Ymag[pos] = np.abs(T.T) @ np.abs(yh[r0:r0 + s]).astype(L)
        back[pos] = X[pos].astype(L)
        back_b[pos] = (48 * U * (np.abs(T.T) @ np.abs(got[r0:r0 + s]).astype(L) + np.abs(T.T) @ xh_mag[r0:r0 + s])
                       + np.abs(T.T @ T - np.eye(s, dtype=L)) @ np.abs(X[pos]).astype(L))
    tmask = touched.reshape(ngroups, ld, 8)[:, :nc, :].transpose(1, 0, 2).reshape(nc, NC)

    def inverse(a):
        yv = ctx.vec(ntot)
        E.orbit_adapted_transform(0, True, ctx.vec_from(np.ascontiguousarray(a).ravel()), yv)
        y = yv.to_numpy()
        assert not np.any(y[~touched])
        return y.reshape(ngroups, ld, 8)[:, :nc, :].transpose(1, 0, 2).reshape(nc, NC)

    goty = inverse(yh)
    erry = np.abs(goty.astype(L) - Y)
    print("inverse transform %s narrow %d: max error / bound %.3f" % (name, narrow, float(np.max(erry[tmask] / (48 * U * Ymag[tmask])))))
    assert np.all(erry[tmask] <= 48 * U * Ymag[tmask]) and np.any(goty)
    rt = inverse(got)
    errb = np.abs(rt.astype(L) - back)
    print("round trip %s narrow %d: max error / bound %.3f" % (name, narrow, float(np.max(errb[tmask] / np.maximum(back_b[tmask], np.finfo(float).tiny)))))
    assert np.all(errb[tmask] <= back_b[tmask])
