"""Host tests (no GPU) of tests/orbit_cases.py: the cases of tests/test_gpu_orbit_paths.py have the structure they are meant to have, their matrices are what the orbit
operator is defined for (symmetric, invariant, free of zeros wherever invariance allows a non-zero), the integer reference is exact in double precision, and the orbit
formula restated from the representatives' rows alone reproduces W X -- exactly on the integer data, within the derived bound on the real data."""
import numpy as np
import pytest

import orbit_cases as oc

NAMES = list(oc.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_case_structure(name):
    d = oc.data(name)
    for ci, (c, exp) in enumerate(zip(d.cls, d.case.expect)):
        assert len(c["blocks"]) == exp["blocks"]
        if exp.get("n_c") == 0:  # a class none of whose blocks is touched
            assert c["n_c"] == 0 and c["ld"] == 32
            continue
        for key in ("S", "groups", "nsym", "n_c"):
            if key in exp:
                assert c[key] == exp[key], (name, ci, key, c[key])
        reps, rep_of, op_of = oc.orbits(c["pm"])
        if "M" in exp:
            assert exp["M"][0] <= reps.size <= exp["M"][1], (name, ci, reps.size)
        tm, tnw = oc.expected_row_tile(reps.size, c["S"], c["nsym"])
        if "tm" in exp:
            assert tm == exp["tm"]
        assert tnw == exp.get("tnw", 0)
        if "row_tiles" in exp:
            assert (reps.size + tm - 1) // tm == exp["row_tiles"]
        if "nc_mod32" in exp:
            assert c["n_c"] % 32 == 0 and c["ld"] == c["n_c"] + 32
        # operation 0 is the identity, every operation a signed permutation of U_c
        assert np.array_equal(c["pm"][0], np.arange(c["n_c"])) and np.all(c["sg"][0] == 1)
        assert all(np.array_equal(np.sort(p), np.arange(c["n_c"])) for p in c["pm"]) and np.all(np.abs(c["sg"]) == 1)
        # every block's positions lie in U_c; position 0 and position n_c - 1 are touched by some block (a padded gather index that hits a real row shows)
        touched = np.zeros(c["n_c"], dtype=bool)
        for p in c["pos"]:
            assert p.min() >= 0
            touched[p] = True
        if name in ("box8_two_tiles", "cube48_multi_tile", "pair8_tn64", "one_dof", "one_orbit"):
            assert touched[0] and touched[-1]
    if name == "cube48_multi_tile":  # a representative fixed by several operations, one of them with sign -1: a dof on a mirror plane
        c = d.cls[0]
        reps, _, _ = oc.orbits(c["pm"])
        fixed = (c["pm"][:, reps] == reps[None, :])
        assert np.any((fixed.sum(axis=0) > 1) & np.any(fixed & (c["sg"][:, reps] < 0), axis=0))


@pytest.mark.parametrize("name", NAMES)
def test_integer_matrices(name):
    d = oc.data(name)
    for ci, c in enumerate(d.cls):
        if not c["n_c"]:
            continue
        W = d.W(ci)
        assert W.dtype == np.int64 and np.array_equal(W, W.T)
        # W[g i][g j] = s_g(i) s_g(j) W[i][j] for every operation: on all rows, for the largest case on 400 rows drawn per operation (all columns)
        W32, rng = W.astype(np.int32), np.random.default_rng(5)
        for g in range(c["nsym"]):
            p, s = c["pm"][g], c["sg"][g].astype(np.int32)
            rows = np.arange(c["n_c"]) if c["n_c"] <= 1500 else rng.choice(c["n_c"], size=400, replace=False)
            assert np.array_equal(np.take(W32[p[rows]], p, axis=1), W32[rows] * s[rows, None] * s[None, :])
        # free of zeros, except where every invariant symmetric matrix vanishes
        assert np.array_equal(W == 0, oc.forced_zero(c["pm"], c["sg"]))
    xs = d.X()
    assert all(np.all(x != 0) for x in xs)
    _, mag = d.reference(xs)
    assert int(mag.max(initial=0)) < 2 ** 53
    lam = np.random.default_rng(3).integers(-3, 4, size=d.n_lambda)
    assert np.abs(d.F_reference(lam)).max(initial=0) < 2 ** 53


def _columns(d, ci, xs):
    """The class's multivector as a matrix n_c x blocks (zero off every block's own touched positions)."""
    c = d.cls[ci]
    X = np.zeros((c["n_c"], len(c["blocks"])), dtype=xs[c["blocks"][0]].dtype)
    for j, b in enumerate(c["blocks"]):
        X[c["pos"][d.order[b][1]], j] = xs[b]
    return X


@pytest.mark.parametrize("name", NAMES)
def test_orbit_formula_integer(name):
    d = oc.data(name)
    xs = d.X()
    ref, _ = d.reference(xs)
    for ci, c in enumerate(d.cls):
        if not c["n_c"]:
            continue
        X = _columns(d, ci, xs).astype(np.int64)
        Y = oc.orbit_apply(d.W(ci), c["pm"], c["sg"], X)
        assert np.array_equal(Y, d.W(ci) @ X)
        for j, b in enumerate(c["blocks"]):  # and the per-block reference is that product on the block's own positions
            assert np.array_equal(ref[d.index(b)], Y[c["pos"][d.order[b][1]], j])


@pytest.mark.parametrize("name", NAMES)
def test_orbit_formula_real(name):
    d = oc.data(name)
    xs = d.X(real=True)
    worst = 0.0
    for ci, c in enumerate(d.cls):
        if not c["n_c"]:
            continue
        W, X = d.W(ci, real=True), _columns(d, ci, xs)
        assert np.array_equal(W, W.T)
        Y = oc.orbit_apply(W, c["pm"], c["sg"], X)
        ref = W.astype(np.longdouble) @ X.astype(np.longdouble)
        bound = (c["n_c"] + 8) * oc.U53 * (np.abs(W).astype(np.longdouble) @ np.abs(X).astype(np.longdouble))
        err = np.abs(Y.astype(np.longdouble) - ref)
        assert np.all(err <= bound)
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    print("orbit formula, real data, %s: worst err / bound %.3e" % (name, worst))


def test_reference_layout():
    """The multivector numbering xoff + group ld S + position S + slot: blocks never collide, the touched mask counts every touched dof once."""
    for name in NAMES:
        d = oc.data(name)
        idx = np.concatenate([d.index(b) for b in range(d.nblocks)]) if d.nblocks else np.zeros(0, dtype=np.int64)
        assert idx.size == np.unique(idx).size and (not idx.size or (idx.min() >= 0 and idx.max() < d.nX))
        assert int(d.touched_mask().sum()) == idx.size and np.all(d.block_slot_mask()[idx.astype(np.int64)])
