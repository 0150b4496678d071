"""Host tests (no GPU) of the symmetry-adapted basis of the cube's boundary dofs (orbitbasis.hip, pmh_orbit_basis): cubes of 5 nodes per edge (odd: nodes on the symmetry
planes, small orbits, sign characters of -1) and 6 (even)."""
import numpy as np
import pytest

from permon_amd.feti import box_symmetries
from permon_amd.mat import orbit_basis

IRREPS = ("A1g", "A2g", "Eg", "T1g", "T2g", "A1u", "A2u", "Eu", "T1u", "T2u")


def _characters(axes, flips):
    """The ten characters of the operation `new coordinate a = flips[a] * old coordinate axes[a]`, restated: delta = det, eps = sign of the permutation, R = delta M."""
    M = np.zeros((3, 3))
    for a in range(3):
        M[a, axes[a]] = flips[a]
    delta = round(np.linalg.det(M))
    eps = round(np.linalg.det(np.abs(M)))
    trR = delta * np.trace(M)
    h = np.sqrt(3.0) / 2.0
    B = np.array([[1.0, 0.0], [-0.5, h], [-0.5, -h]])
    trE = np.trace(np.linalg.pinv(B) @ np.abs(M) @ B)
    even = np.array([1.0, eps, trE, trR, eps * trR])
    return np.concatenate([even, delta * even])


def _setup(N):
    nodes = np.arange(N ** 3)
    i, j, k = nodes % N, (nodes // N) % N, nodes // (N * N)
    surf = (i == 0) | (i == N - 1) | (j == 0) | (j == N - 1) | (k == 0) | (k == N - 1)
    rel = (np.nonzero(surf)[0][:, None] * 3 + np.arange(3)).ravel()
    n = rel.size
    b = orbit_basis((N, N, N), 3, rel)
    perm, sign = box_symmetries((N, N, N), 3)
    assert perm.shape[0] == 48
    pos = -np.ones(3 * N ** 3, dtype=np.int64)
    pos[rel] = np.arange(n)
    pm = pos[perm[:, rel]]
    sg = sign[:, rel].astype(float)
    tb = np.concatenate([[0], np.cumsum(b["orb_size"])])
    U = np.zeros((n, n))
    for o, no in enumerate(b["orb_size"]):
        for t in range(tb[o], tb[o] + no):
            U[t, b["orb_pos"][tb[o]:tb[o] + no]] = b["table"][t, :no]
    return dict(n=n, rel=rel, b=b, pm=pm, sg=sg, tb=tb, U=U, N=N)


@pytest.fixture(scope="module", params=[5, 6])
def cube(request):
    return _setup(request.param)


def test_multiplicities_against_characters(cube):
    """m_i = (1 / 48) sum_g chi_i(g) chi_perm(g) with chi_perm(g) = sum of the signs of the dofs g fixes; the operations rebuilt here from their action on a generic node."""
    N, n, b, pm, sg = cube["N"], cube["n"], cube["b"], cube["pm"], cube["sg"]
    import itertools

    ops = [(ax, fl) for ax in itertools.permutations(range(3)) for fl in itertools.product((1, -1), repeat=3)]
    perm, sign = box_symmetries((N, N, N), 3)
    node = 1 + N * (2 + N * 0)  # (1, 2, 0): its images tell all 48 operations apart
    mult = np.zeros(10)
    found = set()
    for g in range(48):
        for ax, fl in ops:
            old = (1, 2, 0)
            nw = [(N - 1 - old[ax[a]]) if fl[a] < 0 else old[ax[a]] for a in range(3)]
            node2 = nw[0] + N * (nw[1] + N * nw[2])
            if all(perm[g, node * 3 + ax[a]] == node2 * 3 + a and sign[g, node * 3 + ax[a]] == fl[a] for a in range(3)):
                found.add((ax, fl))
                chi_perm = float(np.sum(sg[g][pm[g] == np.arange(n)]))
                mult += _characters(ax, fl) * chi_perm / 48.0
                break
    assert len(found) == 48
    assert np.allclose(mult, np.round(mult), atol=1e-9)
    assert np.array_equal(np.round(mult).astype(int), b["mult"]), dict(zip(IRREPS, b["mult"]))
    assert np.array_equal(b["dim"], [1, 1, 2, 3, 3, 1, 1, 2, 3, 3]) and int(np.sum(b["mult"] * b["dim"])) == n
    if N == 5:
        assert n == 294 and len(b["orb_size"]) == 12 and np.all(b["mult"] > 0)


def test_tables_orthonormal(cube):
    U, n = cube["U"], cube["n"]
    assert np.abs(U @ U.T - np.eye(n)).max() <= 1e-13


def test_block_structure_and_setup_formula(cube):
    """A random symmetric matrix averaged over the group: U W U' is zero off the predicted blocks, the d partner blocks of an irrep are equal, and the set-up formula
    W^_i[(P,k),(C,l)] = sqrt(|O_P| / d) sum_b v_{P,k}[b] <phi_{C,l,b}, W[p, :]> from the representatives' rows alone reproduces them."""
    n, b, pm, sg, tb, U = cube["n"], cube["b"], cube["pm"], cube["sg"], cube["tb"], cube["U"]
    A = np.random.default_rng(0).standard_normal((n, n))
    A = A + A.T
    W = np.zeros((n, n))
    for g in range(48):
        Wg = np.zeros((n, n))
        Wg[np.ix_(pm[g], pm[g])] = A * np.outer(sg[g], sg[g])
        W += Wg / 48.0
    H = U @ W @ U.T
    scale = np.abs(H).max()
    same = (b["irrep"][:, None] == b["irrep"][None, :]) & (b["partner"][:, None] == b["partner"][None, :])
    assert np.abs(H[~same]).max() <= 1e-13 * scale
    orb_of = np.repeat(np.arange(len(b["orb_size"])), b["orb_size"])
    What = U @ W  # column p: the forward transform of row p
    for ir in range(10):
        d, m = int(b["dim"][ir]), int(b["mult"][ir])
        if m == 0:
            continue
        blocks = []
        for a in range(d):
            idx = np.nonzero((b["irrep"] == ir) & (b["partner"] == a))[0]
            idx = idx[np.argsort(b["index"][idx])]
            assert np.array_equal(b["index"][idx], np.arange(m))
            blocks.append(H[np.ix_(idx, idx)])
        for a in range(1, d):
            assert np.abs(blocks[a] - blocks[0]).max() <= 1e-13 * scale
        idx0 = np.nonzero((b["irrep"] == ir) & (b["partner"] == 0))[0]
        idx0 = idx0[np.argsort(b["index"][idx0])]
        F = np.zeros((m, m))
        for r, fr in enumerate(idx0):
            o = orb_of[fr]
            p = b["orb_pos"][tb[o]]  # the orbit's representative: its first position
            for bb in range(d):
                F[r, :] += np.sqrt(b["orb_size"][o] / d) * b["v"][fr, bb] * What[idx0 + bb, p]
        assert np.abs(F - blocks[0]).max() <= 1e-13 * scale


def test_not_closed_is_refused():
    from permon_amd._lib import PermonHipError

    with pytest.raises(PermonHipError, match="closed"):
        orbit_basis((5, 5, 5), 3, np.arange(6))
