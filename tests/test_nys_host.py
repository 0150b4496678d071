"""Host tests of the Nystroem map (permon_amd/nystroem.py): the set-up against the restatement of tests/nys_cases.py and against the exact kernel matrices, the
rank-deficient paths (polynomial kernels, n_components, a repeated landmark), the refusals that need no device, and the ctypes argument lists against
include/permon_hip.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import permon_amd as pa
from permon_amd import _lib, nystroem
import nys_cases as N
import rff_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rings():
    c = N.RINGS
    return R.rings(c["n_train"], c["seed_train"])[0], R.rings(c["n_test"], c["seed_test"])[0]


def test_set_up_is_the_restatement():
    X = R.density_points()
    L = nystroem.sample_landmarks(X, 20, 3)
    assert np.array_equal(L, N.landmarks(X, 20, 3))
    for kw in (dict(kernel="rbf", gamma=0.25), dict(kernel="poly", gamma=0.5, coef0=1.0, degree=3)):
        np.testing.assert_allclose(nystroem.gram(X, L, **kw), N.gram(X, L, **kw), rtol=8 * 2.0 ** -52, atol=0)  # (numpy's integer power against repeated products)
        M, lam = nystroem.whitening(L, **kw)
        Mr, lamr = N.whitening(L, **kw)
        assert M.shape == Mr.shape == (20, lam.size) and (np.diff(lam) <= 0).all() and lam[-1] > 1e-12 * lam[0]
        np.testing.assert_allclose(lam, lamr, rtol=1e-12)
        np.testing.assert_allclose(M @ M.T, Mr @ Mr.T, rtol=0, atol=1e-9 * np.abs(Mr @ Mr.T).max())  # (eigenvectors up to sign: compare K^+ = M M')


def test_features_are_the_projected_kernel():
    """Z Z' = C K_mm^+ C' with 20 of the 40 points as landmarks."""
    X = R.density_points()
    L = N.landmarks(X, 20, 0)
    M, lam = nystroem.whitening(L, "rbf", N.DENSITY_GAMMA)
    assert M.shape == (20, 20)
    Z = N.features(X, L, M, "rbf", N.DENSITY_GAMMA)
    Cb = N.gram(X, L, "rbf", N.DENSITY_GAMMA)
    want = Cb @ np.linalg.pinv(N.gram(L, L, "rbf", N.DENSITY_GAMMA), hermitian=True) @ Cb.T
    err, cap = float(np.abs(Z @ Z.T - want).max()), N.projection_cap(lam, 20)
    print("projected kernel: max error %.3e, cap %.3e (condition %.3e)" % (err, cap, lam[0] / lam[-1]))
    assert err <= cap


def test_all_points_as_landmarks_give_the_kernel():
    X = R.density_points()
    M, lam = nystroem.whitening(X, "rbf", N.DENSITY_GAMMA)
    assert M.shape == (40, 40)
    Z = N.features(X, X, M, "rbf", N.DENSITY_GAMMA)
    err, cap = float(np.abs(Z @ Z.T - N.gram(X, X, "rbf", N.DENSITY_GAMMA)).max()), N.projection_cap(lam, 40)
    print("all points as landmarks: max error %.3e, cap %.3e (condition %.3e)" % (err, cap, lam[0] / lam[-1]))
    assert err <= cap


@pytest.mark.parametrize("m", [8, 32])
def test_polynomial_kernel_has_its_rank(m):
    """Degree 2 in 2 dimensions: the monomials 1, x, y, x^2, x y, y^2 -- D = 6 whatever m is, and the map is then exact on points it has never seen."""
    X, Xt = _rings()
    p = N.RINGS["poly"]
    L = nystroem.sample_landmarks(X, m, N.RINGS["landmark_seed"])
    M, lam = nystroem.whitening(L, "poly", p["gamma"], p["coef0"], p["degree"])
    assert M.shape == (m, p["D"]) and lam.size == p["D"]
    Z = N.features(Xt, L, M, "poly", p["gamma"], p["coef0"], p["degree"])
    K = N.gram(Xt, Xt, "poly", p["gamma"], p["coef0"], p["degree"])
    err = float(np.abs(Z @ Z.T - K).max() / np.abs(K).max())
    print("poly degree 2, m = %d: |Z Z' - K| / max|K| = %.3e, condition %.3e" % (m, err, lam[0] / lam[-1]))
    assert err <= 8.0 * (lam[0] / lam[-1]) * m * 2.0 ** -52  # (projection_cap relative to max|K|)


def test_n_components_truncates():
    X = R.density_points()
    M, lam = nystroem.whitening(X, "rbf", N.DENSITY_GAMMA)
    M7, lam7 = nystroem.whitening(X, "rbf", N.DENSITY_GAMMA, n_components=7)
    assert M7.shape == (40, 7) and np.array_equal(lam7, lam[:7]) and np.array_equal(M7, M[:, :7])
    assert nystroem.whitening(X, "rbf", N.DENSITY_GAMMA, n_components=100)[0].shape == (40, 40)
    with pytest.raises(ValueError):
        nystroem.whitening(X, "rbf", N.DENSITY_GAMMA, n_components=0)


def test_rcond_drops_a_repeated_landmark():
    L = R.density_points()[:12].copy()
    L[7] = L[2]
    M, lam = nystroem.whitening(L, "rbf", N.DENSITY_GAMMA)
    assert M.shape == (12, 11) and lam.size == 11
    assert nystroem.whitening(L, "rbf", N.DENSITY_GAMMA, rcond=0.5)[0].shape[1] < 11


def test_sample_landmarks():
    X = R.density_points()
    a, b = nystroem.sample_landmarks(X, 9, 4), nystroem.sample_landmarks(X, 9, 4)
    assert a.shape == (9, 8) and np.array_equal(a, b) and not np.array_equal(a, nystroem.sample_landmarks(X, 9, 5))
    assert len({tuple(r) for r in a}) == 9 and all(any(np.array_equal(r, x) for x in X) for r in a)  # rows of X, none twice
    assert np.array_equal(np.sort(nystroem.sample_landmarks(X, 40, 0), axis=0), np.sort(X, axis=0))
    with pytest.raises(ValueError):
        nystroem.sample_landmarks(X, 41, 0)
    with pytest.raises(ValueError):
        nystroem.sample_landmarks(X, 0, 0)


def test_refusals():
    X = R.density_points()
    for kw in (dict(kernel="laplacian"), dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(coef0=float("inf")),
               dict(kernel="poly", degree=0), dict(kernel="poly", degree=17), dict(kernel="poly", degree=2.5)):
        with pytest.raises(ValueError):
            nystroem.whitening(X, **kw)
        with pytest.raises(ValueError):
            nystroem.gram(X, X, **kw)
        with pytest.raises(ValueError):
            pa.NystroemMap(None, X, **kw)  # refused before the context is touched
    with pytest.raises(ValueError):
        nystroem.gram(X, X[:, :5])  # another width


def test_sparse_samples_are_refused():
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(TypeError) as e:
        nystroem.sample_landmarks(sp.csr_matrix(np.eye(3)), 2, 0)
    assert "sparse" in str(e.value)
    fmap = object.__new__(pa.NystroemMap)  # the refusal comes before anything of the map is touched
    for call in (fmap.transform, fmap.kernel_block, fmap.arguments, fmap.distances):
        with pytest.raises(TypeError) as e:
            call(sp.csr_matrix(np.eye(3)))
        assert "sparse" in str(e.value) and "toarray()" in str(e.value)


class _Buf:
    """Stands for a device buffer where no device is touched."""
    p = C.c_void_p(64)

    def free(self):
        pass


def test_wrong_width_is_refused():
    fmap = object.__new__(pa.NystroemMap)
    fmap.d, fmap.h = 5, None
    for call in (fmap.transform, fmap.kernel_block, fmap.arguments, fmap.distances):
        with pytest.raises(ValueError) as e:
            call(pa.DeviceSamples(None, 4, 3, np.float64, _Buf()))
        assert "(n, 5)" in str(e.value) and "(n, 3)" in str(e.value)
    with pytest.raises(ValueError):
        fmap.transform(pa.DeviceSamples(None, 4, 5, np.float64, _Buf()), np.int32)
    with pytest.raises(RuntimeError):
        fmap.transform(pa.DeviceSamples(None, 4, 5, np.float64, _Buf()))  # destroyed


def _header_protos():
    txt = open(os.path.join(ROOT, "include", "permon_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(pmh_nys_[a-z_]+)\s*\(([^)]*)\)\s*;", txt)}


def _ctype_of(param):
    param = param.strip()
    if "*" in param or "[" in param:
        return "pointer"
    t = param.rsplit(None, 1)[0].strip()
    return {"pmh_ctx": "pointer", "pmh_nys": "pointer", "int": C.c_int, "long long": C.c_longlong, "double": C.c_double}[t]


def test_ctypes_argument_lists_match_the_header():
    protos = _header_protos()
    assert sorted(protos) == ["pmh_nys_apply", "pmh_nys_create", "pmh_nys_destroy", "pmh_nys_get", "pmh_nys_info", "pmh_nys_kernel", "pmh_nys_set_chunk_rows", "pmh_nys_test_args"]
    for name, params in protos.items():
        assert name in _lib.EXPORTED
        want = [_ctype_of(p) for p in params.split(",")]
        got = _lib._PROTOS[name]
        assert len(got) == len(want), name
        for g, w in zip(got, want):
            if w == "pointer":
                assert g is _lib.vp or issubclass(g, C._Pointer), (name, g)
            else:
                assert g is w, (name, g, w)
    txt = open(os.path.join(ROOT, "include", "permon_hip.h")).read()
    assert re.search(r"enum\s*\{\s*PMH_NYS_RBF\s*=\s*0\s*,\s*PMH_NYS_POLY\s*=\s*1\s*\}", txt)
    assert nystroem.KERNELS == ("rbf", "poly")
