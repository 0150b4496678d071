"""Host tests of the scoring on unstored random Fourier features (permon_amd/rff.py lazy / dots, include/permon_hip.h): the derived bound of
tests/rff_score_cases.py holds for plain fp64 numpy against the long-double reference on every shape the GPU tests use -- so it tests the kernel, not the
yardstick -- MappedSamples needs no device for its argument checks, and the new entries are declared alike in the header and the ctypes table."""
import os
import re

import numpy as np
import pytest

import permon_amd as pa
from permon_amd import _lib
from permon_amd.svm import _Samples
import rff_score_cases as S
import rff_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,d,D", S.SCORE_SHAPES)
def test_numpy_is_inside_the_derived_bound(n, d, D):
    X, omega, beta = S.real_case(n, d, D, n + d + D)
    scale = np.sqrt(2.0 / D)
    W = S.real_weights(S.SCORE_K, D, 31 * D + d)
    ref, Z, T = S.dots_longdouble(X, omega, beta, scale, W)
    bound = S.dots_bound(X, omega, beta, scale, W)
    got = R.features(X, omega, beta, scale) @ W.T
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    print("(%d, %d, %d): max |dot| %.2f, max error %.2e, max error / bound %.3f, smallest bound %.2e" % (n, d, D, np.abs(got).max(), err.max(), (err / bound).max(), bound.min()))
    assert ref.shape == bound.shape == (n, S.SCORE_K) and (bound > 0).all()
    assert (err <= bound).all()
    assert bound.max() <= 1e-9 * max(1.0, float(np.abs(ref).max()))  # and the bound says something: nine digits of the largest dot product


def test_padded_columns_are_not_zero_features():
    """What test 2 on the GPU can catch and test 1 cannot: with beta and the arguments 0 a padded column's feature is s, so a kernel that summed it would be off
    by s times whatever weight it read."""
    assert R.features(np.zeros((1, 3)), np.zeros((3, 2)), np.zeros(2), 0.5).tolist() == [[0.5, 0.5]]


def test_chunk_counts_and_weights():
    assert S.chunk_counts(4) == [1, 3, 4, 5, 9] and S.chunk_counts(2) == [1, 2, 3, 5] and S.chunk_counts(1) == [1, 2, 3]
    W = S.int_weights(9, 257, 3)
    assert W.shape == (9, 257) and np.abs(W).max() == 8 and (W == np.round(W)).all()
    lab = S.radius_classes(S.rings(400, 1)[0])
    assert sorted(set(lab.tolist())) == [0.0, 1.0, 2.0] and min(np.bincount(lab.astype(int))) >= 20


class _Buf:
    p = object()

    def free(self):
        self.freed = True


class _Map:
    d, D, h = 3, 8, object()

    def _need(self):
        pass


def test_mapped_samples_without_a_device():
    src = pa.DeviceSamples(None, 5, 3, np.float32, _Buf())
    M = pa.MappedSamples(_Map(), src, owned=False)
    assert (M.n, M.d, M.shape, M.ndim) == (5, 8, (5, 8), 2) and M.map.D == 8 and M.source is src
    assert M.entry_args() == (_Map.h, 5, src.p, 1)  # PMH_F32: the source's own type, whatever a handle's sample_dtype is
    T = _Samples(None, M, dtype=np.float64)
    assert T.mapped and T.suffix == "_rff" and not T.f32 and not T.sparse and T.X is M
    with T as (n, xa):
        assert n == 5 and xa == M.entry_args()
    assert _Samples(None, M, dtype=np.float32).suffix == "_rff"
    with pytest.raises(TypeError) as e:
        _Samples(None, M, with_d=True)  # training samples
    assert "transform" in str(e.value)
    for train in (lambda: pa.MatCreateSVMDual(None, M, np.ones(5)), lambda: pa.MatCreateSVRDual(None, M)):
        with pytest.raises(TypeError) as e:
            train()
        assert "transform" in str(e.value)
    M.free()
    assert M.source is None and src.buf is not None  # not owned: the caller's samples stay
    with pytest.raises(RuntimeError):
        M.entry_args()
    own = pa.MappedSamples(_Map(), pa.DeviceSamples(None, 5, 3, np.float64, _Buf()), owned=True)
    assert own.entry_args()[3] == 0
    s = own.source
    own.free()
    assert s.buf is None
    with pytest.raises(ValueError) as e:
        pa.MappedSamples(_Map(), pa.DeviceSamples(None, 5, 4, np.float64, _Buf()), owned=False)
    assert "3" in str(e.value) and "4" in str(e.value)


NEW = ["pmh_rffdots", "pmh_rffdots_test_args"] + ["pmh_%s_%s_rff" % (h, e) for h, es in (("svm", ("predict", "test", "predict_proba", "calibrate")),
                                                                                             ("svm_multi", ("predict", "test", "predict_proba", "calibrate")),
                                                                                             ("svr", ("predict", "test"))) for e in es]


def test_new_entries_are_declared_alike():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "permon_hip.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        got = _lib._PROTOS[name]
        assert name in _lib.EXPORTED and len(got) == len(params), name
        for g, p in zip(got, params):
            if "*" in p or "[" in p or p.split()[0] in ("pmh_rff", "pmh_svm", "pmh_svm_multi", "pmh_svr"):
                assert g is _lib.vp or issubclass(g, _lib.C._Pointer), (name, p, g)
            else:
                assert g is {"int": _lib.C.c_int, "long long": _lib.C.c_longlong}[p.rsplit(None, 1)[0]], (name, p, g)
    # the front ends' entries: the dense twin's arguments with (map, n, X_dev, x_type) where it has (n, X_dev)
    for name in NEW[2:]:
        twin = _lib._PROTOS[name[:-len("_rff")]]
        assert _lib._PROTOS[name] == [twin[0], _lib.vp, twin[1], twin[2], _lib.C.c_int] + twin[3:], name
    assert pa.rff.INFO[6:] == ("classes_per_chunk", "dots_lds_bytes")
