"""Host tests of the random Fourier feature map (permon_amd/rff.py): the draw against the exact Gram matrices, the restatement of tests/rff_cases.py against the
product's draw, the refusals that need no device, and the ctypes argument lists against include/permon_hip.h."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import permon_amd as pa
from permon_amd import _lib, rff
from permon_amd.svm import _Samples
import rff_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kernel", ["rbf", "laplacian"])
def test_spectral_density(kernel):
    """Z Z' of D = 4096 features is within 5 / sqrt(D) of the exact Gram matrix (checked on the CPU: rbf 0.040, 0.042, 0.038 and laplacian 0.057, 0.043, 0.053 for
    seeds 0 .. 2); drawn with variance gamma in place of 2 gamma the rbf features are off by 0.28 on these points."""
    X = R.density_points()
    omega, beta, scale = rff.draw(X.shape[1], R.DENSITY_D, R.DENSITY_GAMMA, kernel, R.DENSITY_SEED)
    err = float(np.abs(R.features(X, omega, beta, scale) @ R.features(X, omega, beta, scale).T - R.gram(X, R.DENSITY_GAMMA, kernel)).max())
    print("spectral density %s: max error %.4f, cap %.4f" % (kernel, err, R.DENSITY_CAP))
    assert err <= R.DENSITY_CAP
    if kernel == "rbf":
        wrong = rff.draw(X.shape[1], R.DENSITY_D, R.DENSITY_GAMMA / 2.0, kernel, R.DENSITY_SEED)  # Omega = sqrt(gamma) N(0, 1): the classic mistake
        assert float(np.abs(R.features(X, *wrong) @ R.features(X, *wrong).T - R.gram(X, R.DENSITY_GAMMA, kernel)).max()) > 2.0 * R.DENSITY_CAP


@pytest.mark.parametrize("kernel", ["rbf", "laplacian"])
def test_draw_is_the_restatement(kernel):
    got, exp = rff.draw(5, 33, 0.7, kernel, 3), R.draw(5, 33, 0.7, kernel, 3)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and got[2] == exp[2] == math.sqrt(2.0 / 33)
    assert got[0].shape == (5, 33) and got[1].shape == (33,) and (got[1] >= 0.0).all() and (got[1] < 2.0 * math.pi).all()


def test_draw_refusals():
    for kw in (dict(kernel="poly"), dict(d=0), dict(D=0), dict(gamma=0.0), dict(gamma=float("nan"))):
        with pytest.raises(ValueError):
            rff.draw(**dict(dict(d=3, D=8, gamma=1.0, kernel="rbf", seed=0), **kw))


class _Buf:
    """Stands for a device buffer where no device is touched."""
    p = C.c_void_p(64)

    def free(self):
        pass


def test_device_samples_dtype_mismatch_is_refused():
    for have, want in ((np.float32, np.float64), (np.float64, np.float32)):
        Z = pa.DeviceSamples(None, 5, 3, have, _Buf())
        assert Z.shape == (5, 3) and np.ndim(Z) == 2 and Z.dtype == have
        with pytest.raises(ValueError) as e:
            _Samples(None, Z, dtype=want)
        assert "float32" in str(e.value) and "float64" in str(e.value)
        S = _Samples(None, Z, with_d=True, dtype=have)  # the matching type: entering uploads nothing, leaving frees nothing
        with S as (n, xa):
            assert n == 5 and xa[:2] == (5, 3) and xa[2] is Z.p
            kept = S.keep()
        assert kept.samples is Z and Z.buf is not None
        kept.free()
        assert Z.buf is not None  # the handle's reference goes, the caller's buffer stays
    with pytest.raises(ValueError):
        pa.DeviceSamples(None, 5, 3, np.int32, _Buf())
    Z = pa.DeviceSamples(None, 5, 3, np.float64, _Buf())
    Z.free()
    with pytest.raises(RuntimeError):
        Z.p


def test_sparse_samples_are_refused_by_the_map():
    sp = pytest.importorskip("scipy.sparse")
    fmap = object.__new__(pa.RFFMap)  # the refusal comes before anything of the map is touched
    with pytest.raises(TypeError) as e:
        fmap.transform(sp.csr_matrix(np.eye(3)))
    assert "sparse" in str(e.value)


def _header_protos():
    txt = open(os.path.join(ROOT, "include", "permon_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(pmh_rff_[a-z_]+)\s*\(([^)]*)\)\s*;", txt)}


def _ctype_of(param):
    param = param.strip()
    if "*" in param or "[" in param:
        return "pointer"
    t = param.rsplit(None, 1)[0].strip()
    return {"pmh_ctx": "pointer", "pmh_rff": "pointer", "int": C.c_int, "long long": C.c_longlong, "double": C.c_double}[t]


def test_ctypes_argument_lists_match_the_header():
    protos = _header_protos()
    assert sorted(protos) == ["pmh_rff_apply", "pmh_rff_create", "pmh_rff_destroy", "pmh_rff_get", "pmh_rff_info", "pmh_rff_test_args"]
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
    assert re.search(r"enum\s*\{\s*PMH_F64\s*=\s*0\s*,\s*PMH_F32\s*=\s*1\s*\}", txt)
    assert rff.TYPE_CODES == {np.dtype(np.float64): 0, np.dtype(np.float32): 1}
