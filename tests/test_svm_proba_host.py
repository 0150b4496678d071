"""The SVM probability model without a GPU: the ABI (every new entry is declared, listed and exported), and that the numpy restatement of the Platt fit
converges, with a Hessian bounded away from singular, on every instance the GPU tests compare the device against."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import svm_proba_cases as PC
from permon_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["pmh_svm_platt_fit", "pmh_svm_calibrate", "pmh_svm_calibrate_csr", "pmh_svm_set_calibration", "pmh_svm_get_calibration", "pmh_svm_predict_proba",
           "pmh_svm_predict_proba_csr", "pmh_svm_multi_calibrate", "pmh_svm_multi_calibrate_csr", "pmh_svm_multi_set_calibration", "pmh_svm_multi_get_calibration",
           "pmh_svm_multi_predict_proba", "pmh_svm_multi_predict_proba_csr"]


@pytest.mark.parametrize("name", ENTRIES)
def test_proba_entries_are_declared_listed_and_exported(name):
    header = open(os.path.join(ROOT, "include", "permon_hip.h")).read()
    assert re.search(r"^int %s\(" % name, header, re.M), "%s is not declared in permon_hip.h" % name
    assert name in _lib.EXPORTED
    lib = C.CDLL(_lib.LIB_PATH)  # (loading needs no GPU)
    assert hasattr(lib, name), "libpermonhip.so does not export %s" % name


def test_platt_stats_layout_matches_the_header():
    """The ctypes mirror has the header's fields in the header's order."""
    header = open(os.path.join(ROOT, "include", "permon_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pmh_svm_platt_stats;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].replace("long ", "").split(",")]
    assert names == [f[0] for f in _lib.SvmPlattStats._fields_]
    assert C.sizeof(_lib.SvmPlattStats) == 56


@pytest.mark.parametrize("inst", PC.INSTANCES)
def test_numpy_fit_converges_on_the_instances(inst):
    f, y = PC.scores(*inst)
    r = PC.platt_np(f, y)
    print("platt_np", inst, r)
    assert r["reason"] == PC.CONVERGED and r["iterations"] <= 100
    assert r["lambda_min"] > 1.0
    # what the issue recorded for these instances
    assert r["iterations"] == PC.ITERATIONS[inst]
    assert abs(r["lambda_min"] - PC.LAMBDA_MIN[inst]) <= 0.01 * PC.LAMBDA_MIN[inst] + 0.05
    # the returned point is stationary for the restatement's own sums, and A < 0: the probability of +1 grows with the score
    t, n_pos, n_neg = PC.targets(y)
    assert n_pos + n_neg == inst[0] and n_pos == int((y > 0).sum())
    h = PC.sums(f, t, r["A"], r["B"])
    assert abs(h[1]) < 1e-5 and abs(h[2]) < 1e-5 and r["A"] < 0.0


def test_numpy_fit_edge_cases():
    # one class: the start point is stationary
    y = np.ones(50)
    r = PC.platt_np(np.linspace(-1.0, 2.0, 50), y)
    assert r["reason"] == PC.CONVERGED and r["iterations"] == 0 and r["A"] == 0.0 and abs(r["B"] - np.log(1.0 / 51.0)) <= 1e-12
    # separable: A runs off, the point stays finite
    f, y = PC.separable_scores()
    r = PC.platt_np(f, y)
    assert np.isfinite(r["A"]) and np.isfinite(r["B"]) and r["A"] < 0.0 and r["reason"] in (PC.CONVERGED, PC.MAX_IT, PC.LINE_SEARCH)


def test_sigma_is_stable():
    z = np.array([-800.0, -40.0, 0.0, 40.0, 800.0])
    s = PC.sigma(z)
    assert np.isfinite(s).all() and s[0] == 1.0 and s[2] == 0.5 and s[4] == 0.0 and (np.diff(s) <= 0.0).all()


@pytest.mark.parametrize("case", PC.MULTI)
def test_numpy_fit_converges_on_every_column_of_the_multiclass_cases(case):
    """The blobs overlap: no class is separable from the rest by the model's scores, so each of the K fits the GPU test compares bit for bit converges."""
    X, labels, W, b = PC.multi_case(*case)
    S = np.asarray(X @ W.T) + b
    for k in range(case[0]):
        r = PC.platt_np(S[:, k], np.where(labels == k, 1.0, -1.0))
        assert r["reason"] == PC.CONVERGED and r["lambda_min"] > 1e-3, (case, k, r)
