"""The ABI of the SVM penalties (no GPU): the three entries are declared, listed and exported, and pmh_svm_opts keeps its six fields -- the penalties live on
the trained handle, not in the options."""
import ctypes as C
import os
import re

import pytest

from permon_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["pmh_op_svm_dual_set_diag", "pmh_svm_set_penalties", "pmh_svm_get_penalties"]


@pytest.mark.parametrize("name", ENTRIES)
def test_penalty_entries_are_declared_listed_and_exported(name):
    header = open(os.path.join(ROOT, "include", "permon_hip.h")).read()
    assert re.search(r"^int %s\(" % name, header, re.M), "%s is not declared in permon_hip.h" % name
    assert name in _lib.EXPORTED
    lib = C.CDLL(_lib.LIB_PATH)  # (loading needs no GPU)
    assert hasattr(lib, name), "libpermonhip.so does not export %s" % name


def test_svm_opts_keeps_its_fields():
    assert [f[0] for f in _lib.SvmOpts._fields_] == ["loss_type", "C", "bias", "qps", "mpgp", "smalxe"]
