"""CPU checks of the SVM front end's ABI (pmh_svm_*, pmh_qppf_create_onerow): the entries are in the header, in _lib.py and exported by the built library; the ctypes
mirrors of pmh_svm_opts / pmh_svm_stats match the header compiled with gcc (size and the offset of every field); option strings parse into pmh_svm_opts."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["pmh_svm_default_opts", "pmh_svm_set_from_options", "pmh_svm_create", "pmh_svm_train", "pmh_svm_get_model", "pmh_svm_get_dual", "pmh_svm_get_stats",
           "pmh_svm_get_solver", "pmh_svm_predict", "pmh_svm_test", "pmh_svm_destroy", "pmh_qppf_create_onerow", "pmh_op_svm_dual_set_terms"]


def _c_layout(struct, fields, extra=""):
    body = " ".join('printf("%%zu ", offsetof(%s, %s));' % (struct, f) for f in fields)
    src = "#include <stddef.h>\n#include <stdio.h>\n#include \"permon_hip.h\"\nint main(void){ printf(\"%%zu \", sizeof(%s)); %s %s return 0; }\n" % (struct, body, extra)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        with open(c, "w") as fh:
            fh.write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        return list(map(int, subprocess.check_output([exe]).split()))


def _py_layout(cls):
    return [ctypes.sizeof(cls)] + [getattr(cls, name).offset for name, _ in cls._fields_]


def test_entries_declared_in_header_lib_and_library():
    from permon_amd import _lib

    header = open(os.path.join(ROOT, "include", "permon_hip.h")).read()
    L = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name + " is not declared in include/permon_hip.h"
        assert name in _lib.EXPORTED, name + " is not declared in permon_amd/_lib.py"
        assert hasattr(L, name), name + " is not exported by libpermonhip.so"


def test_svm_opts_layout_matches_header():
    from permon_amd import _lib

    fields = [name for name, _ in _lib.SvmOpts._fields_]
    assert fields == ["loss_type", "C", "bias", "qps", "mpgp", "smalxe"]
    assert _py_layout(_lib.SvmOpts) == _c_layout("pmh_svm_opts", fields)


def test_svm_stats_layout_matches_header():
    from permon_amd import _lib

    fields = [name for name, _ in _lib.SvmStats._fields_]
    assert _py_layout(_lib.SvmStats) == _c_layout("pmh_svm_stats", fields)
    got = _c_layout("pmh_svm_stats", [], extra='printf("%d %d", PMH_SVM_LOSS_L1, PMH_SVM_LOSS_L2);')
    assert got[1:] == [0, 1]


def _parse(s):
    from permon_amd import _lib

    L = _lib.load()
    o = _lib.SvmOpts()
    assert L.pmh_svm_default_opts(o) == 0
    left = ctypes.create_string_buffer(512)
    rc = L.pmh_svm_set_from_options(s.encode(), o, left, len(left))
    return rc, o, left.value.decode().split(), L.pmh_last_error().decode()


def test_defaults():
    rc, o, left, _ = _parse("")
    assert rc == 0 and left == []
    assert (o.loss_type, o.C, o.bias) == (0, 1.0, 1)
    assert (o.qps.rtol, o.qps.max_it, o.smalxe.max_it, o.smalxe.rho_user, o.mpgp.gamma) == (1e-5, 10000, 100, 1.1, 1.0)


def test_option_strings_parse_into_svm_opts():
    rc, o, left, _ = _parse("-svm_loss_type L2 -svm_C 2.5 -svm_bias 0 -qps_rtol 1e-6 -qps_max_it 77 -qps_mpgp_gamma 2 -qps_smalxe_rho 3 -smalxe_qps_mpgp_gamma 4 -not_ours 1")
    assert rc == 0
    assert (o.loss_type, o.C, o.bias) == (1, 2.5, 0)
    assert (o.qps.rtol, o.qps.max_it, o.qps.max_it_set) == (1e-6, 77, 1)
    assert o.mpgp.gamma == 2.0 and o.smalxe.rho_user == 3.0 and o.smalxe.inner.gamma == 4.0  # passed through to the QPS parser unchanged
    assert left == ["-not_ours"]  # reported, not an error (PETSc's -options_left)
    rc, o, _, _ = _parse("-svm_loss_type l1 -svm_bias true")
    assert rc == 0 and (o.loss_type, o.bias) == (0, 1)


@pytest.mark.parametrize("s,word", [("-svm_loss_type hinge", "hinge"), ("-svm_loss_type", "needs a value"), ("-svm_C -1", "positive"), ("-svm_C 0", "positive")])
def test_bad_values_are_errors_with_a_message(s, word):
    rc, _, _, msg = _parse(s)
    assert rc != 0 and word in msg, (rc, msg)


def test_python_front_end_is_exported():
    import permon_amd as pa
    from permon_amd import problems as P

    assert pa.SVM.__module__ == "permon_amd.svm" and hasattr(pa.QPPF, "onerow")
    p = P.svm_offset(200, 8, 2.0, N_test=50)
    q = P.svm_dual(200, 8)
    assert (p["X"] == q["X"]).all() and p["X_test"].shape == (50, 8) and set(p["y"]) == {-1.0, 1.0}
    assert (p["y"] != q["y"]).any() and (p["y"] == 1).mean() > (q["y"] == 1).mean()  # the planted offset moves labels to +1
