"""CPU check of the ABI that the automatic K^+ choice of pmh_feti_contact_solve added: the ctypes mirrors of pmh_feti_contact_opts / pmh_feti_contact_stats
against the public header compiled with gcc (size and the offset of every field), and the value of PMH_KPLUS_AUTO as the Python wrapper passes it."""
import ctypes
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_feti_contact_opts_layout_matches_header():
    from permon_amd import _lib

    fields = [name for name, _ in _lib.FetiContactOpts._fields_]
    assert fields[-1] == "expected_applies"  # appended, nothing reordered
    assert _py_layout(_lib.FetiContactOpts) == _c_layout("pmh_feti_contact_opts", fields)


def test_feti_contact_stats_layout_matches_header():
    from permon_amd import _lib

    fields = [name for name, _ in _lib.FetiContactStats._fields_]
    assert fields[:11] == ["smalxe", "n_lambda", "n_eq", "coarse_dim", "n_active", "explicit_solves", "setup_seconds", "solve_seconds", "explicit_seconds",
                           "norm_Glambda_minus_e", "explicit_symmetries"]  # the fields before the automatic choice keep their places
    assert fields[11:] == ["kplus_path", "kplus_auto", "setup_solves_planned", "expected_applies_used", "est_explicit_seconds", "est_iterative_seconds",
                           "probe_seconds", "f_applies"]
    assert _py_layout(_lib.FetiContactStats) == _c_layout("pmh_feti_contact_stats", fields)


def test_kplus_auto_constants():
    from permon_amd import chain

    got = _c_layout("pmh_feti_contact_opts", [], extra='printf("%d %d", PMH_KPLUS_AUTO, PMH_KPLUS_AUTO_DEFAULT_APPLIES);')
    assert got[1] == chain.PMH_KPLUS_AUTO and got[2] > 0
