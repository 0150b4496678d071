"""pmh_feti_contact_solve with explicit_dual = PMH_KPLUS_AUTO: the K^+ of F (explicit local dual operators or the inner Krylov solve) chosen by the estimated time to
solution from a short probe.  Two cuts of the same (42 elements)^3 body: the staircase cut of permon_amd.feti.irregular_partition (8 blocks of 21^3 scale that are not boxes:
algebraic hierarchy, one K^+ column per touched dof) and the congruent 2 x 2 x 2 boxes (box hierarchy, the orbit storage of configs[2]).

The rule is checked where it cannot tie: expected_applies = 1 (one F application can never repay a set-up of thousands of K^+ solves) and 1e9 (the set-up is nothing against
1e9 applications that are each several times cheaper).  After the choice the solve runs exactly the forced path, so u, lambda and the SMALXE counters are compared with
np.array_equal against the run forced to that path: the library is deterministic (fixed reduction trees, no atomics on the data path), and the probe's
set-up batch is the one the forced set-up would run first, with the same columns."""
import math

import numpy as np
import pytest

import permon_amd as pa
from permon_amd import feti
from permon_amd.chain import FETIContactSolve

pytestmark = pytest.mark.gpu

NEL = 21  # half the elements per edge: 8 blocks of 21^3 scale


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def runs(ctx):
    cache = {}

    def run(cut, explicit, expected_applies=0.0):
        key = (cut, explicit, expected_applies)
        if key not in cache:
            if cut not in cache:
                cache[cut] = feti.MeshFeti(feti.irregular_partition(NEL, cut), contact=True)
            f = cache[cut]
            kw = dict(dims=None) if cut == "staircase" else dict(dims=[(NEL + 1,) * 3] * 8, explicit_storage="class_orbit")
            cache[key] = FETIContactSolve(ctx, f, explicit=explicit, expected_applies=expected_applies, **kw)
        return cache[key]

    return run


def _smalxe_counters(st):
    s = st.smalxe
    return (s.iteration, s.reason, s.inner_iter_accu, s.M1_hits, s.eta_hits, s.M1_updates, s.rho_updates, s.inner.nmv, s.inner.ncg, s.inner.nexp, s.inner.nprop, st.f_applies, st.n_active)


def _same_solution(a, b):
    ua, la, sa = a
    ub, lb, sb = b
    assert np.array_equal(ua, ub)
    assert np.array_equal(la, lb)
    assert _smalxe_counters(sa) == _smalxe_counters(sb)


def _check_auto_stats(st, expected_applies, forced_explicit):
    assert st.kplus_auto == 1
    assert st.expected_applies_used == expected_applies
    for v in (st.est_explicit_seconds, st.est_iterative_seconds, st.probe_seconds):
        assert math.isfinite(v) and v > 0.0
    assert st.probe_seconds <= st.setup_seconds
    assert st.setup_solves_planned == forced_explicit.explicit_solves  # the probe plans the set-up exactly as the explicit path runs it
    assert (st.est_explicit_seconds < st.est_iterative_seconds) == (st.kplus_path == 1)  # the stated rule, on the numbers it reports


@pytest.mark.parametrize("cut", ["staircase", "cubes"])
def test_forced_choices_and_same_result_as_the_forced_path(runs, cut):
    exp, it = runs(cut, True), runs(cut, False)
    assert exp[2].smalxe.reason > 0 and it[2].smalxe.reason > 0
    assert exp[2].kplus_path == 1 and it[2].kplus_path == 0
    assert exp[2].explicit_solves > 0 and it[2].explicit_solves == 0
    # one F application: the inner Krylov path
    a1 = runs(cut, "auto", 1.0)
    assert a1[2].kplus_path == 0
    _check_auto_stats(a1[2], 1.0, exp[2])
    assert a1[2].explicit_solves == 0 and a1[2].explicit_symmetries == 0
    _same_solution(a1, it)
    # 1e9 F applications: the explicit path, its set-up completed from the probe's first batch
    a9 = runs(cut, "auto", 1e9)
    assert a9[2].kplus_path == 1
    _check_auto_stats(a9[2], 1e9, exp[2])
    assert a9[2].explicit_solves == exp[2].explicit_solves and a9[2].explicit_symmetries == exp[2].explicit_symmetries
    _same_solution(a9, exp)


def test_box_cut_default_expected_applies_picks_explicit(runs):
    """configs[2]'s shape: 715-ish orbit representatives per class make the set-up cheap, the orbit GEMM makes every application cheap."""
    a0 = runs("cubes", "auto", 0.0)
    assert a0[2].kplus_path == 1 and a0[2].explicit_symmetries == 48
    _check_auto_stats(a0[2], float(_default_applies()), runs("cubes", True)[2])
    _same_solution(a0, runs("cubes", True))


def test_default_options_unchanged(runs):
    """explicit_dual keeps its default 1: the explicit path, no probe."""
    for cut in ("staircase", "cubes"):
        st = runs(cut, True)[2]
        assert st.kplus_path == 1 and st.kplus_auto == 0
        assert st.probe_seconds == 0.0 and st.est_explicit_seconds == 0.0 and st.est_iterative_seconds == 0.0
        assert st.setup_solves_planned == st.explicit_solves and st.f_applies > 0


def _default_applies():
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "permon_hip.h")).read()
    return int(re.search(r"#define PMH_KPLUS_AUTO_DEFAULT_APPLIES (\d+)", hdr).group(1))
