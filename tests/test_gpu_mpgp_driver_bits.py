"""The fused MPGP driver under SMALXE computes, bit for bit, what tests/golden/mpgp_driver_bits.json recorded: per inner solve the step string, the monitor's norms
and nmv / ncg / nexp / nprop, and for the whole solve lambda and the outer and inner totals -- on each K^+ path of tests/test_gpu_chain_replay.py and two sizes of its contact problem, with the chain's
replay on and off, with the gradient carried between the inner solves, with row-distributed scalars on one rank, and with a proportioning constant at which
the inner solves take proportioning steps.  The whole-solve tests of
tests/test_gpu_mpgp_phases.py run MPGP alone; the other SMALXE tests compare counts and tolerances.  The cases and how they are recorded:
tests/golden/make_mpgp_driver_bits.py, which this test runs again."""
import importlib.util
import json
import os

import pytest

import permon_amd as pa
from permon_amd._lib import check
from test_gpu_chain_replay import KPLUS

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_mpgp_driver_bits", os.path.join(GOLDEN, "make_mpgp_driver_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def recorded():
    with open(gen.JSON) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    check(c.L.pmh_set_knob(b"chain", 1)), check(c.L.pmh_set_knob(b"chain_replay", 1))
    c.close()


@pytest.fixture(scope="module")
def problems(ctx):
    """One problem per K^+ path and size, built when its first case asks for it and shared by the modes that run on the module's context"""
    made = {}
    return lambda kplus, nel: made[kplus, nel] if (kplus, nel) in made else made.setdefault((kplus, nel), gen.problem(ctx, kplus, nel))


def test_the_generator_covers_what_it_must(recorded):
    """(no GPU work) the generator's copy of the K^+ paths is test_gpu_chain_replay.py's, the recorded cases are the generator's, and between them they hold all
    three step types, a carried gradient and a solve that ends within three steps"""
    assert sorted(gen.KPLUS) == sorted(KPLUS) and all(gen.KPLUS[k](4) == KPLUS[k](4) for k in KPLUS)
    assert sorted(recorded["cases"]) == sorted("%s/nel%d/%s" % c for c in gen.CASES)
    gen.covers(recorded["cases"])


@pytest.mark.parametrize("kplus,nel,mode", gen.CASES)
def test_driver_bits_equal_the_recorded_ones(ctx, problems, recorded, kplus, nel, mode):
    if mode.endswith("dist"):
        c = gen.dist_context()
        try:
            got = gen.compute_case(c, gen.problem(c, kplus, nel), mode)
        finally:
            c.close()
    else:
        got = gen.compute_case(ctx, problems(kplus, nel), mode)
    got, want = json.loads(json.dumps(gen.compact(got))), recorded["cases"]["%s/nel%d/%s" % (kplus, nel, mode)]
    for f in sorted(want):
        if got.get(f) != want[f]:
            print(f, "recorded", want[f], "now", got.get(f))
    assert got == want, ("the driver's bits differ from those recorded at %s with %s; if the toolchain or the intended arithmetic changed, record them again with "
                         "tests/golden/make_mpgp_driver_bits.py" % (recorded["meta"]["commit"][:12], recorded["meta"]["hipcc"]))
