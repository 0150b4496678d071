"""The orbit operator in the symmetry-adapted basis, bit for bit against tests/golden/orbit_adapted_bits.json (recorded by tests/golden/make_orbit_adapted_bits.py on the
commit the file's meta names, before the way k_fxa_prod loads its operands was changed): every output entry keeps its order of
summation -- the four waves' k ranges, the k steps in increasing order, the first half of a step before its second, wave 0 adding the others' sums in wave order --
so dense_mult and F.mult give the recorded bits.  The cases are the smallest at which the k loop can go wrong (waves with no trip, with one, unequal waves, both trip
sizes, items of 1, 2, 3 and 4 blocks of columns); that the file covers them is asserted of the file, that the library still plans them so of pmh_fexplicit_orbit_adapted_info."""
import importlib.util
import json
import os

import pytest

import permon_amd as pa

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_orbit_adapted_bits", os.path.join(HERE, "golden", "make_orbit_adapted_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.JSON) as _f:
    GOLD = json.load(_f)


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    c.close()


def test_file_covers_the_loop():
    assert sorted(GOLD["cases"]) == sorted(gen.CASES)
    gen.covers(GOLD["cases"])


@pytest.mark.parametrize("name", sorted(gen.CASES))
def test_bits(ctx, name):
    """compute_case asserts that two applications give the same bits; here: the plan, the sizes and both hashes equal the file's"""
    sub, nel = gen.CASES[name]
    f, q = gen.problem(ctx, sub, nel)
    got = gen.compute_case(ctx, f, q, nel)
    want = GOLD["cases"][name]
    assert got["plan"] == want["plan"] and (got["groups"], got["n"], got["n_lambda"]) == (want["groups"], want["n"], want["n_lambda"])
    assert got["dense_mult"] == want["dense_mult"]
    assert got["F_mult"] == want["F_mult"]
