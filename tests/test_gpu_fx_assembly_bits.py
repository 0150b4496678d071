"""The set-up of the explicit local dual operators, bit for bit against tests/golden/fx_assembly_bits.json (recorded by tests/golden/make_fx_assembly_bits.py on the commit
the file's meta names, while the set-up loop still existed twice): which column is solved in which slot of which batch decides its companions in the batched K^+ solve,
hence its bits, and a row stored twice or into another place changes a block -- the tolerance tests of tests/test_gpu_explicit.py would let either pass.  The same
hashes from the set-up cut into windows of batches (pmh_fexplicit_assemble_window), which the library itself reaches only through the probe of pmh_feti_contact_solve."""
import importlib.util
import json
import os

import numpy as np
import pytest

import permon_amd as pa

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_fx_assembly_bits", os.path.join(HERE, "golden", "make_fx_assembly_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.JSON) as _f:
    GOLD = json.load(_f)


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    c.close()


def test_file_has_every_case():
    assert sorted(GOLD["cases"]) == sorted(gen.CASES)
    for name, case in GOLD["cases"].items():
        assert ("blocks" in case) == (name not in gen.NO_BLOCKS) and ("mult" in case) == (name in gen.STRIPED), name


@pytest.mark.parametrize("name", sorted(gen.CASES))
def test_bits(ctx, name):
    assert gen.compute_case(ctx, name) == GOLD["cases"][name]


# one per-block form, the set-up by symmetry on the symmetric tiles and the orbit storage (both end with the self-check batch)
WINDOWED = ["edge/127-128-129/sym/mv0", "class_sym+sym/2x2x2/nel4", "class_orbit/2x2x2/nel5"]


@pytest.mark.parametrize("name", WINDOWED)
def test_windows(ctx, name, monkeypatch):
    """The set-up in three windows of batches gives the plan, the solve count and the bits of the whole set-up, and the operator applies only after the last one.
    Cut points: [0, 1), [1, 3), [3, end) where the plan has four batches or more, [0, 1), [1, 2), [2, end) where it has three (2x2x2 cubes by symmetry: two batches of
    representatives on the 8 slots and the self-check, which is then a window of its own)."""
    whole = pa.MatExplicitDual.assemble
    plans = []

    def run(cuts):
        def windowed(E, solver, **kw):
            lam = ctx.vec_from(np.ones(E.B.n_lambda))
            y = ctx.vec(E.B.n_lambda)
            for i, (lo, hi) in enumerate(cuts):
                if i:  # (before the first window the operator is as unassembled as after it)
                    with pytest.raises(pa.PermonHipError, match="assembl"):
                        E.mult(lam, y)
                plans.append(whole(E, solver, window=(lo, hi), **kw))
            return None

        monkeypatch.setattr(pa.MatExplicitDual, "assemble", windowed)
        got = gen.compute_case(ctx, name)
        monkeypatch.setattr(pa.MatExplicitDual, "assemble", whole)
        return got

    want = GOLD["cases"][name]
    assert run([(0, None)]) == want  # the whole set-up through the window entry
    nbatch, nsolves, complete = plans.pop()
    assert complete and nbatch >= 3 and nsolves == want["n_solves"]
    c2 = 3 if nbatch >= 4 else 2
    assert run([(0, 1), (1, c2), (c2, None)]) == want  # (n_solves = assemble_stats()[0], the blocks' hashes)
    assert plans == [(nbatch, nsolves, False), (nbatch, nsolves, False), (nbatch, nsolves, True)]
