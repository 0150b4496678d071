"""The dual-space chain multiplies the same vector again (permon_amd/csrc/dualchain.hip pmh_dc_replay): SMALXE's objective and the first gradient of the next inner
MPGP solve are taken at the iterate the previous inner solve ended its last gradient on.  c = S G0 x and [w; sums of G0 w] of that application are still in the chain's
buffers and do not depend on rho, b or the epilogue, so the last kernel alone gives the bits the five launches would give.  Checked here: bit equality with the full
chain, every way the record of "whose intermediates these are" has to be dropped, SMALXE with the feature on against off, and two ranks."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import permon_amd as pa
from permon_amd._lib import check
from permon_amd.chain import FetiDualQP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

KPLUS = {
    "orbit": lambda nn: dict(explicit=dict(rtol=1e-13, storage="class_orbit", symmetry=dict(dims=(nn, nn, nn), ndof=3))),
    "sym": lambda nn: dict(explicit=dict(rtol=1e-13, storage="sym")),
    "iterative": lambda nn: dict(),
}
CAP = 4096  # room per row of block partials / for the segment sums (n <= 4096 * 1024 entries, at most 64 segments per tile of 1024: far above these shapes)


@pytest.fixture(scope="module")
def ctx():
    c = pa.Context(0)
    yield c
    check(c.L.pmh_set_knob(b"chain", 1)), check(c.L.pmh_set_knob(b"chain_replay", 1))
    c.close()


def _knob(ctx, name):
    v = C.c_int()
    check(ctx.L.pmh_get_knob(name.encode(), C.byref(v)))
    return v.value


def _set(ctx, name, value):
    check(ctx.L.pmh_set_knob(name.encode(), int(value)))


def _problem(ctx, kplus, sub=(2, 2, 2), nel=3):
    f = pa.CubeFeti(sub, nel, contact=True)
    G0, e0 = f.coarse(orthonormalize=False)
    q = FetiDualQP(ctx, f.subset(range(f.nsub)), G0, e0, f.c, f.lb, orthonormal="implicit", kplus_rtol=1e-13, **KPLUS[kplus](nel + 1))
    return f, G0, q


def _f_applies(ctx, q):
    n = C.c_longlong()
    check(ctx.L.pmh_feti_dual_applies(q.F.h, C.byref(n)))
    return n.value


def _middle_stage_work(q, kplus):
    """A count that grows with every run of the chain's middle stage: the timed dense launches of the explicit operators, or the running total of the K x products of
    the inner Krylov solves (`total_spmv` of pmh_matinv_last_iterations: summed over all solves, not the last solve's).  The check that stands on its own is the one
    beside it, `pmh_feti_dual_applies`: F counts every run of its middle stage where it starts it."""
    return q.E.timing_get()[0] if kplus != "iterative" else q.Kplus.last_iterations()[1]


def _mult(ctx, op, xv, same_input):
    y = ctx.vec(xv.n)
    check(ctx.L.pmh_op_penalized_test_mult_epi(op.h, 0, int(same_input), xv.p, None, None, 0.0, y.p, None, None, 0, None, None, None, None))
    return y.to_numpy()


def _grad_split(ctx, op, xv, bv, lbv, same_input):
    """g, gf, p, the four rows of block partials and the emitted segment sums of G0 p of one gradient split through the operator's last kernel"""
    n = xv.n
    g, gf, p = ctx.vec(n), ctx.vec(n), ctx.vec(n)
    part, psum = np.zeros(4 * CAP), np.zeros(CAP)
    nb, ns = C.c_int(), C.c_int()
    check(ctx.L.pmh_op_penalized_test_mult_epi(op.h, 2, int(same_input), xv.p, bv.p, lbv.p, 1e-12, g.p, gf.p, p.p, CAP, part.ctypes.data_as(C.c_void_p),
                                               psum.ctypes.data_as(C.c_void_p), C.byref(nb), C.byref(ns)))
    assert nb.value == (n + 1023) // 1024 and ns.value > 0
    return dict(g=g.to_numpy(), gf=gf.to_numpy(), p=p.to_numpy(), partials=part[:4 * nb.value].reshape(4, nb.value).copy(), psums=psum[:ns.value].copy())


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _iterate(rng, lb):
    """A feasible vector with entries ON the bound (the split's chopped part is exercised) and free ones"""
    x = rng.standard_normal(lb.size)
    fin = np.isfinite(lb)
    x[fin] = lb[fin] + np.maximum(x[fin], 0.0)
    return x


@pytest.mark.parametrize("kplus,nel", [("orbit", 3), ("sym", 3), ("iterative", 3), ("orbit", 7)])  # nel = 7: more than one tile of 1024 dual entries
def test_last_stage_alone_equals_full_chain(ctx, kplus, nel):
    _set(ctx, "chain", 1), _set(ctx, "chain_replay", 1)
    f, G0, q = _problem(ctx, kplus, nel=nel)
    n = f.n_lambda
    assert (n > 1024) == (nel == 7)
    rng = np.random.default_rng(11)
    lb = q.lb_new.to_numpy()
    A1 = pa.MatCreatePenalized(q.A, q.pf, 2.5)
    Aref = pa.MatCreatePenalized(q.A, q.pf, 2.5)
    if kplus != "iterative":
        q.E.timing_enable(64)
    # (a) a plain product, then the gradient split of the same x with another rho and another b
    x, b = _iterate(rng, lb), rng.standard_normal(n)
    xv, bv = ctx.vec_from(x), ctx.vec_from(b)
    _mult(ctx, A1, xv, False)
    _set(ctx, "chain_replays", 0), _set(ctx, "chain_applies", 0), _set(ctx, "chain_launches", 0)
    fa, mid = _f_applies(ctx, q), _middle_stage_work(q, kplus)
    check(ctx.L.pmh_op_penalized_set_penalty(A1.h, 7.25))
    got = _grad_split(ctx, A1, xv, bv, q.lb_new, True)
    assert _knob(ctx, "chain_replays") == 1 and _knob(ctx, "chain_applies") == 1
    assert _knob(ctx, "chain_launches") == 2  # the emission of G0 x for SMALXE's ||B u|| and the last kernel
    assert _f_applies(ctx, q) == fa and _middle_stage_work(q, kplus) == mid  # the middle stage did not run
    check(ctx.L.pmh_op_penalized_set_penalty(Aref.h, 7.25))
    _set(ctx, "chain_replay", 0)
    _mult(ctx, Aref, xv, False)
    ref = _grad_split(ctx, Aref, xv, bv, q.lb_new, True)  # the switch is off: the full chain whatever the caller says
    _set(ctx, "chain_replay", 1)
    assert _knob(ctx, "chain_replays") == 1 and _f_applies(ctx, q) == fa + 2
    _same(got, ref)
    assert np.count_nonzero(got["gf"] == 0.0) > 0 and np.count_nonzero(got["gf"]) > 0 and np.all(got["partials"][1:].sum(axis=1) > 0.0)
    # (b) a gradient split, then the plain product of the same x with another rho
    x2 = _iterate(rng, lb)
    xv2 = ctx.vec_from(x2)
    _grad_split(ctx, A1, xv2, bv, q.lb_new, False)
    fa = _f_applies(ctx, q)
    check(ctx.L.pmh_op_penalized_set_penalty(A1.h, 0.75)), check(ctx.L.pmh_op_penalized_set_penalty(Aref.h, 0.75))
    _set(ctx, "chain_launches", 0)
    y = _mult(ctx, A1, xv2, True)
    assert _knob(ctx, "chain_replays") == 2 and _knob(ctx, "chain_launches") == 1 and _f_applies(ctx, q) == fa
    assert np.array_equal(y, _mult(ctx, Aref, xv2, False))
    # ... and once more: a replay leaves the record as it was
    assert np.array_equal(y, _mult(ctx, A1, xv2, True)) and _knob(ctx, "chain_replays") == 3
    A1.destroy(), Aref.destroy()


@pytest.mark.parametrize("case", ["control", "other_vector", "invalidate", "emitted", "stages", "realloc"])
def test_record_is_dropped_when_it_must_be(ctx, case):
    """A request to multiply 'the same vector again' is served by the full chain -- equal result, no replay counted -- whenever the chain cannot know that its
    intermediates are still that vector's."""
    _set(ctx, "chain", 1), _set(ctx, "chain_replay", 1)
    f, G0, q = _problem(ctx, "iterative" if case == "stages" else "sym")
    n = f.n_lambda
    rng = np.random.default_rng(5)
    A1 = pa.MatCreatePenalized(q.A, q.pf, 2.5)
    x = rng.standard_normal(n)
    xv = ctx.vec_from(x)
    y0 = _mult(ctx, A1, xv, False)
    _set(ctx, "chain_replays", 0)
    fa = _f_applies(ctx, q)
    expect_replays, expect = 0, y0
    if case == "control":  # nothing happened: this is the situation all the others differ from
        expect_replays = 1
    elif case == "other_vector":
        zv = ctx.vec_from(rng.standard_normal(n))
        _mult(ctx, A1, zv, False)
        fa += 1
    elif case == "invalidate":  # x or p are about to change without emission
        check(ctx.L.pmh_op_penalized_test_emit(A1.h, 0, None))
    elif case == "emitted":  # a kernel wrote x and left the segment sums of G0 x behind
        x2 = rng.standard_normal(n)
        xv.set_numpy(x2)
        check(ctx.L.pmh_op_penalized_test_emit(A1.h, 1, xv.p))
    elif case == "stages":  # the explicit operators are attached to K^+: F's gather, middle and scatter stages are others now
        q.E = q.assemble_explicit(f.subset(range(f.nsub)), rtol=1e-13, storage="sym")
        fa = _f_applies(ctx, q)
    elif case == "realloc":  # the vector is freed, another one is allocated (at its address, as the allocator usually does for equal sizes) with other contents
        old = xv.p.value
        xv.free()
        xv = ctx.vec_from(rng.standard_normal(n))  # (wherever it lands: the full chain either way)
        # the count of pmh_free calls is what drops the record where the address came back; elsewhere the address comparison alone already does
        print("realloc: the new vector %s the freed one's address" % ("got" if xv.p.value == old else "did NOT get"))
    y = _mult(ctx, A1, xv, True)
    assert _knob(ctx, "chain_replays") == expect_replays
    assert _f_applies(ctx, q) == fa + (0 if expect_replays else 1)
    if case in ("emitted", "stages", "realloc"):
        expect = _mult(ctx, A1, xv, False)
        assert not np.array_equal(expect, y0)
    assert np.array_equal(y, expect)
    A1.destroy()


@pytest.mark.parametrize("kplus,sub,nel", [("orbit", (2, 2, 2), 3), ("iterative", (2, 1, 2), 3)])
def test_smalxe_replay_on_against_off(ctx, kplus, sub, nel):
    """The contact problem of test_gpu_chain.py's SMALXE test: the same bits and the same counters with the feature on and off; on, at least the first gradient of every
    inner solve after the first is a replay, and F itself runs that many times less.  On these inputs every inner solve after the first starts from a feasible u: no
    first gradient has to be taken again because the solve's projection changed the iterate (`chain_replays_redone`; test_contact_solve_projection_changes_iterate has one)."""
    _set(ctx, "chain", 1)
    f, G0, q = _problem(ctx, kplus, sub, nel)
    res = {}
    for on in (1, 0):
        _set(ctx, "chain_replay", on)
        _set(ctx, "chain_replays", 0), _set(ctx, "chain_applies", 0), _set(ctx, "chain_replays_redone", 0)
        fa = _f_applies(ctx, q)
        q.lam.set(0.0)
        st = q.solve_smalxe()
        res[on] = dict(lam=q.lam.to_numpy(), counts=(st.reason, st.iteration, st.inner_iter_accu, st.M1_updates, st.rho_updates, st.inner.ncg, st.inner.nexp, st.inner.nprop, st.inner.nmv),
                       replays=_knob(ctx, "chain_replays"), applies=_knob(ctx, "chain_applies"), f_applies=_f_applies(ctx, q) - fa, iteration=st.iteration)
        q.qps.Destroy()
    _set(ctx, "chain_replay", 1)
    on, off = res[1], res[0]
    print("SMALXE %s: outer %d, chain applications %d, replays %d, F applications %d (on) / %d (off)" % (kplus, on["iteration"], on["applies"], on["replays"], on["f_applies"], off["f_applies"]))
    assert on["counts"][0] > 0 and on["counts"] == off["counts"]
    assert np.array_equal(on["lam"], off["lam"])
    assert off["replays"] == 0 and on["iteration"] > 1 and on["replays"] >= on["iteration"] - 1
    assert _knob(ctx, "chain_replays_redone") == 0
    assert on["applies"] == off["applies"]  # a replay is an application of the operator
    assert on["f_applies"] == off["f_applies"] - on["replays"]


def test_contact_solve_projection_changes_iterate(ctx):
    """An expansion step leaves x - afeas p - alpha gr without re-projection, which may lie a rounding error below a bound; the next inner solve's projection then changes
    the vector the chain's intermediates belong to.  The one-call contact solve of tests/test_gpu_explicit.py (2 x 2 x 1 cubes of 6^3 elements, Knoll start) on the
    inner-Krylov K^+ has such an iterate (the arithmetic is deterministic: fixed summation orders).  The solve notices at its first wait and takes that gradient again in full: the same bits and counters
    as with the feature off."""
    _set(ctx, "chain", 1)
    f = pa.CubeFeti((2, 2, 1), 6, contact=True)
    res = {}
    for on in (1, 0):
        _set(ctx, "chain_replay", on)
        _set(ctx, "chain_replays", 0), _set(ctx, "chain_replays_redone", 0)
        u, lam, st = pa.FETIContactSolve(ctx, f, explicit=False)
        s = st.smalxe
        res[on] = dict(u=u, lam=lam, counts=(s.reason, s.iteration, s.inner_iter_accu, s.M1_updates, s.rho_updates, s.inner.ncg, s.inner.nexp, s.inner.nprop, s.inner.nmv),
                       replays=_knob(ctx, "chain_replays"), redone=_knob(ctx, "chain_replays_redone"), f_applies=st.f_applies)
    _set(ctx, "chain_replay", 1)
    on, off = res[1], res[0]
    print("contact solve: outer %d, replays %d of which %d taken again in full, F applications %d (on) / %d (off)" % (on["counts"][1], on["replays"], on["redone"], on["f_applies"], off["f_applies"]))
    assert on["counts"][0] > 0 and on["counts"] == off["counts"]
    assert np.array_equal(on["lam"], off["lam"]) and np.array_equal(on["u"], off["u"])
    assert off["replays"] == 0 and off["redone"] == 0
    assert on["redone"] >= 1 and on["replays"] >= on["counts"][1] - 1
    assert on["f_applies"] == off["f_applies"] - (on["replays"] - on["redone"])  # a gradient taken again runs F after all


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_replay_alike():
    """Two processes on the one GPU, the B u all-reduce on the host transport: a replay has no collective, so both ranks must take the same ones.
    What tests/chain_replay_worker.py holds the two ranks to: the counters and `chain_replays` equal to one rank's and equal on both ranks; the all-reduces fewer by
    exactly the replays; lambda bit-equal between the ranks and bit-equal with the feature on and off on two ranks.  Against ONE rank lambda is compared to 1e-8
    relative only, not bit for bit: two ranks sum their shares of B u in another order than one rank sums all blocks, with the feature off just as well."""
    # (torch is not imported into this process: it brings a HIP runtime of its own, and this process has already initialised the library's.  The workers import it
    # first, as tests/dist_transport_worker.py does, and say with exit status 77 that there is no gloo to carry the transport)
    import importlib.util

    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch is not installed: no carrier for the host transport")
    port = str(_free_port())
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "chain_replay_worker.py")], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate()[0] for p in procs]
    if all(p.returncode == 77 for p in procs):
        pytest.skip("torch.distributed has no gloo backend: no carrier for the host transport")
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, o[-4000:])
        assert "rank %d ok" % r in o, o[-2000:]
