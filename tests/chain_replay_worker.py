"""World-size-2 worker for tests/test_gpu_chain_replay.py::test_two_ranks_replay_alike: SMALXE on the dual-space chain with the subdomains split among two processes that share
the box's one GPU, the chain's all-reduce of [w; sums of G0 w] on the library's host transport carried by gloo (as tests/dist_transport_worker.py does).  A replay of the
chain's last stage has no collective: both ranks must take the same replays, and the solve must be the one-rank solve.

usage: chain_replay_worker.py   (RANK / WORLD_SIZE / MASTER_PORT in the environment)"""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import permon_amd as pa  # noqa: E402
from permon_amd._lib import check  # noqa: E402

CALLS = {0: 0, 1: 0, 2: 0}


def transport(op, arr):
    CALLS[op] += 1
    if op == 2 or arr.size == 0:
        dist.barrier()
        return
    t = torch.from_numpy(arr)  # a view of the library's pinned staging buffer: reduced in place
    dist.all_reduce(t, op=dist.ReduceOp.SUM if op == 0 else dist.ReduceOp.MIN)


def knob(ctx, name):
    v = C.c_int()
    check(ctx.L.pmh_get_knob(name.encode(), C.byref(v)))
    return v.value


def solve(ctx, q, replay):
    check(ctx.L.pmh_set_knob(b"chain_replay", replay))
    check(ctx.L.pmh_set_knob(b"chain_replays", 0)), check(ctx.L.pmh_set_knob(b"chain_applies", 0))
    q.lam.set(0.0)
    st = q.solve_smalxe()
    out = dict(counts=(st.reason, st.iteration, st.inner_iter_accu, st.M1_updates, st.rho_updates, st.inner.ncg, st.inner.nexp, st.inner.nprop, st.inner.nmv),
               lam=q.lam.to_numpy().copy(), replays=knob(ctx, "chain_replays"), applies=knob(ctx, "chain_applies"))
    q.qps.Destroy()
    return out


def run(ctx, rank, world):
    from permon_amd.chain import FetiDualQP

    check(ctx.L.pmh_set_knob(b"chain", 1))
    f = pa.CubeFeti((2, 2, 2), 3, contact=True)
    G0, e0 = f.coarse(orthonormalize=False)
    kw = dict(orthonormal="implicit", kplus_rtol=1e-13)
    # one rank: all 8 blocks on this process, no transport
    one = solve(ctx, FetiDualQP(ctx, f.subset(range(f.nsub)), G0, e0, f.c, f.lb, **kw), 1)
    assert one["counts"][0] > 0 and one["applies"] > 0 and one["replays"] >= one["counts"][1] - 1 > 0, one
    # two ranks: 4 blocks each, lambda replicated
    ctx.comm_set_host_transport(rank, world, transport)
    per = f.nsub // world
    q = FetiDualQP(ctx, f.subset(range(rank * per, (rank + 1) * per)), G0, e0, f.c, f.lb, **kw)
    c0 = CALLS[0]
    two = solve(ctx, q, 1)
    exchanges_on = CALLS[0] - c0
    c0 = CALLS[0]
    off = solve(ctx, q, 0)
    exchanges_off = CALLS[0] - c0
    assert two["applies"] > 0 and off["replays"] == 0
    assert two["counts"] == one["counts"] == off["counts"], (two["counts"], one["counts"], off["counts"])
    assert two["replays"] == one["replays"], (two["replays"], one["replays"])
    assert exchanges_off - exchanges_on == two["replays"], (exchanges_on, exchanges_off, two["replays"])  # a replay has no collective
    assert np.array_equal(two["lam"], off["lam"])  # on against off, same ranks: the same bits
    errl = np.linalg.norm(two["lam"] - one["lam"]) / np.linalg.norm(one["lam"])
    assert errl <= 1e-8, errl  # (the ranks' shares of B u are summed in another order than one rank sums them)
    t = torch.tensor(list(two["counts"]) + [two["replays"], two["applies"]], dtype=torch.float64)
    t2 = t.clone()
    dist.all_reduce(t2, op=dist.ReduceOp.MAX)
    assert torch.equal(t, t2), "the ranks disagree on the counters or on the replays"
    tl = torch.from_numpy(two["lam"].copy())
    tm = tl.clone()
    dist.all_reduce(tm, op=dist.ReduceOp.MAX)
    assert torch.equal(tl, tm), "replicated lambda differs between the ranks"
    return "2 ranks %s == 1 rank, %d replays of %d applications on every rank, |lambda - lambda_1| = %.1e" % (two["counts"], two["replays"], two["applies"], errl)


def main():
    if not (dist.is_available() and dist.is_gloo_available()):
        sys.exit(77)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["MASTER_PORT"], rank=rank, world_size=world)
    ctx = pa.Context(0)  # both ranks on the box's one GPU
    try:
        msg = run(ctx, rank, world)
        ok = True
    except Exception:  # noqa: BLE001
        import traceback

        traceback.print_exc()
        msg, ok = "failed", False
    t = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    ctx.comm_set_host_transport(0, 1, None)
    ctx.close()
    dist.destroy_process_group()
    if not (ok and t.item() == 1.0):
        sys.exit(1)
    print("rank %d ok: %s" % (rank, msg))


if __name__ == "__main__":
    main()
