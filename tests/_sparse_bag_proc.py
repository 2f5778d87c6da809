"""Helper: one rank of a gloo sparse-PS run that interleaves row and
pooled (bag) requests. World 2 = one PS homing both tables + one worker;
world 3 = two PS homing one table each + one worker. The PS ranks print a
checksum of every table they home; the worker saves what it pulled.

usage: _sparse_bag_proc.py PULLS_OUT.pt

Imported by test_embedding_bag.py for the request script, so that the
test applies the very same sequence to local tables."""

import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd.ps.sparse import (  # noqa: E402
    EmbeddingTable, SparsePSServer, SparseWorkerClient,
    make_sparse_pair_groups)

TABLES = {      # name -> constructor arguments
    "A": dict(rows=50, dim=8, lr=0.1, seed=11, optimizer="adagrad"),
    "B": dict(rows=40, dim=12, lr=0.05, seed=12, optimizer="adam"),
}


def make_tables(names):
    return [EmbeddingTable(n, **TABLES[n]) for n in names]


def requests():
    """The fixed request script: (method, table, args...). Gradients are
    dyadic (randint/16), so the bf16 wire format carries them exactly."""
    gen = torch.Generator().manual_seed(5)
    reqs = []
    modes = [("sum", False), ("mean", True), ("sum", True), ("mean", False)]
    for k in range(8):
        name = "AB"[k % 2]
        rows, dim = TABLES[name]["rows"], TABLES[name]["dim"]
        combiner, weighted = modes[(k // 2) % 4]
        lens = torch.randint(0, 6, (7,), generator=gen)
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64),
                             lens.cumsum(0)])
        n = int(offsets[-1])
        ids = torch.randint(0, rows, (n,), generator=gen)
        weights = None
        if weighted:
            weights = torch.tensor([0.5, 1.0, 2.0])[
                torch.randint(0, 3, (n,), generator=gen)]
        bag_g = torch.randint(-32, 33, (7, dim), generator=gen).float() / 16
        row_ids = torch.randint(0, rows, (9,), generator=gen)
        row_g = torch.randint(-32, 33, (9, dim), generator=gen).float() / 16
        reqs.append(("pull", name, row_ids))
        reqs.append(("pull_pooled", name, ids, offsets, weights, combiner))
        reqs.append(("push_pooled", name, ids, offsets, bag_g, weights,
                     combiner))
        reqs.append(("push", name, row_ids, row_g))
        reqs.append(("pull_pooled", name, ids, offsets, weights, combiner))
    return reqs


def apply_local(tables, reqs):
    """The request script on local tables {name: EmbeddingTable}; pushes
    see bf16 gradients, as over the wire. Returns the pulled tensors."""
    pulled = []
    for method, name, *args in reqs:
        t = tables[name]
        if method == "pull":
            pulled.append(t.pull(*args))
        elif method == "pull_pooled":
            pulled.append(t.pull_pooled(*args))
        elif method == "push":
            t.push(args[0], args[1].to(torch.bfloat16))
        else:
            ids, offsets, g, weights, combiner = args
            t.push_pooled(ids, offsets, g.to(torch.bfloat16), weights,
                          combiner)
    return pulled


def checksum(table):
    h = hashlib.sha256()
    for t in [table.master] + [table.state[k] for k in sorted(table.state)]:
        h.update(t.numpy().tobytes())
    h.update(str(table.step).encode())
    return h.hexdigest()


def main():
    import torch.distributed as dist
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ps_ranks = list(range(world - 1))
    worker = world - 1
    homes = {"A": 0, "B": ps_ranks[-1]}
    chans = make_sparse_pair_groups(ps_ranks, [worker])
    if rank == worker:
        client = SparseWorkerClient(
            rank, homes, {n: kw["dim"] for n, kw in TABLES.items()}, chans)
        pulled = []
        for method, name, *args in requests():
            out = getattr(client, method)(name, *args)
            if out is not None:
                pulled.append(out)
        client.done_all()
        torch.save(pulled, sys.argv[1])
    else:
        tables = make_tables(sorted(n for n, h in homes.items() if h == rank))
        SparsePSServer(rank, tables, [worker], chans).serve()
        for t in tables:
            print("CHECKSUM %s %s" % (t.name, checksum(t)))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
