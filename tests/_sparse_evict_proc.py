"""Helper: one rank of a gloo sparse-PS run that serves a hashed table WITH
THE AUTOMATIC EVICTION POLICY (evict_every=2, max_idle=2) through the stock
SparsePSServer / SparseWorkerClient. Worlds, tables and key pools are those
of _sparse_hash_proc.py (world 2: one unsharded Adagrad table; world 3: two
``shard_of`` shards of an Adam table); the script walks a window over the
key pool so that keys go idle, are evicted on the PS and are named again.
Every PS rank saves its table BY GLOBAL KEY, stamps and counters included.

usage: _sparse_evict_proc.py OUT_PREFIX
       (HASH_PROC_DEVICE: cpu | cuda:0, HASH_PROC_COALESCE: 0 | 1)
       writes OUT_PREFIX.pulls.pt (worker) and OUT_PREFIX.ps<rank>.pt

Imported by test_hash_evict_dist.py / test_hash_evict_gpu.py for the request
script, so that the tests apply the very same sequence locally."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sparse_hash_proc as base  # noqa: E402
from tfmesos_amd import ops  # noqa: E402
from tfmesos_amd.ps.sparse import (  # noqa: E402
    HashedEmbeddingTable, SparsePSServer, SparseWorkerClient,
    make_sparse_pair_groups)

DIM, N, CAPACITY, BAGS = base.DIM, base.N, base.CAPACITY, base.BAGS
POLICY = dict(evict_every=2, max_idle=2)
WINDOWS = [(0, 12), (8, 20), (12, 24), (14, 24), (4, 16)]


def requests(world):
    """Per window of the 24-key pool: pull, push, pull, pooled pull, pooled
    push, pooled pull — two pushes, so the policy runs once per window.
    Gradients and bags as in _sparse_hash_proc.requests (exact per-key sums,
    one residue class mod 2 per bag). The script ends with a pull of every
    key: the evicted ones come back with their initial rows."""
    pool = base.key_pool(world)
    gen = torch.Generator().manual_seed(170 + world)

    def grads(n):
        return torch.randint(-4, 5, (n, DIM), generator=gen).float() / 16

    def bagged(keys):
        lens = torch.randint(0, 9, (BAGS,), generator=gen)
        cls = [keys[keys % 2 == b % 2] for b in range(BAGS)]
        k = torch.cat([c[torch.randint(0, c.numel(), (int(n),),
                                       generator=gen)]
                       for c, n in zip(cls, lens)])
        offsets = torch.cat([torch.tensor([0]), lens.cumsum(0)])
        weights = torch.randint(1, 5, (k.numel(),), generator=gen) / 4
        return k, offsets, weights

    reqs = []
    for lo, hi in WINDOWS:
        k = pool[lo:hi][torch.randint(0, hi - lo, (N,), generator=gen)]
        reqs += [("pull", k), ("push", k, grads(N)), ("pull", k)]
        k, o, w = bagged(pool[lo:hi])
        reqs += [("pull_pooled", k, o, None, "sum"),
                 ("push_pooled", k, o, grads(BAGS), w, "mean"),
                 ("pull_pooled", k, o, w, "mean")]
    reqs.append(("pull", pool))
    return reqs


def make_local(world, device="cpu"):
    """One unsharded table with the PS tables' parameters and policy."""
    return HashedEmbeddingTable("T", DIM, CAPACITY, device=device,
                                **base.config(world)["table"], **POLICY)


def by_key(table):
    """base.by_key plus "last_used" and "evicted"."""
    out = base.by_key(table)
    n = out["keys"].numel()
    out["last_used"] = table.last_used[:n].cpu()
    out["evicted"] = table.stats()["evicted"]
    return out


def main():
    import torch.distributed as dist
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    device = os.environ.get("HASH_PROC_DEVICE", "cpu")
    coalesce = os.environ.get("HASH_PROC_COALESCE", "0") == "1"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = base.config(world)
    home = cfg["homes"]["T"]
    sharded = isinstance(home, list)
    ps_ranks = list(range(world - 1))
    worker = world - 1
    chans = make_sparse_pair_groups(ps_ranks, [worker])
    if rank == worker:
        client = SparseWorkerClient(
            rank, cfg["homes"], {"T": DIM}, chans, device=device,
            rows={"T": ops.HASH_KEY_SPACE} if sharded else None,
            strategy="mod", coalesce=coalesce)
        pulled = []
        for method, *args in requests(world):
            res = getattr(client, method)("T", *args)
            if method.startswith("pull"):
                pulled.append(res.cpu())
        client.done_all()
        torch.save(pulled, sys.argv[1] + ".pulls.pt")
    else:
        kw = dict(device=device, **cfg["table"], **POLICY)
        if sharded:
            table = HashedEmbeddingTable.shard_of(
                "T", DIM, home.index(rank), len(home), CAPACITY, **kw)
        else:
            table = HashedEmbeddingTable("T", DIM, CAPACITY, **kw)
        SparsePSServer(rank, [table], [worker], chans).serve()
        torch.save(by_key(table), sys.argv[1] + ".ps%d.pt" % rank)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
