"""Helper: one rank of a gloo sparse-PS run that serves a HASHED table
through the stock SparsePSServer / SparseWorkerClient. World 2 = one PS rank
holding the unsharded Adagrad table "T" + one worker; world 3 = 2 PS ranks
holding the two ``HashedEmbeddingTable.shard_of`` shards of the Adam table
"T" + one worker (``rows={"T": ops.HASH_KEY_SPACE}``, strategy "mod"). The
worker runs a fixed script of row and pooled pulls and pushes, with
``coalesce`` on (HASH_PROC_COALESCE=1) or off, and saves what it pulled;
every PS rank saves its table BY GLOBAL KEY.

usage: _sparse_hash_proc.py OUT_PREFIX
       (HASH_PROC_DEVICE: cpu | cuda:0, HASH_PROC_COALESCE: 0 | 1)
       writes OUT_PREFIX.pulls.pt (worker) and OUT_PREFIX.ps<rank>.pt

Imported by test_hash_dist.py / test_hash_gpu.py for the request script, so
that the tests apply the very same sequence locally."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd import ops  # noqa: E402
from tfmesos_amd.ps.sparse import (  # noqa: E402
    HashedEmbeddingTable, SparsePSServer, SparseWorkerClient,
    make_sparse_pair_groups)

DIM = 8
N = 40              # positions per request
CAPACITY = 64       # per table (and per shard)
BAGS = 6


def config(world):
    if world == 2:
        return dict(homes={"T": 0},
                    table=dict(lr=0.1, seed=51, optimizer="adagrad"))
    return dict(homes={"T": [0, 1]},
                table=dict(lr=0.05, seed=52, optimizer="adam"))


def key_pool(world):
    """24 keys. The unsharded table takes the full int64 range; the sharded
    one keys in [0, 2**62)."""
    gen = torch.Generator().manual_seed(60 + world)
    if world == 2:
        return torch.cat([
            torch.randint(-2 ** 62, 2 ** 62, (20,), generator=gen),
            torch.tensor([2 ** 63 - 1, 0, -1, 2 ** 40 + 3])])
    return torch.cat([
        torch.randint(0, ops.HASH_KEY_SPACE, (20,), generator=gen),
        torch.tensor([0, 1, ops.HASH_KEY_SPACE - 1, 2 ** 40 + 3])])


def requests(world):
    """The fixed script: (method, args...). Keys appear gradually (the
    first 12 of the pool, then all 24). Gradients are randint(-4, 5)/16 and
    a per-key sum over at most 40 positions is exact in bf16, so the PS
    gets the same per-key totals with and without coalescing. Every bag of
    a pooled request draws its keys from ONE residue class mod 2: a sharded
    table's pooled pull is then one shard's partial plus zeros, equal to
    the unsharded table's bag bit for bit."""
    pool = key_pool(world)
    gen = torch.Generator().manual_seed(70 + world)

    def draw(hi):
        return pool[torch.randint(0, hi, (N,), generator=gen)]

    def grads(n):
        return torch.randint(-4, 5, (n, DIM), generator=gen).float() / 16

    def bagged(hi):
        lens = torch.randint(0, 9, (BAGS,), generator=gen)
        cls = [pool[:hi][pool[:hi] % 2 == b % 2] for b in range(BAGS)]
        keys = torch.cat([c[torch.randint(0, c.numel(), (int(n),),
                                          generator=gen)]
                          for c, n in zip(cls, lens)])
        offsets = torch.cat([torch.tensor([0]), lens.cumsum(0)])
        weights = torch.randint(1, 5, (keys.numel(),), generator=gen) / 4
        return keys, offsets, weights

    reqs = []
    for hi in (12, 24, 24):
        k = draw(hi)
        reqs += [("pull", k), ("push", k, grads(N)), ("pull", k)]
        k, o, w = bagged(hi)
        reqs += [("pull_pooled", k, o, None, "sum"),
                 ("push_pooled", k, o, grads(BAGS), w, "mean"),
                 ("pull_pooled", k, o, w, "mean")]
    reqs.append(("pull", pool))     # every key has a row in the end
    return reqs


def make_local(world, device="cpu"):
    """One unsharded table with the PS tables' parameters."""
    return HashedEmbeddingTable("T", DIM, CAPACITY, device=device,
                                **config(world)["table"])


def apply_local(table, reqs, device="cpu"):
    """The script on a local table, uncoalesced; pushes see bf16 gradients,
    as over the wire. Returns the pulled tensors."""
    pulled = []
    for method, *args in reqs:
        args = [a.to(device) if isinstance(a, torch.Tensor) else a
                for a in args]
        if method == "push":
            table.push(args[0], args[1].to(torch.bfloat16))
        elif method == "push_pooled":
            k, o, g, w, comb = args
            table.push_pooled(k, o, g.to(torch.bfloat16), w, comb)
        else:
            pulled.append(getattr(table, method)(*args))
    return pulled


def by_key(table):
    """{"keys" (global), "master", "state", "step", "dropped"} on the CPU."""
    st = table.stats()
    n = st["size"]
    return {"keys": table.index.row_keys[:n].cpu() * table.key_mul
            + table.key_add,
            "master": table.master[:n].cpu(),
            "state": {k: v[:n].cpu() for k, v in table.state.items()},
            "step": table.step, "dropped": st["dropped"]}


def main():
    import torch.distributed as dist
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    device = os.environ.get("HASH_PROC_DEVICE", "cpu")
    coalesce = os.environ.get("HASH_PROC_COALESCE", "0") == "1"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = config(world)
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
        if sharded:
            table = HashedEmbeddingTable.shard_of(
                "T", DIM, home.index(rank), len(home), CAPACITY,
                device=device, **cfg["table"])
        else:
            table = HashedEmbeddingTable("T", DIM, CAPACITY, device=device,
                                         **cfg["table"])
        SparsePSServer(rank, [table], [worker], chans).serve()
        torch.save(by_key(table), sys.argv[1] + ".ps%d.pt" % rank)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
