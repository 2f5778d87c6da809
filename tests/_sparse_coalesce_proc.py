"""Helper: one rank of a gloo sparse-PS run whose worker COALESCES its row
requests. World 2 = one PS rank holding one unsharded Adagrad table "T" +
one worker; world 3 = 2 PS ranks holding one "mod"-sharded Adam table "T" +
one worker. The worker runs a fixed script of pulls and pushes with
``coalesce`` on (COALESCE_PROC_ON=1) or off; every PS rank counts the ids
its table is handed per call ("SEEN" lines) and prints a checksum of the
table (shard) it holds; the worker saves what it pulled.

usage: _sparse_coalesce_proc.py PULLS_OUT.pt
       (COALESCE_PROC_DEVICE: cpu | cuda:0, COALESCE_PROC_ON: 0 | 1)

Imported by test_coalesce.py / test_coalesce_gpu.py for the request script,
so that the tests apply the very same sequence locally."""

import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd.ps.sparse import (  # noqa: E402
    EmbeddingTable, ShardedEmbeddingTable, SparsePSServer,
    SparseWorkerClient, make_sparse_pair_groups)

V = 97
DIM = 8
N = 40                                  # positions per request
ROWS = [3 + 7 * k for k in range(12)]   # the 12 rows the ids come from
EVEN_ROWS = [r for r in ROWS if r % 2 == 0]     # shard 0 under "mod", S = 2


def config(world):
    """homes / strategy / constructor arguments by world size."""
    if world == 2:
        return dict(homes={"T": 0}, strategy="mod",
                    table=dict(rows=V, dim=DIM, lr=0.1, seed=31,
                               optimizer="adagrad"))
    return dict(homes={"T": [0, 1]}, strategy="mod",
                table=dict(rows=V, dim=DIM, lr=0.05, seed=32,
                           optimizer="adam"))


def requests(world):
    """The fixed request script: (method, ids[, grads]). Gradients are
    randint(-4, 5)/16: a per-id sum over at most 40 positions is a multiple
    of 1/16 of magnitude <= 10, exact in bf16, so the PS receives the same
    per-id totals with and without coalescing. One push (and pull) draws
    from the even rows only: a single shard of the sharded table. The
    unsharded world also goes through pull_many / push_many."""
    gen = torch.Generator().manual_seed(40 + world)

    def draw(rows):
        ids = torch.tensor(rows)[torch.randint(0, len(rows), (N,),
                                               generator=gen)]
        g = torch.randint(-4, 5, (N, DIM), generator=gen).float() / 16
        return ids, g

    reqs = []
    for k in range(3):
        ids, g = draw(ROWS)
        reqs += [("pull", ids), ("push", ids, g), ("pull", ids)]
        if k == 1:
            one, g1 = draw(EVEN_ROWS)
            reqs += [("push", one, g1), ("pull", one)]
    if world == 2:
        ids, g = draw(ROWS)
        reqs += [("pull_many", ids), ("push_many", ids, g), ("pull", ids)]
    return reqs


def make_local(world, device="cpu"):
    """The table the PS ranks hold, in one process."""
    cfg = config(world)
    home = cfg["homes"]["T"]
    if isinstance(home, list):
        return ShardedEmbeddingTable("T", num_shards=len(home),
                                     strategy=cfg["strategy"], device=device,
                                     **cfg["table"])
    return EmbeddingTable("T", device=device, **cfg["table"])


def apply_local(table, reqs, device="cpu"):
    """The UNCOALESCED script on a local table; pushes see bf16 gradients,
    as over the wire. Returns the pulled tensors."""
    pulled = []
    for method, ids, *g in reqs:
        ids = ids.to(device)
        if method.startswith("pull"):
            pulled.append(table.pull(ids))
        else:
            table.push(ids, g[0].to(device=device, dtype=torch.bfloat16))
    return pulled


def expected_seen(world, coalesce):
    """{"T/shard": [(kind, ids handed to the table)]} in script order:
    the distinct ids of each request (positions without coalescing), per
    owning shard; a pull skips a shard it has no ids for, a push does not."""
    home = config(world)["homes"]["T"]
    S = len(home) if isinstance(home, list) else 1
    seen = {"T/%d" % s: [] for s in range(S)}
    for method, ids, *_ in requests(world):
        kind = method.split("_")[0]
        items = ids.tolist()
        if coalesce:
            items = set(items)
        for s in range(S):
            cnt = sum(1 for i in items if i % S == s)
            if cnt or kind == "push":
                seen["T/%d" % s].append((kind, cnt))
    return seen


def distinct(ids):
    return len(set(ids.tolist()))


def checksum(table):
    h = hashlib.sha256()
    for t in [table.master] + [table.state[k] for k in sorted(table.state)]:
        h.update(t.cpu().numpy().tobytes())
    h.update(str(table.step).encode())
    return h.hexdigest()


def local_checksums(table):
    """{"T/shard": digest} as the PS ranks print them."""
    shards = table.shards if isinstance(table, ShardedEmbeddingTable) \
        else [table]
    return {"T/%d" % s: checksum(t) for s, t in enumerate(shards)}


def count_ids(table, tag):
    """Wrap the table's pull / push: print how many ids each call gets."""
    pull, push = table.pull, table.push

    def counted_pull(ids):
        print("SEEN %s pull %d" % (tag, ids.numel()))
        return pull(ids)

    def counted_push(ids, grads, lr=None):
        print("SEEN %s push %d" % (tag, ids.numel()))
        return push(ids, grads, lr)

    table.pull, table.push = counted_pull, counted_push


def main():
    import torch.distributed as dist
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    device = os.environ.get("COALESCE_PROC_DEVICE", "cpu")
    coalesce = os.environ.get("COALESCE_PROC_ON", "1") == "1"
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
            rows={"T": V} if sharded else None, strategy=cfg["strategy"],
            coalesce=coalesce)
        pulled = []
        for method, ids, *g in requests(world):
            if method == "pull":
                pulled.append(client.pull("T", ids).cpu())
            elif method == "push":
                client.push("T", ids, g[0])
            elif method == "pull_many":
                pulled.append(client.pull_many([("T", ids)])[0].cpu())
            else:
                client.push_many([("T", ids, g[0])])
        client.done_all()
        torch.save(pulled, sys.argv[1])
    else:
        kw = dict(cfg["table"])
        if sharded:
            rows, dim = kw.pop("rows"), kw.pop("dim")
            shard = home.index(rank)
            table = EmbeddingTable.shard_of("T", rows, dim, shard, len(home),
                                            cfg["strategy"], device=device,
                                            **kw)
        else:
            shard = 0
            table = EmbeddingTable("T", device=device, **kw)
        count_ids(table, "T/%d" % shard)
        SparsePSServer(rank, [table], [worker], chans).serve()
        print("CHECKSUM T/%d %s" % (shard, checksum(table)))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
