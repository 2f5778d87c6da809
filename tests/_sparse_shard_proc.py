"""Helper: one rank of a gloo sparse-PS run against a ROW-SHARDED table.
World 3 = 2 PS ranks holding one "mod"-sharded Adagrad table "S" (plus an
unsharded Adam table "U" on rank 0) + one worker; world 4 = 3 PS ranks
holding one "div"-sharded Adam table "S" + one worker. The worker
interleaves row and pooled requests; every PS rank prints a checksum of
every table (shard) it holds; the worker saves what it pulled.

usage: _sparse_shard_proc.py PULLS_OUT.pt     (SHARD_PROC_DEVICE: cpu | cuda:0)

Imported by test_shard_dist.py / test_shard_partition_gpu.py for the
request script, so that the tests apply the very same sequence locally."""

import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd.ps.sparse import (  # noqa: E402
    EmbeddingTable, ShardedEmbeddingTable, SparsePSServer,
    SparseWorkerClient, make_sparse_pair_groups)

V = 97
# multiples of 6 below 33: shard 0 under "mod" for 2 and 3 shards, and
# under "div" for 3 shards (shard 0 = rows 0..32) — a push that hits no
# row of the other shards
ONE_SHARD_IDS = [0, 6, 12, 18, 24, 30, 6, 0]


def config(world):
    """homes / strategy / constructor arguments by world size."""
    if world == 3:
        return dict(
            homes={"S": [0, 1], "U": 0}, strategy="mod",
            tables={"S": dict(rows=V, dim=8, lr=0.1, seed=21,
                              optimizer="adagrad"),
                    "U": dict(rows=40, dim=12, lr=0.05, seed=22,
                              optimizer="adam")})
    return dict(
        homes={"S": [0, 1, 2]}, strategy="div",
        tables={"S": dict(rows=V, dim=8, lr=0.05, seed=23,
                          optimizer="adam")})


def requests(world):
    """The fixed request script: (method, table, args...). Gradients are
    dyadic (randint/16), so the bf16 wire format carries them exactly."""
    cfg = config(world)
    names = sorted(cfg["tables"])
    gen = torch.Generator().manual_seed(5 + world)
    reqs = []
    modes = [("sum", False), ("mean", True), ("sum", True), ("mean", False)]
    for k in range(8):
        name = names[k % len(names)]
        rows, dim = cfg["tables"][name]["rows"], cfg["tables"][name]["dim"]
        combiner, weighted = modes[(k // len(names)) % 4]
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
        if k == 2:
            one = torch.tensor(ONE_SHARD_IDS)
            g = torch.randint(-32, 33, (one.numel(), 8),
                              generator=gen).float() / 16
            reqs.append(("push", "S", one, g))
            reqs.append(("pull", "S", one))
    return reqs


def make_local(world, device="cpu"):
    """{name: table} holding what the PS ranks hold, in one process."""
    cfg = config(world)
    out = {}
    for name, kw in cfg["tables"].items():
        home = cfg["homes"][name]
        if isinstance(home, list):
            out[name] = ShardedEmbeddingTable(
                name, num_shards=len(home), strategy=cfg["strategy"],
                device=device, **kw)
        else:
            out[name] = EmbeddingTable(name, device=device, **kw)
    return out


def apply_local(tables, reqs, device="cpu"):
    """The request script on local tables; pushes see bf16 gradients, as
    over the wire. Returns the pulled tensors."""
    def dev(t):
        return t.to(device) if torch.is_tensor(t) else t
    pulled = []
    for method, name, *args in reqs:
        t = tables[name]
        args = [dev(a) for a in args]
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
        h.update(t.cpu().numpy().tobytes())
    h.update(str(table.step).encode())
    return h.hexdigest()


def local_checksums(tables):
    """{"name/shard": digest} as the PS ranks print them."""
    out = {}
    for name, t in tables.items():
        if isinstance(t, ShardedEmbeddingTable):
            for s, shard in enumerate(t.shards):
                out["%s/%d" % (name, s)] = checksum(shard)
        else:
            out["%s/0" % name] = checksum(t)
    return out


def main():
    import torch.distributed as dist
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    device = os.environ.get("SHARD_PROC_DEVICE", "cpu")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = config(world)
    ps_ranks = list(range(world - 1))
    worker = world - 1
    chans = make_sparse_pair_groups(ps_ranks, [worker])
    if rank == worker:
        client = SparseWorkerClient(
            rank, cfg["homes"],
            {n: kw["dim"] for n, kw in cfg["tables"].items()}, chans,
            device=device,
            rows={n: kw["rows"] for n, kw in cfg["tables"].items()
                  if isinstance(cfg["homes"][n], list)},
            strategy=cfg["strategy"])
        pulled = []
        for method, name, *args in requests(world):
            out = getattr(client, method)(name, *args)
            if out is not None:
                pulled.append(out.cpu())
        client.done_all()
        torch.save(pulled, sys.argv[1])
    else:
        tables, shard_no = [], {}
        for name in sorted(cfg["tables"]):
            home, kw = cfg["homes"][name], cfg["tables"][name]
            if isinstance(home, list) and rank in home:
                s = home.index(rank)
                kw = dict(kw)
                rows, dim = kw.pop("rows"), kw.pop("dim")
                tables.append(EmbeddingTable.shard_of(
                    name, rows, dim, s, len(home), cfg["strategy"],
                    device=device, **kw))
                shard_no[name] = s
            elif home == rank:
                tables.append(EmbeddingTable(name, device=device, **kw))
                shard_no[name] = 0
        SparsePSServer(rank, tables, [worker], chans).serve()
        for t in tables:
            print("CHECKSUM %s/%d %s" % (t.name, shard_no[t.name],
                                         checksum(t)))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
