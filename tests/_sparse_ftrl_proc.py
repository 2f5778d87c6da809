"""Helper: one rank of a world-2 gloo sparse-PS run whose PS (rank 0) holds
two "ftrl_proximal" tables behind the stock SparsePSServer — "D", an
EmbeddingTable, and "H", a HashedEmbeddingTable — and whose worker (rank 1)
sends a fixed request script through the stock SparseWorkerClient. The PS
saves both tables.

usage: _sparse_ftrl_proc.py OUT_PREFIX
       writes OUT_PREFIX.pulls.pt (worker) and OUT_PREFIX.ps.pt (PS)

Imported by test_sparse_ftrl_dist.py for the tables and the script, so that
the test applies the very same sequence in process."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd.ps.sparse import (  # noqa: E402
    EmbeddingTable, HashedEmbeddingTable, SparsePSServer, SparseWorkerClient,
    make_sparse_pair_groups)

ROWS, DIM, CAPACITY, N, BAGS = 40, 8, 64, 24, 6
HP = dict(lr=0.1, optimizer="ftrl_proximal", l1=0.5, l2=0.01,
          initial_accumulator_value=0.1)
KEYS = torch.tensor([3, -17, 2 ** 40 + 5, 99, 123456789, 7, 2 ** 61 + 1, 11])


def make_tables():
    return {"D": EmbeddingTable("D", ROWS, DIM, seed=4, **HP),
            "H": HashedEmbeddingTable("H", DIM, CAPACITY, seed=5, **HP)}


def requests():
    """Per round and table: pull, push (duplicate ids), pooled push (mean,
    weights), pooled pull. Gradients randint(-8, 9)/4: exact in bf16, the
    wire dtype."""
    gen = torch.Generator().manual_seed(77)

    def grads(n):
        return torch.randint(-8, 9, (n, DIM), generator=gen).float() / 4

    reqs = []
    for _ in range(3):
        for name in ("D", "H"):
            pick = torch.randint(0, ROWS if name == "D" else KEYS.numel(),
                                 (N,), generator=gen)
            ids = pick if name == "D" else KEYS[pick]
            lens = torch.randint(0, 9, (BAGS,), generator=gen)
            offsets = torch.cat([torch.tensor([0]), lens.cumsum(0)])
            bag_ids = ids[torch.randint(0, N, (int(offsets[-1]),),
                                        generator=gen)]
            w = torch.randint(1, 5, (bag_ids.numel(),), generator=gen) / 4
            reqs += [("pull", name, ids),
                     ("push", name, ids, grads(N)),
                     ("push_pooled", name, bag_ids, offsets, grads(BAGS), w,
                      "mean"),
                     ("pull_pooled", name, bag_ids, offsets, w, "mean")]
    return reqs


def apply_local(tables, reqs):
    """The script on in-process tables; pushes see bf16 gradients, as over
    the wire. Returns the pulled tensors."""
    pulled = []
    for method, name, *args in reqs:
        t = tables[name]
        if method == "push":
            t.push(args[0], args[1].to(torch.bfloat16))
        elif method == "push_pooled":
            k, o, g, w, comb = args
            t.push_pooled(k, o, g.to(torch.bfloat16), w, comb)
        else:
            pulled.append(getattr(t, method)(*args))
    return pulled


def main():
    import torch.distributed as dist
    rank = int(os.environ["RANK"])
    dist.init_process_group("gloo", rank=rank, world_size=2)
    chans = make_sparse_pair_groups([0], [1])
    if rank == 1:
        client = SparseWorkerClient(1, {"D": 0, "H": 0},
                                    {"D": DIM, "H": DIM}, chans)
        pulled = []
        for method, *args in requests():
            res = getattr(client, method)(*args)
            if method.startswith("pull"):
                pulled.append(res.cpu())
        client.done_all()
        torch.save(pulled, sys.argv[1] + ".pulls.pt")
    else:
        tables = make_tables()
        SparsePSServer(0, list(tables.values()), [1], chans).serve()
        torch.save({k: t.state_dict() for k, t in tables.items()},
                   sys.argv[1] + ".ps.pt")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
