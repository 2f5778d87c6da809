"""Helper: one rank of a gloo sparse-PS run (world 2: one PS rank, one worker)
that serves a hashed table WITH FEATURE ADMISSION (admit_after=2) through the
stock SparsePSServer / SparseWorkerClient. Table parameters, key pool and
request script are those of _sparse_hash_proc.py; the PS rank saves its table
BY KEY, the sketch and the ``filtered`` counter included.

usage: _sparse_admit_proc.py OUT_PREFIX
       (HASH_PROC_DEVICE: cpu | cuda:0, HASH_PROC_COALESCE: 0 | 1)
       writes OUT_PREFIX.pulls.pt (worker) and OUT_PREFIX.ps0.pt

Imported by test_hash_admit_dist.py / test_hash_admit_gpu.py for the request
script, so that the tests apply the very same sequence locally."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sparse_hash_proc as base  # noqa: E402
from tfmesos_amd.ps.sparse import (  # noqa: E402
    HashedEmbeddingTable, SparsePSServer, SparseWorkerClient,
    make_sparse_pair_groups)

DIM, CAPACITY = base.DIM, base.CAPACITY
WORLD = 2
POLICY = dict(admit_after=2, admit_width=256)
requests = base.requests


def make_local(device="cpu"):
    return HashedEmbeddingTable("T", DIM, CAPACITY, device=device,
                                **base.config(WORLD)["table"], **POLICY)


def by_key(table):
    """base.by_key plus "filtered" and the sketch's "counters"."""
    out = base.by_key(table)
    out["filtered"] = table.stats()["filtered"]
    out["counters"] = table.sketch.counters.cpu()
    return out


def main():
    import torch.distributed as dist
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    assert world == WORLD
    device = os.environ.get("HASH_PROC_DEVICE", "cpu")
    coalesce = os.environ.get("HASH_PROC_COALESCE", "0") == "1"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = base.config(world)
    worker = world - 1
    chans = make_sparse_pair_groups([0], [worker])
    if rank == worker:
        client = SparseWorkerClient(rank, cfg["homes"], {"T": DIM}, chans,
                                    device=device, coalesce=coalesce)
        pulled = []
        for method, *args in requests(world):
            res = getattr(client, method)("T", *args)
            if method.startswith("pull"):
                pulled.append(res.cpu())
        client.done_all()
        torch.save(pulled, sys.argv[1] + ".pulls.pt")
    else:
        table = make_local(device)
        SparsePSServer(rank, [table], [worker], chans).serve()
        torch.save(by_key(table), sys.argv[1] + ".ps%d.pt" % rank)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
