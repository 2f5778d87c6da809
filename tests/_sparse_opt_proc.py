"""Helper: one rank of a 3-process sparse NMF run with a non-SGD table
optimizer; the worker prints every minibatch loss.

usage: _sparse_opt_proc.py STEPS OPTIMIZER LR"""

import os
import sys

import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd.models.nmf import SparseNMF  # noqa: E402


def main():
    steps = int(sys.argv[1])
    optimizer = sys.argv[2]
    lr = float(sys.argv[3])
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    wl = SparseNMF(rank, world, n=300, factor_rank=32, batch=64, lr=lr,
                   optimizer=optimizer)
    for _ in range(steps):
        wl.one_step()
    wl.finalize()
    if not wl.is_ps:
        print("LOSSES " + " ".join("%r" % v for v in wl.losses))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
