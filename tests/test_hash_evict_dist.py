"""A hashed table with the automatic eviction policy behind the stock
SparsePSServer / SparseWorkerClient over gloo: one PS rank (world 2) and two
PS ranks sharding one table (world 3). The PS tables must end equal BY KEY
(rows, optimizer state, use stamps) to a single-process table fed the same
requests, the worker must have pulled the same rows, and its pull of an
evicted key must return the key's initial row. The ranks are
_sparse_evict_proc.py."""

import os
import subprocess
import sys

import pytest
import torch

import _sparse_evict_proc as proc

from tfmesos_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def run_world(world, prefix, coalesce, device="cpu", timeout=180):
    """Start the ranks and wait for each (its own timeout). A rank that
    fails ends the run: its peers are killed."""
    from tfmesos_amd.utils import free_port
    port = free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ)
        env.update({
            "RANK": str(rank), "WORLD_SIZE": str(world),
            "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
            "PYTHONPATH": REPO, "HASH_PROC_DEVICE": device,
            "HASH_PROC_COALESCE": "1" if coalesce else "0",
        })
        if device == "cpu":
            # CPU + gloo is what this covers, also on a GPU box
            env.update({"HIP_VISIBLE_DEVICES": "-1",
                        "CUDA_VISIBLE_DEVICES": "-1"})
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, "_sparse_evict_proc.py"),
             prefix], env=env, stdout=subprocess.PIPE,
            stderr=subprocess.STDOUT, text=True))
    try:
        for p in procs:
            out, _ = p.communicate(timeout=timeout)     # per process
            assert p.returncode == 0, out
    finally:
        # a rank that died must not leave its peers waiting behind
        for p in procs:
            if p.poll() is None:
                p.kill()


def apply_local(world, device="cpu"):
    """The script on a local unsharded table: (table, pulls, the keys that
    had no row just before the final pull of every key)."""
    reqs = proc.requests(world)
    local = proc.make_local(world, device)
    pulls = proc.base.apply_local(local, reqs[:-1], device)
    final = reqs[-1][1].to(device)
    gone = (ops.hash_find(local.index, final) < 0).cpu()
    pulls += proc.base.apply_local(local, reqs[-1:], device)
    return local, pulls, gone


def check_against_local(world, prefix, device="cpu"):
    local, want_pulls, gone = apply_local(world, device)
    want = proc.by_key(local)
    pool = proc.base.key_pool(world)
    row_of = {k: r for r, k in enumerate(want["keys"].tolist())}
    # the script evicted keys, and all 24 are back after the final pull
    assert len(row_of) == 24 and want["dropped"] == 0
    assert want["evicted"] > 0 and 0 < int(gone.sum()) < 24
    seen, evicted = [], 0
    for rank in range(world - 1):
        got = torch.load("%s.ps%d.pt" % (prefix, rank))
        keys = got["keys"].tolist()
        seen += keys
        evicted += got["evicted"]
        if world == 3:      # shard ``rank`` holds its residue class only
            assert keys and all(k % 2 == rank for k in keys)
        rows = torch.tensor([row_of[k] for k in keys])
        assert got["step"] == want["step"] == 10 and got["dropped"] == 0
        assert torch.equal(got["master"], want["master"][rows])
        assert torch.equal(got["last_used"], want["last_used"][rows])
        assert sorted(got["state"]) == sorted(want["state"])
        for k in want["state"]:
            assert torch.equal(got["state"][k], want["state"][k][rows]), k
    assert sorted(seen) == sorted(row_of)       # every key, on one rank
    assert evicted == want["evicted"]
    got_pulls = torch.load(prefix + ".pulls.pt")
    assert len(got_pulls) == len(want_pulls) == 21
    for a, b in zip(got_pulls, want_pulls):
        assert a.dtype == torch.bfloat16 and a.shape == b.shape
        assert torch.equal(a, b.cpu())
    # the worker's pull of an evicted key is the key's initial row
    cfg = proc.base.config(world)["table"]
    init = ops.hash_init_rows(pool, proc.DIM, cfg["seed"]).to(torch.bfloat16)
    assert torch.equal(got_pulls[-1][gone], init[gone])
    assert not torch.equal(got_pulls[-1][~gone], init[~gone])


@pytest.mark.timeout(240)
@pytest.mark.parametrize("world,coalesce", [(2, False), (3, True)],
                         ids=["unsharded_adagrad", "mod_2ps_adam_coalesce"])
def test_evicting_table_over_gloo(world, coalesce, tmp_path):
    prefix = str(tmp_path / "run")
    run_world(world, prefix, coalesce)
    check_against_local(world, prefix)
