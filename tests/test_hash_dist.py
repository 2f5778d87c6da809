"""A hashed table behind the stock SparsePSServer / SparseWorkerClient over
gloo: one PS rank (world 2) and two PS ranks sharding one table (world 3),
with and without worker-side coalescing. The PS tables must end equal BY
KEY to a single-process HashedEmbeddingTable fed the same requests, and the
worker must have pulled the same rows. The ranks are _sparse_hash_proc.py."""

import os
import subprocess
import sys

import pytest
import torch

import _sparse_hash_proc as proc

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
            [sys.executable, os.path.join(HERE, "_sparse_hash_proc.py"),
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


def check_against_local(world, prefix, device="cpu"):
    """PS tables by key, step and pulls against one local unsharded table
    given the uncoalesced script."""
    reqs = proc.requests(world)
    local = proc.make_local(world, device)
    want_pulls = proc.apply_local(local, reqs, device)
    want = proc.by_key(local)
    row_of = {k: r for r, k in enumerate(want["keys"].tolist())}
    assert len(row_of) == 24 and want["dropped"] == 0
    seen = []
    for rank in range(world - 1):
        got = torch.load("%s.ps%d.pt" % (prefix, rank))
        keys = got["keys"].tolist()
        seen += keys
        if world == 3:      # shard ``rank`` holds its residue class only
            assert keys and all(k % 2 == rank for k in keys)
        rows = torch.tensor([row_of[k] for k in keys])
        assert got["step"] == want["step"] == 6 and got["dropped"] == 0
        assert torch.equal(got["master"], want["master"][rows])
        assert sorted(got["state"]) == sorted(want["state"])
        for k in want["state"]:
            assert torch.equal(got["state"][k], want["state"][k][rows]), k
    assert sorted(seen) == sorted(row_of)       # every key, on one rank
    init = proc.make_local(world).pull(want["keys"])
    assert not torch.equal(want["master"].to(torch.bfloat16), init)
    got_pulls = torch.load(prefix + ".pulls.pt")
    assert len(got_pulls) == len(want_pulls) == 13
    for a, b in zip(got_pulls, want_pulls):
        assert a.dtype == torch.bfloat16 and a.shape == b.shape
        assert torch.equal(a, b.cpu())


@pytest.mark.timeout(240)
@pytest.mark.parametrize("coalesce", [True, False], ids=["coalesce", "plain"])
@pytest.mark.parametrize("world", [2, 3], ids=["unsharded_adagrad",
                                               "mod_2ps_adam"])
def test_hashed_table_over_gloo(world, coalesce, tmp_path):
    prefix = str(tmp_path / "run")
    run_world(world, prefix, coalesce)
    check_against_local(world, prefix)
