"""Row-sharded embedding tables over gloo: the worker/server protocol
(kind-2 row requests to every shard, pooled requests per shard) against
the same request script applied to local tables."""

import os
import subprocess
import sys

import pytest
import torch

import _sparse_shard_proc as proc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def run_world(world, pulls, device="cpu", timeout=180):
    """Start the ranks, return {"name/shard": digest} printed by the PS
    ranks. A rank that fails ends the run: its peers are killed."""
    from tfmesos_amd.utils import free_port
    port = free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ)
        env.update({
            "RANK": str(rank), "WORLD_SIZE": str(world),
            "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
            "PYTHONPATH": REPO, "SHARD_PROC_DEVICE": device,
        })
        if device == "cpu":
            # CPU + gloo is what this covers, also on a GPU box
            env.update({"HIP_VISIBLE_DEVICES": "-1",
                        "CUDA_VISIBLE_DEVICES": "-1"})
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, "_sparse_shard_proc.py"),
             pulls], env=env, stdout=subprocess.PIPE, text=True))
    sums = {}
    try:
        for p in procs:
            out, _ = p.communicate(timeout=timeout)     # per process
            assert p.returncode == 0, out
            for line in out.splitlines():
                if line.startswith("CHECKSUM"):
                    _, name, digest = line.split()
                    sums[name] = digest
    finally:
        # a rank that died must not leave its peers waiting behind
        for p in procs:
            if p.poll() is None:
                p.kill()
    return sums


def check_against_local(world, sums, pulls, device="cpu"):
    reqs = proc.requests(world)
    local = proc.make_local(world, device)
    init = proc.local_checksums(local)
    want = proc.apply_local(local, reqs, device)
    assert sums == proc.local_checksums(local)
    assert all(sums[k] != init[k] for k in sums)
    got = torch.load(pulls)
    assert len(got) == len(want) == sum(
        1 for r in reqs if r[0].startswith("pull"))
    for a, b in zip(got, want):
        assert a.dtype == torch.bfloat16 and torch.equal(a, b.cpu())
    return local, reqs


@pytest.mark.timeout(240)
@pytest.mark.parametrize("world", [3, 4], ids=["mod_2ps_plus_unsharded",
                                               "div_3ps"])
def test_sharded_protocol_over_gloo(world, tmp_path):
    """The PS ranks end with the state of local shard tables given the same
    requests, the worker pulls what ShardedEmbeddingTable pulls, and the
    unsharded table beside it behaves as a plain EmbeddingTable."""
    pulls = str(tmp_path / "pulls.pt")
    sums = run_world(world, pulls)
    cfg = proc.config(world)
    assert sorted(sums) == sorted(
        "%s/%d" % (n, s) for n, h in cfg["homes"].items()
        for s in range(len(h) if isinstance(h, list) else 1))
    local, reqs = check_against_local(world, sums, pulls)
    # every shard stepped once per push, also for the one-shard push
    n_push = sum(1 for r in reqs if r[0].startswith("push") and r[1] == "S")
    assert [t.step for t in local["S"].shards] == \
        [n_push] * len(cfg["homes"]["S"])
    if "U" in local:
        from tfmesos_amd.ps.sparse import EmbeddingTable
        plain = EmbeddingTable("U", **cfg["tables"]["U"])
        proc.apply_local({"U": plain}, [r for r in reqs if r[1] == "U"])
        assert sums["U/0"] == proc.checksum(plain)
