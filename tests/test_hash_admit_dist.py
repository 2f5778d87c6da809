"""A hashed table with feature admission (admit_after=2) behind the stock
SparsePSServer / SparseWorkerClient over gloo, one PS rank and one worker,
with and without worker-side coalescing. Both runs must end bit-identical,
BY KEY, to a single-process table fed the uncoalesced requests — rows,
optimizer state, the sketch's counters and ``filtered`` — and the worker must
have pulled the same rows: a request counts a key once, whatever the number
of its occurrences. The ranks are _sparse_admit_proc.py."""

import os
import subprocess
import sys

import pytest
import torch

import _sparse_admit_proc as proc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def run_world(prefix, coalesce, device="cpu", timeout=180):
    """Start the ranks and wait for each (its own timeout). A rank that
    fails ends the run: its peers are killed."""
    from tfmesos_amd.utils import free_port
    port = free_port()
    procs = []
    for rank in range(proc.WORLD):
        env = dict(os.environ)
        env.update({
            "RANK": str(rank), "WORLD_SIZE": str(proc.WORLD),
            "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
            "PYTHONPATH": REPO, "HASH_PROC_DEVICE": device,
            "HASH_PROC_COALESCE": "1" if coalesce else "0",
        })
        if device == "cpu":
            # CPU + gloo is what this covers, also on a GPU box
            env.update({"HIP_VISIBLE_DEVICES": "-1",
                        "CUDA_VISIBLE_DEVICES": "-1"})
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, "_sparse_admit_proc.py"),
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


def check_against_local(prefix, device="cpu"):
    reqs = proc.requests(proc.WORLD)
    local = proc.make_local(device)
    want_pulls = proc.base.apply_local(local, reqs, device)
    want = proc.by_key(local)
    row_of = {k: r for r, k in enumerate(want["keys"].tolist())}
    # admission did filter, and did admit
    assert 0 < len(row_of) <= 24 and want["filtered"] > 0
    assert want["dropped"] == 0 and int(want["counters"].sum()) > 0
    got = torch.load(prefix + ".ps0.pt")
    keys = got["keys"].tolist()
    assert sorted(keys) == sorted(row_of)
    rows = torch.tensor([row_of[k] for k in keys])
    assert got["step"] == want["step"] == 6 and got["dropped"] == 0
    assert got["filtered"] == want["filtered"]
    assert torch.equal(got["counters"], want["counters"])
    assert torch.equal(got["master"], want["master"][rows])
    assert sorted(got["state"]) == sorted(want["state"])
    for k in want["state"]:
        assert torch.equal(got["state"][k], want["state"][k][rows]), k
    got_pulls = torch.load(prefix + ".pulls.pt")
    assert len(got_pulls) == len(want_pulls) == 13
    for a, b in zip(got_pulls, want_pulls):
        assert a.dtype == b.dtype == torch.bfloat16 and a.shape == b.shape
        assert torch.equal(a, b.cpu())


@pytest.mark.timeout(240)
@pytest.mark.parametrize("coalesce", [True, False], ids=["coalesce", "plain"])
def test_admitting_table_over_gloo(coalesce, tmp_path):
    prefix = str(tmp_path / "run")
    run_world(prefix, coalesce)
    check_against_local(prefix)
