""""ftrl_proximal" tables behind the sparse PS over gloo, on the CPU: a
3-process SparseNMF run (2 ps + 1 worker, _sparse_opt_proc.py) whose loss
must fall, and a world-2 run (_sparse_ftrl_proc.py) after which the
PS-resident dense and hashed tables must equal in-process tables fed the
same requests."""

import math
import os
import subprocess
import sys

import pytest
import torch

import _sparse_ftrl_proc as proc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

FTRL_LR = 0.1


def run_ranks(script, args, world, timeout=180):
    """Start the ranks and wait for each; returns their outputs. A rank
    that fails ends the run: its peers are killed."""
    from tfmesos_amd.utils import free_port
    port = free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ)
        env.update({
            "RANK": str(rank), "WORLD_SIZE": str(world),
            "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
            "PYTHONPATH": REPO,
            # CPU + gloo is what this covers, also on a GPU box
            "HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1",
        })
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, script)] + args, env=env,
            stdout=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=timeout)     # per process
            assert p.returncode == 0, out
            outs.append(out)
    finally:
        # a rank that died must not leave its peers waiting behind
        for p in procs:
            if p.poll() is None:
                p.kill()
    return outs


@pytest.mark.timeout(240)
def test_sparse_nmf_ftrl_proximal_loss_decreases():
    """n=300, rank 32, batch 64, 20 steps, optimizer="ftrl_proximal" with
    its default hyper-parameters (l1 = l2 = 0, initial accumulator 0.1).

    lr = 0.1 was picked by running this configuration on the CPU. The first
    touch seeds the linear term from the initial factors, so the run starts
    where SGD would (first loss 3.3e-3) and every lr tried descends; the
    per-coordinate step is lr * g / sqrt(0.1 + sum g^2), small while the
    gradients are. Measured first-quarter -> last-quarter mean loss: lr
    0.005: 3.0e-3 -> 2.8e-3; 0.01: 3.0e-3 -> 2.7e-3; 0.02: 3.0e-3 ->
    2.4e-3; 0.05: 2.9e-3 -> 1.9e-3; 0.1: 2.7e-3 -> 1.3e-3 (steady
    descent); 0.2: 2.5e-3 -> 8.3e-4; 0.5: 2.3e-3 -> 5.1e-4; 1.0: 2.4e-3 ->
    1.3e-3 (the loss jumps between steps)."""
    outs = run_ranks("_sparse_opt_proc.py",
                     ["20", "ftrl_proximal", str(FTRL_LR)], 3)
    losses = None
    for out in outs:
        if "LOSSES" in out:
            losses = [float(x) for x in out.split("LOSSES")[1].split()]
    assert losses is not None and len(losses) == 20
    assert all(math.isfinite(v) for v in losses), losses
    k = len(losses) // 4
    first, last = sum(losses[:k]) / k, sum(losses[-k:]) / k
    print("ftrl_proximal lr=%g: first-quarter %g last-quarter %g"
          % (FTRL_LR, first, last))
    assert last < first, losses


@pytest.mark.timeout(240)
def test_ps_resident_tables_equal_in_process_tables(tmp_path):
    prefix = str(tmp_path / "run")
    run_ranks("_sparse_ftrl_proc.py", [prefix], 2)
    local = proc.make_tables()
    want_pulls = proc.apply_local(local, proc.requests())
    got = torch.load(prefix + ".ps.pt")
    for name, t in local.items():
        want = t.state_dict()
        assert got[name]["optimizer"] == "ftrl_proximal"
        assert got[name]["step"] == want["step"] == 6
        assert torch.equal(got[name]["master"], want["master"]), name
        assert sorted(got[name]["state"]) == ["accum", "linear"]
        for k in ("accum", "linear"):
            assert torch.equal(got[name]["state"][k], want["state"][k]), k
            assert want["state"][k].any()
        assert (want["master"] == 0).any()      # l1 at work on the PS too
    assert torch.equal(got["H"]["keys"], local["H"].state_dict()["keys"])
    assert got["H"]["keys"].numel() == proc.KEYS.numel()
    got_pulls = torch.load(prefix + ".pulls.pt")
    assert len(got_pulls) == len(want_pulls) == 12
    for a, b in zip(got_pulls, want_pulls):
        assert a.dtype == torch.bfloat16 and torch.equal(a, b)
