"""SparseNMF trained with an Adagrad embedding-table optimizer over the
sparse PS — 3-process gloo run on CPU (2 ps + 1 worker)."""

import math
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

ADAGRAD_LR = 0.01


@pytest.mark.timeout(240)
def test_sparse_nmf_adagrad_loss_decreases():
    """n=300, rank 32, batch 64, 20 steps, optimizer="adagrad".

    lr = 0.01 was picked by running this configuration on the CPU.
    Adagrad's first step moves every touched element by ~lr whatever
    the gradient's size, and the factors start around 1/sqrt(32) ~ 0.18,
    so the step has to stay well under that. Measured first-quarter ->
    last-quarter mean loss: lr 0.01: 2.4e-3 -> 7.2e-4 (steady descent);
    0.02: 2.7e-3 -> 7.8e-4; 0.05: 8.6e-3 -> 3.8e-3 and 0.1: 3.3e-2 ->
    1.5e-2 (both overshoot on the first steps, then recover)."""
    from tfmesos_amd.utils import free_port
    port = free_port()
    script = os.path.join(HERE, "_sparse_opt_proc.py")
    procs = []
    for rank in range(3):
        env = dict(os.environ)
        env.update({
            "RANK": str(rank), "WORLD_SIZE": "3",
            "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
            "PYTHONPATH": REPO,
            # CPU + gloo is what this test covers, also on a GPU box
            "HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1",
        })
        procs.append(subprocess.Popen(
            [sys.executable, script, "20", "adagrad", str(ADAGRAD_LR)],
            env=env, stdout=subprocess.PIPE, text=True))
    losses = None
    try:
        for p in procs:
            out, _ = p.communicate(timeout=180)
            assert p.returncode == 0, out
            if "LOSSES" in out:
                losses = [float(x) for x in
                          out.split("LOSSES")[1].split()]
    finally:
        # a rank that died must not leave its peers waiting behind
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert losses is not None and len(losses) == 20
    assert all(math.isfinite(v) for v in losses), losses
    k = len(losses) // 4
    first, last = sum(losses[:k]) / k, sum(losses[-k:]) / k
    print("adagrad lr=%g: first-quarter %g last-quarter %g"
          % (ADAGRAD_LR, first, last))
    assert last < first, losses
