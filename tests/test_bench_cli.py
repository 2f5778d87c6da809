"""bench.py command line: --steps/ms_per_step, --dump-outputs, --full
(CPU dev run; the GPU is hidden from the child so the test means the
same on every box)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _bench(*argv):
    env = dict(os.environ, PYTHONPATH=REPO, HIP_VISIBLE_DEVICES="-1",
               CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", "7", "--warmup", "2"] + list(argv),
        env=env, cwd=REPO, capture_output=True, timeout=120, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout      # ONE result line
    return json.loads(lines[0])


@pytest.mark.timeout(300)
def test_dump_outputs_repeatable_and_full_accepted(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    ra = _bench("--dump-outputs", a)
    rb = _bench("--full", "--dump-outputs", b)
    for r in (ra, rb):
        assert r["steps"] == 7 and r["unit"] == "steps/s"
        assert r["higher_is_better"] is True
        # ms_per_step is one timed step: consistent with steps/s
        assert r["ms_per_step"] == pytest.approx(1000.0 / r["value"])
    names = sorted(os.listdir(a))
    assert names == ["hid_b.npy", "hid_w.npy", "loss.npy", "sm_b.npy",
                     "sm_w.npy"]
    assert sorted(os.listdir(b)) == names
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n    # same arguments, same outputs
    assert np.load(os.path.join(a, "hid_w.npy")).shape == (784, 100)

    # the dumped parameters are those after warmup + steps SGD steps
    from tfmesos_amd.models.mlp import MnistMLP, synthetic_batch
    from tfmesos_amd.ps.replica import SyncReplicaTrainer
    m = MnistMLP()
    t = SyncReplicaTrainer(m.init_params(), optimizer="sgd",
                           hparams={"lr": 0.01}, device="cpu")
    xb, yb = synthetic_batch(100, seed=1000)
    for _ in range(9):
        loss = m.fwd_bwd(t.store.view, xb, yb, t.grad_view)
        t.step()
    assert np.array_equal(np.load(os.path.join(a, "sm_w.npy")),
                          t.store.view("sm_w").numpy())
    assert float(np.load(os.path.join(a, "loss.npy"))) == float(loss)


def test_dump_outputs_samples_large_arrays(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4096)
    big = torch.arange(10000, dtype=torch.float64)
    small = torch.ones(3, 5, dtype=torch.bfloat16)
    for d in ("p", "q"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    p = np.load(str(tmp_path / "p" / "big.npy"))
    assert p.dtype == np.float64 and p.nbytes <= 2048
    assert len(np.unique(p)) == p.size and (np.diff(p) > 0).all()
    assert np.array_equal(p, np.load(str(tmp_path / "q" / "big.npy")))
    s = np.load(str(tmp_path / "p" / "small.npy"))
    assert s.dtype == np.float32 and s.shape == (3, 5)
    total = sum(os.path.getsize(str(tmp_path / "p" / f))
                for f in os.listdir(str(tmp_path / "p")))
    assert total <= 4096 + 2 * 128        # budget + .npy headers
