"""Unit tests for the small utility subsystems (metrics, hipGraph step
capture fallback, wire edge cases)."""

import pytest
import torch

from tfmesos_amd import wire
from tfmesos_amd.utils.graphstep import GraphedStep
from tfmesos_amd.utils.metrics import StepTimer


def test_step_timer_counts_and_reports():
    lines = []
    t = StepTimer(report_every=10, emit=lines.append, prefix="w0 ").start()
    for _ in range(25):
        t.step()
    s = t.summary()
    assert s["steps"] == 25
    assert s["steps_per_sec"] > 0
    assert len(lines) == 2 and lines[0].startswith("w0 step 10")


def test_graphed_step_cpu_fallback_runs_eagerly(monkeypatch):
    # the CPU fallback is what is under test, also on a box with a GPU
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    calls = []
    g = GraphedStep(lambda: calls.append(1))
    assert g.graph is None          # no GPU here
    g()
    g()
    assert len(calls) == 2


def test_wire_rejects_tampered_frame():
    import socket
    a, b = socket.socketpair()
    try:
        wire.send_msg(a, {"x": 1}, b"secret")
        raw = b.recv(65536)
        # flip a payload byte and replay
        tampered = raw[:-1] + bytes([raw[-1] ^ 0xFF])
        a2, b2 = socket.socketpair()
        a2.sendall(tampered)
        with pytest.raises(wire.AuthError):
            wire.recv_msg(b2, b"secret")
        a2.close()
        b2.close()
    finally:
        a.close()
        b.close()


def test_wire_rejects_wrong_secret():
    import socket
    a, b = socket.socketpair()
    try:
        wire.send_msg(a, "hello", b"key1")
        with pytest.raises(wire.AuthError):
            wire.recv_msg(b, b"key2")
    finally:
        a.close()
        b.close()


def test_wire_bf16_tensor_roundtrip():
    buf = wire.pack({"t": torch.randn(3, 4).to(torch.bfloat16)})
    out = wire.unpack(buf)
    assert out["t"].dtype == torch.bfloat16 and out["t"].shape == (3, 4)


def test_scheduler_rendezvous_timeout():
    from tfmesos_amd import Job, LocalScheduler

    class NeverLaunch:
        def start(self, listener):
            pass

        def stop(self):
            pass

        def suppress(self):
            pass

        def revive(self):
            pass

        def decline(self, offer):
            pass

    s = LocalScheduler([Job(name="w", num=1)], quiet=True,
                       backend=NeverLaunch(), start_timeout=1.0)
    with pytest.raises(RuntimeError, match="rendezvous timed out"):
        s.start()
