"""CPU reference path of the fused head+tail ops and the model plumbing
that routes through them (the GPU kernel is covered by
test_mlp_headtail_gpu.py)."""

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.models.mlp import MnistMLP, synthetic_batch
from tfmesos_amd.ps.replica import SyncReplicaTrainer

SHAPES = [(100, 784, 100, 10), (7, 33, 4, 1)]


def _inputs(B, M, H, C):
    g = torch.Generator().manual_seed(B + M + H + C)
    x = torch.rand(B, M, generator=g)
    h = torch.relu(torch.randn(B, H, generator=g))
    w2 = torch.randn(H, C, generator=g) * 0.1
    b2 = torch.randn(C, generator=g) * 0.1
    y = torch.randint(0, C, (B,), generator=g)
    return x, h, w2, b2, y


def _torch_grads(x, h, w2, b2, y):
    """Plain fp32 autograd composition of the same head + dW1."""
    B = x.shape[0]
    hh = h.clone().requires_grad_(True)
    w2g = w2.clone().requires_grad_(True)
    b2g = b2.clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(hh @ w2g + b2g, y)
    loss.backward()
    dh = hh.grad * (h > 0)
    return loss.detach(), x.t() @ dh, dh.sum(0), w2g.grad, b2g.grad


@pytest.mark.parametrize("shape", SHAPES)
def test_grads_op_matches_torch(shape):
    x, h, w2, b2, y = _inputs(*shape)
    B, M, H, C = shape
    outs = [torch.empty(M, H), torch.empty(H), torch.empty(H, C),
            torch.empty(C)]
    loss = ops.mlp_head_tail_grads(x, h, w2, b2, y, *outs)
    want = _torch_grads(x, h, w2, b2, y)
    for got, ref in zip([loss] + outs, want):
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("shape", SHAPES)
def test_sgd_op_matches_torch(shape):
    x, h, w2, b2, y = _inputs(*shape)
    B, M, H, C = shape
    g = torch.Generator().manual_seed(5)
    w1 = torch.randn(M, H, generator=g) * 0.1
    b1 = torch.randn(H, generator=g) * 0.1
    masters = [w1.clone(), b1.clone(), w2.clone(), b2.clone()]
    # fp32 "shadows": the op refreshes them in whatever dtype they have
    w2s, b2s = w2.clone(), b2.clone()
    w1s, b1s = w1.clone(), b1.clone()
    lr = 0.05
    loss = ops.mlp_head_tail_sgd(x, h, w2s, b2s, y, *masters, w1s, b1s, lr)
    ref_loss, dw1, db1, dw2, db2 = _torch_grads(x, h, w2, b2, y)
    torch.testing.assert_close(loss, ref_loss, rtol=1e-5, atol=1e-6)
    for m, s, p0, gr in zip(masters, [w1s, b1s, w2s, b2s],
                            [w1, b1, w2, b2], [dw1, db1, dw2, db2]):
        torch.testing.assert_close(m, p0 - lr * gr, rtol=1e-5, atol=1e-6)
        assert torch.equal(s, m)


def _trainer(model):
    return SyncReplicaTrainer(model.init_params(), optimizer="sgd",
                              hparams={"lr": 0.01}, device="cpu")


def test_model_fwd_bwd_routes_through_grads_op(monkeypatch):
    model = MnistMLP()
    t = _trainer(model)
    x, y = synthetic_batch(100)
    calls = []
    real = ops.mlp_head_tail_grads
    monkeypatch.setattr(ops, "mlp_head_tail_grads",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    p = lambda n: t.store.view(n)
    loss = model.fwd_bwd(p, x, y, t.grad_view)
    assert calls == [1]
    h = torch.relu(x @ p("hid_w") + p("hid_b"))
    want = _torch_grads(x, h, p("sm_w"), p("sm_b"), y)
    got = [loss] + [t.grad_view(n)
                    for n in ("hid_w", "hid_b", "sm_w", "sm_b")]
    for a, b in zip(got, want):
        torch.testing.assert_close(a.float(), b, rtol=1e-4, atol=1e-5)


def test_model_fwd_bwd_apply_routes_through_sgd_op(monkeypatch):
    model = MnistMLP()
    t = _trainer(model)
    x, y = synthetic_batch(100)
    x = x.to(torch.bfloat16)          # the shadows it runs on are bf16
    calls = []
    real = ops.mlp_head_tail_sgd
    monkeypatch.setattr(ops, "mlp_head_tail_sgd",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    before = t.store.flat.clone()
    l0 = float(model.fwd_bwd_apply(t, x, y, lr=0.01))
    for _ in range(20):
        l1 = float(model.fwd_bwd_apply(t, x, y, lr=0.01))
    assert len(calls) == 21 and t.store.global_step == 21
    assert not torch.equal(before, t.store.flat)
    assert torch.equal(t.store.flat_bf16,
                       t.store.flat.to(torch.bfloat16))
    assert l1 < l0


def test_gate_selects_the_two_kernel_sequence(monkeypatch):
    from tfmesos_amd.models import mlp
    monkeypatch.setattr(mlp, "_HEADTAIL", False)
    x, _ = synthetic_batch(100)
    assert not MnistMLP()._headtail_ok(x)
    monkeypatch.setattr(mlp, "_HEADTAIL", True)
    assert MnistMLP()._headtail_ok(x)
    assert not MnistMLP(hidden_units=102)._headtail_ok(x)   # H % 4
