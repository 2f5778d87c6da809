"""ops.dot_interaction on the CPU: the fp32 torch reference, forward and
backward, against an fp64 oracle — exactly.

Inputs are dyadic (multiples of 1/4 in [-2, 2], exact in bf16): every
product lies on a 1/16 grid and every partial sum stays far below 2**24
grid steps for F <= 64, D <= 256, so fp32 accumulation is exact in any
order and the oracle's values are representable in fp32. All assertions
are torch.equal.
"""

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import EmbeddingTable


def make(B, F, D, diagonal, keep_first, seed=0, dout_dtype=torch.bfloat16):
    """Dyadic x [B,F,D] bf16 and dout [B, (D) + P]."""
    gen = torch.Generator().manual_seed(seed)
    P = F * (F + 1) // 2 if diagonal else F * (F - 1) // 2
    x = (torch.randint(-8, 9, (B, F, D), generator=gen) / 4).to(torch.bfloat16)
    dout = (torch.randint(-8, 9, (B, (D if keep_first else 0) + P),
                          generator=gen) / 4).to(dout_dtype)
    return x, dout


def oracle(x, dout, diagonal, keep_first):
    """fp64 (out, dx): bmm, tril_indices gather, cat, autograd."""
    xd = x.double().cpu().requires_grad_(True)
    F = xd.shape[1]
    i, j = torch.tril_indices(F, F, 0 if diagonal else -1)
    out = torch.bmm(xd, xd.transpose(1, 2))[:, i, j]
    if keep_first:
        out = torch.cat([xd[:, 0], out], 1)
    out.backward(dout.double().cpu())
    return out.detach(), xd.grad


def check(x, dout, diagonal, keep_first, out_dtype=None):
    """dot_interaction on x's device equals the oracle, forward and back."""
    want, want_dx = oracle(x, dout, diagonal, keep_first)
    assert want.abs().sum() > 0 and want_dx.abs().sum() > 0
    xr = x.detach().requires_grad_(True)
    out = ops.dot_interaction(xr, diagonal, keep_first, out_dtype)
    out.backward(dout)
    assert out.dtype == (out_dtype or torch.bfloat16)
    assert xr.grad.dtype == torch.bfloat16
    assert torch.equal(out.detach().cpu(), want.to(out.dtype))
    assert torch.equal(xr.grad.cpu(), want_dx.to(torch.bfloat16))


@pytest.mark.parametrize("F,D,diagonal,keep_first", [
    (2, 7, False, True), (16, 8, True, True), (27, 72, False, False),
    (33, 24, True, False), (64, 200, False, True)])
def test_cpu_reference_equals_oracle(F, D, diagonal, keep_first):
    check(*make(5, F, D, diagonal, keep_first), diagonal, keep_first)
    check(*make(3, F, D, diagonal, keep_first, 1, torch.float32), diagonal,
          keep_first, torch.float32)


def test_validation_and_degenerate_shapes():
    x, _ = make(3, 4, 8, False, True)
    for bad in (x.float(), x[0], torch.zeros(2, 65, 8, dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            ops.dot_interaction(bad)
    with pytest.raises(ValueError):
        ops.dot_interaction(x, out_dtype=torch.float16)
    assert ops.dot_interaction(x[:0]).shape == (0, 8 + 6)
    assert ops.dot_interaction(x[:0], True, False).shape == (0, 10)
    one = x[:, :1].clone().requires_grad_(True)
    assert ops.dot_interaction(one, keep_first=False).shape == (3, 0)
    out = ops.dot_interaction(one, out_dtype=torch.float32)
    assert torch.equal(out, x[:, 0].float())
    out.backward(torch.ones_like(out))
    assert torch.equal(one.grad, torch.ones_like(one))


def test_pooled_pull_interaction_pooled_push():
    tables = [EmbeddingTable("t%d" % f, 12, 8, seed=f, lr=0.5)
              for f in range(2)]
    for f, t in enumerate(tables):      # dyadic rows: the bag sums are exact
        t.master.copy_(make(1, 12, 8, False, False, seed=f)[0][0])
        t.shadow.copy_(t.master)
    before = [t.master.clone() for t in tables]
    ids = torch.tensor([0, 3, 3, 7, 11, 5])
    offsets = torch.tensor([0, 2, 3, 6])
    x = torch.stack([t.pull_pooled(ids, offsets) for t in tables], 1)
    x.requires_grad_(True)
    out = ops.dot_interaction(x, out_dtype=torch.float32)
    w = torch.arange(1., out.numel() + 1).view_as(out) / 4
    (out * w).sum().backward()
    _, want_dx = oracle(x.detach(), w, False, True)
    assert want_dx.abs().sum() > 0
    assert torch.equal(x.grad, want_dx.to(torch.bfloat16))
    for f, t in enumerate(tables):
        t.push_pooled(ids, offsets, x.grad[:, f].contiguous())
        assert not torch.equal(t.master, before[f])
