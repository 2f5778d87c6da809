"""ops.dot_softmax_loss on the CPU: the input maker, the fp64 oracle and the
check (shared with test_dot_softmax_gpu.py), the fp32 torch reference within
the bounds, validation.

Inputs, on the grid of test_sampled_softmax.py: rows are multiples of 1/16 in
[-1/4, 1/4], bias multiples of 1/4 in [-2, 2], g multiples of 1/8 in
[1/8, 1]. Every score then sits on a 1/256 grid with |score| <= 18: exact in
fp32 in any summation order. labels[0] = 0, labels[-1] = V - 1, labels[1] =
-1 (ignored) when B >= 3; item V // 2 is no label and has bias -inf when
V >= 3.

Bounds (those derived in test_sampled_softmax.py; V <= 330 keeps the sum's
length inside the loss bound's headroom):
  loss: |err| <= 2^-14 max(1, |lse|).
  dq, dw: |err| <= (2^-7 + 2^-16) A componentwise, A the fp64 sum of the
    absolute values of the component's terms.
  dbias (fp32, never bf16): 2^-14 A.
"""

import pytest
import torch

from tfmesos_amd import ops

SHAPES = [(5, 130, 200), (67, 65, 72), (130, 5, 256), (3, 64, 7)]
GRADS = ("q", "w", "bias")


def make(B, V, D, seed=0):
    """dict of q, w, bias, labels, g."""
    gen = torch.Generator().manual_seed(seed)
    row = lambda n: (torch.randint(-4, 5, (n, D), generator=gen) / 16).to(  # noqa: E731
        torch.bfloat16)
    q, w = row(B), row(V)
    bias = torch.randint(-8, 9, (V,), generator=gen) / 4
    labels = torch.randint(0, V, (B,), generator=gen)
    if V >= 3:
        labels[labels == V // 2] = 0
        bias[V // 2] = float("-inf")
    labels[0], labels[-1] = 0, V - 1
    if B >= 3:
        labels[1] = -1
    return dict(q=q, w=w, bias=bias, labels=labels,
                g=torch.randint(1, 9, (B,), generator=gen) / 8)


def oracle(q, w, bias, labels, g):
    """fp64: loss, lse, the three gradients and their absolute-term sums A."""
    d = lambda t: t.detach().double().cpu().requires_grad_(True)  # noqa: E731
    x = dict(q=d(q), w=d(w), bias=d(bias))
    labels = labels.cpu()
    live, col = labels >= 0, labels.clamp(min=0)[:, None]
    s = x["q"] @ x["w"].t() + x["bias"]
    lse = torch.logsumexp(s, 1)
    t = s.gather(1, col)[:, 0]
    loss = torch.where(live, lse - t, torch.zeros_like(lse))
    gd = g.double().cpu() * live
    loss.backward(gd)
    with torch.no_grad():
        p = gd[:, None] * torch.exp(s - lse[:, None])
        p.scatter_(1, col, (gd * (torch.exp(t - lse) - 1)).abs()[:, None])
        A = dict(q=p @ x["w"].abs(), w=p.t() @ x["q"].abs(), bias=p.sum(0))
    return loss.detach(), lse.detach(), {k: x[k].grad for k in GRADS}, A


def check(inp, splits=None, bias=True):
    """dot_softmax_loss on the inputs' device within the bounds; returns the
    loss and the gradients."""
    inp = dict(inp)
    if not bias:
        inp["bias"] = torch.zeros_like(inp["bias"])
    want, lse, want_g, A = oracle(**inp)
    # detached views: they keep the inputs' storage offsets
    x = {k: inp[k].detach().requires_grad_(True) for k in GRADS}
    loss = ops.dot_softmax_loss(x["q"], x["w"], inp["labels"],
                                x["bias"] if bias else None, splits)
    loss.backward(inp["g"])
    assert loss.dtype == torch.float32 and loss.shape == want.shape
    err = (loss.detach().cpu().double() - want).abs()
    bound = 2.0 ** -14 * lse.abs().clamp(min=1)
    print("loss ratio %.4f" % (err / bound).max())
    assert (err <= bound).all()
    grads = {k: x[k].grad for k in (GRADS if bias else GRADS[:2])}
    for k, got in grads.items():
        assert got.dtype == inp[k].dtype and got.device == inp[k].device
        tol = 2.0 ** -14 if k == "bias" else 2.0 ** -7 + 2.0 ** -16
        err = (got.cpu().double() - want_g[k]).abs()
        assert A[k].sum() > 0
        print("d%s ratio %.4f" % (k, (err / (tol * A[k]).clamp(min=1e-300))
                                  .max()))
        assert (err <= tol * A[k]).all(), k
    B, V = inp["q"].shape[0], inp["w"].shape[0]
    if B >= 3:                      # the ignored example
        assert loss[1].item() == 0 and not torch.signbit(loss[1])
        assert not grads["q"][1].any()
    if V >= 3 and bias:             # the masked item
        assert not grads["w"][V // 2].any() and grads["bias"][V // 2] == 0
    return loss.detach(), grads


@pytest.mark.parametrize("B,V,D", SHAPES)
def test_cpu_reference_within_bounds(B, V, D):
    check(make(B, V, D))
    check(make(B, V, D), bias=False)


def test_validation_and_empty_batch():
    i = make(3, 20, 8)
    q, w, bias, labels = i["q"], i["w"], i["bias"], i["labels"]
    wide = torch.zeros(3, 257, dtype=torch.bfloat16)
    f = ops.dot_softmax_loss
    bad = [lambda: f(q.float(), w, labels),
           lambda: f(q, w.float(), labels),
           lambda: f(q[0], w, labels),
           lambda: f(q, w[:, :7], labels),
           lambda: f(wide, wide, labels),                   # D > 256
           lambda: f(q, w, labels, bias.double()),
           lambda: f(q, w, labels, bias[:19]),
           lambda: f(q, w, labels.int()),
           lambda: f(q, w, labels[:2]),
           lambda: f(q, w, labels + 20),                    # a label >= V
           lambda: f(q, w, labels - 1),                     # a label < -1
           lambda: f(q, w, labels, splits=0),
           lambda: f(q, w, labels, splits=1.5)]
    for call in bad:
        with pytest.raises(ValueError, match="dot_softmax_loss"):
            call()
    empty = f(q[:0], w, labels[:0], bias)
    assert empty.shape == (0,) and empty.dtype == torch.float32
