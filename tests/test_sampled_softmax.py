"""ops.sampled_softmax_loss on the CPU: the fp32 torch reference, forward and
backward, against an fp64 oracle (masked_fill(-inf), logsumexp, autograd).

Inputs: rows are multiples of 1/16 in [-1/4, 1/4], adjustments multiples of
1/4 in [-2, 2], g multiples of 1/8 in [1/8, 1], ids drawn from range(50) so
that accidental hits occur. Every score then sits on a 1/256 grid with
|score| < 19: exact in fp32 in any summation order.

Bounds (derived; bf16 has 8 significant bits, unit roundoff 2^-8):
  loss: |err| <= 2^-14 max(1, |lse|) — a sum of <= 256 positive fp32 terms is
    off by <= 2^-16 relative, exp / log add a few ulp, the final subtraction
    2^-24 |lse|; the rest is headroom.
  dh, dw_samp, dw_true: |err| <= (2^-7 + 2^-16) A componentwise, A the fp64
    sum of the absolute values of the component's terms — one bf16 rounding
    of p (2^-8 A), one of the result (2^-8 A), 2^-16 for the fp32 exp / lse.
  dtrue_adj, dsamp_adj (fp32, never bf16): 2^-14 A.
"""

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import EmbeddingTable

SHAPES = [(5, 130, 200), (67, 65, 72), (130, 5, 256), (5, 64, 7)]


def make(B, S, D, seed=0):
    """dict of h, w_true, w_samp, true_adj, samp_adj, labels, sampled, g."""
    gen = torch.Generator().manual_seed(seed)
    row = lambda n: (torch.randint(-4, 5, (n, D), generator=gen) / 16).to(  # noqa: E731
        torch.bfloat16)
    adj = lambda n: torch.randint(-8, 9, (n,), generator=gen) / 4  # noqa: E731
    ids = lambda n: torch.randint(0, 50, (n,), generator=gen)  # noqa: E731
    return dict(h=row(B), w_true=row(B), w_samp=row(S), true_adj=adj(B),
                samp_adj=adj(S), labels=ids(B), sampled=ids(S),
                g=torch.randint(1, 9, (B,), generator=gen) / 8)


GRADS = ("h", "w_true", "w_samp", "true_adj", "samp_adj")


def oracle(h, w_true, w_samp, true_adj, samp_adj, labels, sampled, g):
    """fp64: loss, lse, the five gradients and their absolute-term sums A."""
    d = lambda t: t.detach().double().cpu().requires_grad_(True)  # noqa: E731
    x = dict(h=d(h), w_true=d(w_true), w_samp=d(w_samp),
             true_adj=d(true_adj), samp_adj=d(samp_adj))
    t = (x["h"] * x["w_true"]).sum(1) + x["true_adj"]
    l = x["h"] @ x["w_samp"].t() + x["samp_adj"]
    if labels is not None:
        l = l.masked_fill(labels.cpu()[:, None] == sampled.cpu()[None, :],
                          float("-inf"))
    lse = torch.logsumexp(torch.cat([t[:, None], l], 1), 1)
    loss = lse - t
    loss.backward(g.double().cpu())
    with torch.no_grad():
        gd = g.double().cpu()
        p = gd[:, None] * torch.exp(l - lse[:, None])
        q = (gd * (torch.exp(t - lse) - 1)).abs()[:, None]
        ah, awt, aws = x["h"].abs(), x["w_true"].abs(), x["w_samp"].abs()
        A = dict(h=p @ aws + q * awt, w_true=q * ah, w_samp=p.t() @ ah,
                 true_adj=q[:, 0], samp_adj=p.sum(0))
    return (loss.detach(), lse.detach(), {k: x[k].grad for k in GRADS}, A)


def check(inp, ids=True, adj=True):
    """sampled_softmax_loss on the inputs' device within the bounds."""
    inp = dict(inp)
    if not ids:
        inp["labels"] = inp["sampled"] = None
    if not adj:
        inp["true_adj"] = torch.zeros_like(inp["true_adj"])
        inp["samp_adj"] = torch.zeros_like(inp["samp_adj"])
    want, lse, want_g, A = oracle(**inp)
    x = {k: inp[k].detach().clone().requires_grad_(True) for k in GRADS}
    loss = ops.sampled_softmax_loss(
        x["h"], x["w_true"], x["w_samp"], x["true_adj"] if adj else None,
        x["samp_adj"] if adj else None, inp["labels"], inp["sampled"])
    loss.backward(inp["g"])
    assert loss.dtype == torch.float32 and loss.shape == want.shape
    err = (loss.detach().cpu().double() - want).abs()
    print("loss ratio %.4f" % (err / (2.0 ** -14 * lse.abs().clamp(min=1)))
          .max())
    assert (err <= 2.0 ** -14 * lse.abs().clamp(min=1)).all()
    for k in GRADS if adj else GRADS[:3]:
        got = x[k].grad
        assert got.dtype == inp[k].dtype and got.device == inp[k].device
        tol = (2.0 ** -7 + 2.0 ** -16) if k in GRADS[:3] else 2.0 ** -14
        err = (got.cpu().double() - want_g[k]).abs()
        assert A[k].sum() > 0
        print("d%s ratio %.4f" % (k, (err / (tol * A[k]).clamp(min=1e-300))
                                  .max()))
        assert (err <= tol * A[k]).all(), k
    return loss.detach()


@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("B,S,D", SHAPES)
def test_cpu_reference_within_bounds(B, S, D, plain):
    check(make(B, S, D), ids=not plain, adj=not plain)


def test_hit_mask_matters():
    inp = make(67, 65, 72)
    assert (inp["labels"][:, None] == inp["sampled"][None, :]).any()
    assert not torch.equal(check(inp), check(inp, ids=False))


def test_in_batch_negatives():
    inp = make(67, 67, 72)
    w = inp["w_true"].clone().requires_grad_(True)
    h = inp["h"].clone().requires_grad_(True)
    loss = ops.sampled_softmax_loss(h, w, w, inp["true_adj"], inp["true_adj"],
                                    inp["labels"], inp["labels"])
    loss.backward(inp["g"])
    inp.update(w_samp=inp["w_true"], samp_adj=inp["true_adj"],
               sampled=inp["labels"])
    want, lse, want_g, A = oracle(**inp)
    assert ((loss.detach().double() - want).abs()
            <= 2.0 ** -14 * lse.abs().clamp(min=1)).all()
    # each of the two gradients of w is rounded once, then their bf16 sum
    tol = 2.0 ** -7 + 2.0 ** -8 + 2.0 ** -16
    err = (w.grad.double() - want_g["w_true"] - want_g["w_samp"]).abs()
    assert (err <= tol * (A["w_true"] + A["w_samp"])).all()


def test_validation_and_degenerate_shapes():
    i = make(3, 4, 8)
    h, wt, ws = i["h"], i["w_true"], i["w_samp"]
    f = ops.sampled_softmax_loss
    for bad in ((h.float(), wt, ws), (h[0], wt, ws), (h, wt[:2], ws),
                (h, wt, ws[:, :7]),
                (torch.zeros(3, 257, dtype=torch.bfloat16),) * 3):
        with pytest.raises(ValueError):
            f(*bad)
    for kw in (dict(labels=i["labels"]), dict(sampled=i["sampled"]),
               dict(true_adj=i["true_adj"].double()),
               dict(samp_adj=i["true_adj"]),
               dict(labels=i["labels"].int(), sampled=i["sampled"])):
        with pytest.raises(ValueError):
            f(h, wt, ws, **kw)
    assert f(h[:0], wt[:0], ws).shape == (0,)
    hr = h.clone().requires_grad_(True)
    loss = f(hr, wt, ws[:0], i["true_adj"], i["samp_adj"][:0])
    assert torch.equal(loss, torch.zeros(3))    # one class: log(1)
    loss.sum().backward()
    assert torch.equal(hr.grad, torch.zeros_like(h))


def test_pull_loss_push_round_trip():
    table = EmbeddingTable("out", 50, 8, lr=0.5)
    table.master.copy_(make(50, 1, 8, seed=3)["h"])
    table.shadow.copy_(table.master)
    before = table.master.clone()
    inp = make(6, 9, 8, seed=4)
    ids = torch.cat([inp["labels"], inp["sampled"]])
    assert ids.unique().numel() < ids.numel()       # duplicates are pushed
    rows = table.pull(ids).requires_grad_(True)
    h = inp["h"].clone().requires_grad_(True)
    loss = ops.sampled_softmax_loss(h, rows[:6], rows[6:], inp["true_adj"],
                                    inp["samp_adj"], inp["labels"],
                                    inp["sampled"])
    loss.sum().backward()
    inp.update(w_true=before[inp["labels"]], w_samp=before[inp["sampled"]],
               g=torch.ones(6))          # the oracle indexes the dense table
    want, lse, want_g, A = oracle(**inp)
    assert ((loss.detach().double() - want).abs()
            <= 2.0 ** -14 * lse.abs().clamp(min=1)).all()
    got = rows.grad.double()
    err = (got - torch.cat([want_g["w_true"], want_g["w_samp"]])).abs()
    assert (err <= (2.0 ** -7 + 2.0 ** -16)
            * torch.cat([A["w_true"], A["w_samp"]])).all()
    table.push(ids, rows.grad)
    assert not torch.equal(table.master, before)
