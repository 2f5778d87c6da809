"""ops.layer_norm on the CPU: the input maker, the fp64 oracle and the check
(shared with test_layer_norm_gpu.py), the fp32 torch reference within the
bounds, validation, autograd wiring, fused = two-step.

Inputs: x, residual, dy, ds ~ N(0, 1) stored as bf16; weight ~ 1 + 0.5 N(0, 1)
and bias ~ N(0, 1) as fp32 (or rounded to bf16 before anything reads them).
The oracle is fp64 on the stored values and on s = bf16(fp32(x) +
fp32(residual)): s is part of the definition and is compared with
torch.equal.

Bounds, with u8 = 2^-8 (one rounding to bf16: 8 significant bits, round to
nearest) and u24 = 2^-24 (one fp32 operation). An output err is bounded by

    [u8 |ref|, if the output is bf16]  +  c u24 A

A is the sum of the absolute values of the terms of the reference expression,
so the fp32 part is a first-order bound on an evaluation whose every
operation rounds once and whose longest summation has c - K terms; K = 10
covers the operations that are not part of that summation (for y: the
division by D, the subtraction of the mean, the variance's division, the eps
add, the square root, the reciprocal, two multiplications, the bias add; for
dx: the subtraction and scale that rebuild x-hat, dy w, two divisions by D,
the product with x-hat, two subtractions, the scale by rstd, the ds add; for
the parameter gradients: x-hat as for dx and the product).

  y:      A = |w xh| + |b|;                              c = D + K
  mean:   A = sum|s| / D;  rstd: A = rstd (a sum of non-negative terms);
                                                          c = D + K, fp32
  dx:     A = rstd (|g| + |mean_D g| + |xh mean_D(g xh)|) + |ds|;
                                                          c = D + K
  dweight: A = sum_rows |dy xh|;  dbias: A = sum_rows |dy|;
                                                          c = max(n, D) + K
          (the sum over rows, or the row sums inside xh, whichever is
          longer), plus u8 |ref| where the parameter is bf16.

Nothing here is fitted to an output; the CPU reference has to meet the same
bounds below, which shows they are attainable.
"""

import pytest
import torch

from tfmesos_amd import ops

U8, U24, K = 2.0 ** -8, 2.0 ** -24, 10
BF16 = torch.bfloat16
SHAPES = [(67, 7), (5, 64), (67, 65), (3, 1), (9, 520), (4, 1024)]


def make(n, D, seed=0):
    """dict of x, residual, dy, ds (bf16 [n, D]) and weight, bias (fp32)."""
    gen = torch.Generator().manual_seed(seed)
    inp = {k: torch.randn(n, D, generator=gen).to(BF16)
           for k in ("x", "residual", "dy", "ds")}
    inp["weight"] = 1 + 0.5 * torch.randn(D, generator=gen)
    inp["bias"] = torch.randn(D, generator=gen)
    return inp


def oracle(x, residual, dy, ds, weight, bias, eps=1e-5, rms=False):
    """fp64: s (bf16, as defined), the references and their A, by output."""
    n, D = x.shape
    f64 = torch.float64
    s = x if residual is None else (x.float() + residual.float()).to(BF16)
    sd, dyd = s.double(), dy.double()
    w = torch.ones(D, dtype=f64) if weight is None else weight.double()
    b = torch.zeros(D, dtype=f64) if bias is None else bias.double()
    up = torch.zeros(n, D, dtype=f64) if ds is None else ds.double()
    mean = torch.zeros(n, dtype=f64) if rms else sd.mean(1)
    d = sd - mean[:, None]
    rstd = 1 / torch.sqrt((d * d).mean(1) + eps)
    r, xh, g = rstd[:, None], d * rstd[:, None], dyd * w
    mg = torch.zeros(n, 1, dtype=f64) if rms else g.mean(1, keepdim=True)
    mgx = (g * xh).mean(1, keepdim=True)
    ref = dict(y=w * xh + b, mean=mean, rstd=rstd,
               dx=r * (g - mg - xh * mgx) + up,
               dweight=(dyd * xh).sum(0), dbias=dyd.sum(0))
    A = dict(y=(w * xh).abs() + b.abs(), mean=sd.abs().mean(1), rstd=rstd,
             dx=r * (g.abs() + mg.abs() + (xh * mgx).abs()) + up.abs(),
             dweight=(dyd * xh).abs().sum(0), dbias=dyd.abs().sum(0))
    return s, ref, A


def check(inp, rms=False, residual=True, weight=True, bias=True, blocks=None,
          eps=1e-5):
    """ops.layer_norm forward and backward (and layer_norm_fwd's mean and
    rstd) on the inputs' device within the bounds; returns the outputs."""
    t = dict(inp)
    for k, keep in (("residual", residual), ("ds", residual),
                    ("weight", weight), ("bias", bias)):
        if not keep:
            t[k] = None
    s_ref, ref, A = oracle(eps=eps, rms=rms, **{
        k: None if v is None else v.cpu() for k, v in t.items()})
    # detached views: they keep the inputs' storage offsets
    x = {k: t[k].detach().requires_grad_(True)
         for k in ("x", "residual", "weight", "bias") if t[k] is not None}
    out = ops.layer_norm(x["x"], x.get("weight"), x.get("bias"), eps,
                         x.get("residual"), rms, blocks)
    outs = out if residual else (out,)
    torch.autograd.backward(outs, (t["dy"], t["ds"])[:len(outs)])
    y, s = outs[0].detach(), (outs[1].detach() if residual else t["x"])
    y2, s2, mean, rstd = ops.layer_norm_fwd(t["x"], t["weight"], t["bias"],
                                            eps, t["residual"], rms)
    assert torch.equal(y2, y) and torch.equal(s2, s)
    assert s.dtype == BF16 and torch.equal(s.cpu(), s_ref)
    assert not rms or not mean.any()
    got = dict(y=y, mean=mean, rstd=rstd, dx=x["x"].grad)
    if residual:
        assert torch.equal(x["residual"].grad, got["dx"])
    for k in ("weight", "bias"):
        if t[k] is not None:
            got["d" + k] = x[k].grad
    n, D = t["x"].shape
    for k, v in got.items():
        want = (torch.float32 if k in ("mean", "rstd") else
                t[k[1:]].dtype if k in ("dweight", "dbias") else BF16)
        assert v.dtype == want and v.shape == ref[k].shape, k
        assert v.device == t["x"].device
        c = (max(n, D) if k in ("dweight", "dbias") else D) + K
        bound = U8 * ref[k].abs() * (want == BF16) + c * U24 * A[k]
        err = (v.cpu().double() - ref[k]).abs()
        print("%s ratio %.4f" % (k, (err / bound.clamp(min=1e-300)).max()))
        assert (err <= bound).all(), k
    return dict(got, s=s)


@pytest.mark.parametrize("n,D", SHAPES)
def test_cpu_reference_within_bounds(n, D):
    check(make(n, D))
    check(make(n, D), rms=True)
    check(make(n, D), residual=False, bias=False)
    check(make(n, D), rms=True, weight=False, bias=False)
    check({k: v.to(BF16) for k, v in make(n, D).items()})


def test_validation_and_no_rows():
    i = make(3, 8)
    x, r, w, b = i["x"], i["residual"], i["weight"], i["bias"]
    f = ops.layer_norm
    bad = [lambda: f(x.float()),
           lambda: f(x.t()),                                # not contiguous
           lambda: f(torch.zeros(2, 1025, dtype=BF16)),     # D > 1024
           lambda: f(torch.zeros(2, 0, dtype=BF16)),
           lambda: f(x, w[:7]),
           lambda: f(x, w.double()),
           lambda: f(x, w, b[None]),
           lambda: f(x, residual=r[:2]),
           lambda: f(x, residual=r.float()),
           lambda: f(x, blocks=0),
           lambda: f(x, blocks=2 ** 31),
           lambda: f(x, blocks=1.5)]
    for call in bad:
        with pytest.raises(ValueError, match="layer_norm"):
            call()
    y, s = f(x[:0], w, b, residual=r[:0])
    assert y.shape == s.shape == (0, 8) and y.dtype == s.dtype == BF16
    _, _, mean, rstd = ops.layer_norm_fwd(x[:0], w, b, 1e-5, None, False)
    dx, dw, db = ops.layer_norm_bwd(x[:0], x[:0], mean, rstd, w, False)
    assert mean.shape == rstd.shape == (0,) and dx.shape == (0, 8)
    assert not dw.any() and not db.any() and dw.shape == db.shape == (8,)


def test_autograd_reaches_every_input():
    i = make(6, 24)
    x = {k: i[k].view(2, 3, 24).requires_grad_(True)
         for k in ("x", "residual")}
    w, b = i["weight"].requires_grad_(True), i["bias"].requires_grad_(True)
    y, s = ops.layer_norm(x["x"], w, b, residual=x["residual"])
    assert y.shape == s.shape == (2, 3, 24)
    (y.float().sum() + 2 * s.float().sum()).backward()
    for t in (x["x"], x["residual"], w, b):
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.any()
    assert torch.equal(x["x"].grad, x["residual"].grad)
    # through y alone: the residual stream's gradient is absent, not zeros
    x2 = i["x"].clone().requires_grad_(True)
    ops.layer_norm(x2, residual=i["residual"])[0].float().sum().backward()
    assert x2.grad is not None


@pytest.mark.parametrize("rms", [False, True])
def test_fused_equals_two_step(rms):
    i = make(67, 65)
    s = (i["x"].float() + i["residual"].float()).to(BF16)
    y, s1 = ops.layer_norm(i["x"], i["weight"], i["bias"],
                           residual=i["residual"], rms=rms)
    assert torch.equal(s1, s)
    assert torch.equal(y, ops.layer_norm(s, i["weight"], i["bias"], rms=rms))
