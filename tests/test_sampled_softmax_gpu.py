"""ops.sampled_softmax_loss on the GPU (csrc/sampled_softmax.hip) against the
fp64 oracle and the derived bounds of test_sampled_softmax.py.

D = 7 takes the guarded path, 8 is under one K step, 72 has steps and a
tail, 200 and 256 (the limit) use the widest register tile; 64 | 65 and
128 | 129 are the two sides of the register-tile dispatch. (B, S) =
(5, 130): one owned tile, three forward splits, a candidate tail; (67, 65):
an owned-tile tail in both roles, a tile plus one; (130, 5): fewer
candidates than a tile, three example tiles for the candidate-owning role;
(1, 64): one full tile.
"""

import pytest
import torch

from tfmesos_amd import ops
from test_sampled_softmax import check, make, oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def gpu(inp):
    return {k: v.to(DEV) for k, v in inp.items()}


BOUNDARY_D = [64, 65, 128, 129]     # both sides of each DP boundary


@pytest.mark.parametrize(
    "B,S,D",
    [(B, S, D) for D in [7, 8, 72, 200, 256]
     for B, S in [(5, 130), (67, 65), (130, 5), (1, 64)]]
    + [(67, 65, D) for D in BOUNDARY_D])
def test_fwd_bwd_within_bounds(B, S, D):
    check(gpu(make(B, S, D)))


@pytest.mark.parametrize("B,S,D", [(5, 130, 200), (67, 65, 72), (130, 5, 7)])
def test_without_ids_and_adjustments(B, S, D):
    check(gpu(make(B, S, D)), ids=False, adj=False)


def test_misaligned_bases_take_guarded_path():
    inp = gpu(make(67, 65, 8))
    for k in ("h", "w_true", "w_samp"):
        buf = torch.zeros(inp[k].numel() + 1, dtype=torch.bfloat16, device=DEV)
        inp[k] = buf[1:].view_as(inp[k]).copy_(inp[k])
        assert inp[k].data_ptr() % 16 == 2 and inp[k].is_contiguous()
    x = {k: v for k, v in inp.items() if k != "g"}
    loss = ops.sampled_softmax_loss(
        inp["h"].requires_grad_(True), inp["w_true"].requires_grad_(True),
        inp["w_samp"].requires_grad_(True), inp["true_adj"], inp["samp_adj"],
        inp["labels"], inp["sampled"])
    loss.backward(inp["g"])
    want, lse, want_g, A = oracle(**x, g=inp["g"])
    assert ((loss.detach().cpu().double() - want).abs()
            <= 2.0 ** -14 * lse.abs().clamp(min=1)).all()
    for k in ("h", "w_true", "w_samp"):
        err = (inp[k].grad.cpu().double() - want_g[k]).abs()
        assert (err <= (2.0 ** -7 + 2.0 ** -16) * A[k]).all(), k


def test_in_batch_negatives():
    inp = gpu(make(67, 67, 72))
    w = inp["w_true"].clone().requires_grad_(True)
    loss = ops.sampled_softmax_loss(inp["h"], w, w, inp["true_adj"],
                                    inp["true_adj"], inp["labels"],
                                    inp["labels"])
    loss.backward(inp["g"])
    inp.update(w_samp=inp["w_true"], samp_adj=inp["true_adj"],
               sampled=inp["labels"])
    want, lse, want_g, A = oracle(**inp)
    assert ((loss.detach().cpu().double() - want).abs()
            <= 2.0 ** -14 * lse.abs().clamp(min=1)).all()
    # each of the two gradients of w is rounded once, then their bf16 sum
    tol = 2.0 ** -7 + 2.0 ** -8 + 2.0 ** -16
    err = (w.grad.cpu().double() - want_g["w_true"] - want_g["w_samp"]).abs()
    assert (err <= tol * (A["w_true"] + A["w_samp"])).all()


def test_degenerate_shapes_take_torch_path():
    inp = gpu(make(3, 4, 8))
    h, wt, ws = inp["h"], inp["w_true"], inp["w_samp"]
    out = ops.sampled_softmax_loss(h[:0], wt[:0], ws)
    assert out.shape == (0,) and out.is_cuda
    out = ops.sampled_softmax_loss(h, wt, ws[:0])
    assert torch.equal(out, torch.zeros(3, device=DEV))


def test_bit_reproducible():
    gen = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    h, wt, ws = (r(n, 128).to(torch.bfloat16).to(DEV) for n in (67, 67, 130))
    ta, sa, g = r(67).to(DEV), r(130).to(DEV), r(67).to(DEV)
    runs = []
    for _ in range(2):
        x = [t.clone().requires_grad_(True) for t in (h, wt, ws, ta, sa)]
        loss = ops.sampled_softmax_loss(*x)
        loss.backward(g)
        runs.append([loss.detach()] + [t.grad for t in x])
    for a, b in zip(*runs):
        assert torch.equal(a, b) and a.float().abs().sum() > 0
