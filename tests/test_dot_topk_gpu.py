"""ops.dot_topk and ops.dot_rank on the GPU (csrc/retrieval.hip) against the
fp64 oracle of test_dot_topk.py.

Exact cases (torch.equal): D = 7 takes the guarded path, 8 is under one K
step, 72 has steps and a tail, 256 is the widest tile; 64 | 65 and 128 | 129
(at (5, 130, 1) only) are the two sides of the register-tile dispatch.
(B, V, k) = (5, 130,
1 / 10): three splits of one tile, an item tail; (67, 65, 64): two owned
tiles with a tail, a tile plus one item, k at its limit; (1, 64, 64): one
full tile, k == V; (130, 5, 5): V below a tile, k == V, three owned tiles;
(3, 387, 64) with splits=1: seven tiles through one block, compaction
mid-stream. The ordered streams replace the whole list every tile
(ascending) or pass nothing after the first compaction (descending).
"""

import pytest
import torch

from tfmesos_amd import ops
from test_dot_topk import make, oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (kind, B, V, D, k, splits, the nsplit the default rule must give)
EXACT = [("pairs", B, V, D, k, splits, n)
         for D in (7, 8, 72, 256)
         for B, V, k, splits, n in ((5, 130, 1, None, 3), (5, 130, 10, None, 3),
                                    (67, 65, 64, None, 2), (1, 64, 64, None, 1),
                                    (130, 5, 5, None, 1),
                                    (3, 387, 64, 1, None))]
EXACT += [("pairs", 5, 130, D, 1, None, 3)      # the register-tile dispatch
          for D in (64, 65, 128, 129)]
EXACT += [(kind, 3, 387, 8, k, 1, None)
          for kind in ("ascending", "descending") for k in (64, 1)]
EXACT += [("masked", 1, 64, 8, 64, None, 1),
          ("misaligned", 67, 65, 8, 10, None, 2)]


@pytest.mark.parametrize("kind,B,V,D,k,splits,nsplit", EXACT)
def test_exact(kind, B, V, D, k, splits, nsplit):
    inp = make(B, V, D, "pairs" if kind == "misaligned" else kind)
    s, order, want_rank = oracle(**inp)
    top = s.gather(1, order[:, :k + 1])
    assert (top[:, 1:] == top[:, :-1]).any(1).all()     # a tie at stake
    if splits is None:
        assert ops.dot_topk_nsplit(B, V) == nsplit
    x = {n: None if t is None else t.to(DEV) for n, t in inp.items()}
    if kind == "misaligned":        # one element into their storage
        for n in ("q", "w"):
            buf = torch.zeros(x[n].numel() + 1, dtype=torch.bfloat16,
                              device=DEV)
            x[n] = buf[1:].view_as(x[n]).copy_(x[n])
            assert x[n].data_ptr() % 16 == 2 and x[n].is_contiguous()
    values, indices = ops.dot_topk(x["q"], x["w"], k, x["bias"], splits)
    rank = ops.dot_rank(x["q"], x["w"], x["labels"], x["bias"], splits)
    assert values.dtype == torch.float32 and indices.dtype == torch.int64
    assert torch.equal(indices.cpu(), order[:, :k])
    assert torch.equal(values.cpu().double(), s.gather(1, order[:, :k]))
    assert torch.equal(rank.cpu(), want_rank)
    if kind == "masked":            # the masked items last, in index order
        assert torch.equal(indices[0, -16:].cpu(), torch.arange(0, 64, 4))


@pytest.mark.parametrize("D", [72, 200])
def test_random_within_bound(D):
    """tol[b] = D * 2**-22 * max_j(|q[b]|.|w[j]| + |bias[j]|): products of two
    bf16 are exact in fp32, any fp32 summation of D + 1 terms errs by at most
    about (D + 1) * 2**-24 of the sum of magnitudes, and the factor 4 covers
    the MFMA's undocumented internal order. Every computed score is within
    tol of the exact one, so order statistics move by at most tol and a
    comparison of two computed scores can differ from the exact one only
    where the exact scores are within 2 tol."""
    B, V, k = 67, 1000, 10
    inp = make(B, V, D, "random")
    s, order, _ = oracle(**inp)
    # labels at the top-k boundary: the k-th and the (k+1)-th item in turn
    inp["labels"] = order.gather(1, (k - 1 + torch.arange(B) % 2)[:, None])[:, 0]
    inp["labels"][::5] = torch.arange(0, V, V // 14)[:14]
    mag = inp["q"].double().abs() @ inp["w"].double().abs().t() + inp["bias"].abs()
    tol = D * 2.0 ** -22 * mag.max(1).values[:, None]
    x = {n: t.to(DEV) for n, t in inp.items()}
    values, indices = ops.dot_topk(x["q"], x["w"], k, x["bias"])
    rank = ops.dot_rank(x["q"], x["w"], x["labels"], x["bias"]).cpu()
    values, indices = values.cpu().double(), indices.cpu()
    err_sorted = (values - s.gather(1, order[:, :k])).abs()
    err_at = (values - s.gather(1, indices)).abs()
    print("D=%d worst |value - oracle| / tol: order statistics %.3f, at the "
          "returned index %.3f" % (D, float((err_sorted / tol).max()),
                                   float((err_at / tol).max())))
    assert (values[:, 1:] <= values[:, :-1]).all()
    assert (err_sorted <= tol).all() and (err_at <= tol).all()
    assert torch.equal(rank < k, (indices == inp["labels"][:, None]).any(1))
    t = s.gather(1, inp["labels"][:, None])
    assert ((s > t + 2 * tol).sum(1) <= rank).all()
    assert (rank <= (s >= t - 2 * tol).sum(1) - 1).all()


def test_bit_reproducible():
    inp = make(67, 1000, 128, "random")
    x = {n: t.to(DEV) for n, t in inp.items()}
    assert ops.dot_topk_nsplit(67, 1000) > 1
    runs = [ops.dot_topk(x["q"], x["w"], 64, x["bias"])
            + (ops.dot_rank(x["q"], x["w"], x["labels"], x["bias"]),)
            for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_empty_batch_stays_on_device():
    x = {n: t.to(DEV) for n, t in make(3, 20, 8).items()}
    values, indices = ops.dot_topk(x["q"][:0], x["w"], 4, x["bias"])
    assert values.shape == indices.shape == (0, 4)
    assert values.is_cuda and indices.is_cuda
    assert ops.dot_rank(x["q"][:0], x["w"], x["labels"][:0]).is_cuda
