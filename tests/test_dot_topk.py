"""ops.dot_topk and ops.dot_rank on the CPU: the input maker and the fp64
oracle (shared with test_dot_topk_gpu.py), the CPU path against the oracle on
exact inputs, and the argument checks.

Exact inputs: every score is an integer of magnitude at most D + 3 <= 259,
exact in fp32 in any summation order, so values, indices and ranks are
compared with torch.equal. Items come in identical adjacent pairs (or, in the
ordered streams, triples), so every query has a tie inside its top-k or
across its boundary: the order's tie rule is what is under test.
"""

import pytest
import torch

from tfmesos_amd import ops


def make(B, V, D, kind="pairs", seed=0):
    """dict of q, w bf16, bias fp32 or None, labels int64 (0 and V - 1 among
    them).

    pairs:      q, w are +-1, bias integers in [-3, 3], w[2i+1] = w[2i] and
                the bias likewise (an odd V leaves its last item single);
    masked:     pairs, with -inf bias on every fourth item;
    ascending:  w[j] = floor(j/3) e_0, q[b,0] = 1 + b % 2, the rest of q +-1,
                no bias: scores nondecreasing in j, ties in triples;
    descending: ascending with w reversed;
    random:     randn rows and bias.
    """
    gen = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * V + D)
    pm = lambda *s: torch.randint(0, 2, s, generator=gen) * 2.0 - 1  # noqa: E731
    q = pm(B, D)
    if kind in ("pairs", "masked"):
        w = pm((V + 1) // 2, D).repeat_interleave(2, 0)[:V]
        bias = torch.randint(-3, 4, ((V + 1) // 2,), generator=gen).float()
        bias = bias.repeat_interleave(2)[:V].contiguous()
        if kind == "masked":
            bias[::4] = float("-inf")
    elif kind in ("ascending", "descending"):
        w = torch.zeros(V, D)
        w[:, 0] = torch.arange(V) // 3
        if kind == "descending":
            w = w.flip(0)
        q[:, 0] = 1 + torch.arange(B) % 2
        bias = None
    else:
        q, w = torch.randn(B, D, generator=gen), torch.randn(V, D, generator=gen)
        bias = torch.randn(V, generator=gen)
    labels = torch.randint(0, V, (B,), generator=gen)
    labels[0], labels[-1] = 0, V - 1
    return dict(q=q.to(torch.bfloat16), w=w.contiguous().to(torch.bfloat16),
                bias=bias, labels=labels)


def oracle(q, w, bias, labels):
    """fp64 from the stored bf16 operands: (s [B,V], order [B,V] best first,
    rank [B] = the number of items that beat labels[b])."""
    s = q.cpu().double() @ w.cpu().double().t()
    if bias is not None:
        s = s + bias.cpu().double()
    order = torch.sort(-s, dim=1, stable=True).indices
    labels = labels.cpu()
    t = s.gather(1, labels[:, None])
    before = torch.arange(s.shape[1])[None, :] < labels[:, None]
    return s, order, ((s > t) | ((s == t) & before)).sum(1)


@pytest.mark.parametrize("kind,B,V,D,k", [
    ("pairs", 5, 130, 7, 10), ("pairs", 67, 65, 72, 64),
    ("pairs", 130, 5, 256, 5), ("masked", 1, 64, 8, 64),
    ("ascending", 3, 387, 8, 1), ("descending", 3, 387, 8, 64)])
def test_cpu_path_matches_oracle(kind, B, V, D, k):
    inp = make(B, V, D, kind)
    s, order, want_rank = oracle(**inp)
    top = s.gather(1, order[:, :k + 1])
    assert (top[:, 1:] == top[:, :-1]).any(1).all()     # a tie at stake
    values, indices = ops.dot_topk(inp["q"], inp["w"], k, inp["bias"])
    rank = ops.dot_rank(inp["q"], inp["w"], inp["labels"], inp["bias"])
    assert values.dtype == torch.float32 and indices.dtype == torch.int64
    assert torch.equal(indices, order[:, :k])
    assert torch.equal(values.double(), s.gather(1, order[:, :k]))
    assert torch.equal(rank, want_rank)
    assert torch.equal(rank < k, (indices == inp["labels"][:, None]).any(1))


def test_empty_batch():
    inp = make(3, 20, 8)
    values, indices = ops.dot_topk(inp["q"][:0], inp["w"], 4)
    assert values.shape == indices.shape == (0, 4)
    assert ops.dot_rank(inp["q"][:0], inp["w"], inp["labels"][:0]).shape == (0,)


def test_argument_checks():
    i = make(3, 20, 8)
    q, w, bias, labels = i["q"], i["w"], i["bias"], i["labels"]
    wide = torch.zeros(3, 257, dtype=torch.bfloat16)
    bad = [lambda: ops.dot_topk(q, w, 21),                  # k > V
           lambda: ops.dot_topk(q, torch.cat([w] * 4), 65),  # k > 64
           lambda: ops.dot_topk(q, w, 0),
           lambda: ops.dot_topk(wide, wide, 1),             # D > 256
           lambda: ops.dot_topk(q.float(), w, 1),
           lambda: ops.dot_topk(q, w[:, :7], 1),
           lambda: ops.dot_topk(q, w, 1, bias.double()),
           lambda: ops.dot_topk(q, w, 1, bias[:19]),
           lambda: ops.dot_topk(q, w, 1, splits=0),
           lambda: ops.dot_rank(q, w.float(), labels),
           lambda: ops.dot_rank(q, w, labels.int()),
           lambda: ops.dot_rank(q, w, labels[:2]),
           lambda: ops.dot_rank(q, w, labels + 20),         # out of range
           lambda: ops.dot_rank(q, w, labels - 20)]
    for f in bad:
        with pytest.raises(ValueError, match="dot_topk|dot_rank"):
            f()
