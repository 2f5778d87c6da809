"""ops.bag_attention on the GPU (csrc/bag_attention.hip) against the fp64
oracle and the derived bounds of test_bag_attention.py.

Query bags (0, 1, 63, 64, 65, 130): an empty bag, one row, the tile edges and
three tiles with a tail (so the causal form skips tiles and masks diagonal
ones). The cross form's key bags (5, 0, 64, 130, 1, 65) put keys against no
query and a query against no keys. D = 7 takes the guarded path, 8 is under
one K step, 64 is exactly DP, 65 the first width of DP = 128 (guarded), 72
has a K tail inside DP = 128, 128 is the limit.
"""

import pytest
import torch

from tfmesos_amd import ops
from test_bag_attention import KL, QL, check, k_is_v, make, oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def gpu(inp):
    return {k: v if v is None else v.to(DEV) for k, v in inp.items()}


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("D", [7, 8, 64, 65, 72, 128])
def test_self_within_bounds(D, H, causal):
    check(gpu(make(QL, None, H, D)), causal)


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("D", [7, 72, 128])
def test_cross_within_bounds(D, H):
    check(gpu(make(QL, KL, H, D)))


def test_default_scale():
    check(gpu(make((3, 70), (66, 2), 2, 64)), scale=0.125)


def test_misaligned_bases_take_guarded_path():
    inp = gpu(make(QL, KL, 3, 8))
    for n in ("q", "k", "v", "dout"):
        buf = torch.zeros(inp[n].numel() + 1, dtype=torch.bfloat16, device=DEV)
        inp[n] = buf[1:].view_as(inp[n]).copy_(inp[n])
        assert inp[n].data_ptr() % 16 == 2 and inp[n].is_contiguous()
    want, want_g, bnd, _ = oracle(inp)
    x = {n: inp[n].requires_grad_(True) for n in "qkv"}
    out = ops.bag_attention(x["q"], x["k"], x["v"], inp["offsets"],
                            inp["kv_offsets"], scale=0.25)
    out.backward(inp["dout"])
    assert ((out.detach().cpu().double() - want).abs() <= bnd["out_q"]).all()
    for n in "qkv":
        err = (x[n].grad.cpu().double() - want_g[n]).abs()
        assert (err <= bnd[n]).all(), n


def test_k_is_v():
    k_is_v(gpu(make(QL, KL, 3, 8)))


def test_no_rows_takes_torch_path():
    inp = gpu(make(QL, KL, 2, 8))
    none = torch.zeros(len(QL) + 1, dtype=torch.int64, device=DEV)
    out = ops.bag_attention(inp["q"][:0], inp["k"], inp["v"], none,
                            inp["kv_offsets"])
    assert out.shape == (0, 2, 8) and out.is_cuda
    out = ops.bag_attention(inp["q"], inp["k"][:0], inp["v"][:0],
                            inp["offsets"], none)
    assert torch.equal(out, torch.zeros_like(inp["q"]))


def test_bit_reproducible():
    gen = torch.Generator().manual_seed(3)
    r = lambda n: torch.randn(n, 2, 72, generator=gen).to(torch.bfloat16).to(  # noqa: E731
        DEV)
    off = make(QL, None, 1, 1)["offsets"].to(DEV)
    q, k, v, g = r(sum(QL)), r(sum(QL)), r(sum(QL)), r(sum(QL))
    runs = []
    for _ in range(2):
        x = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out = ops.bag_attention(*x, off, causal=True)
        out.backward(g)
        runs.append([out.detach()] + [t.grad for t in x])
    for a, b in zip(*runs):
        assert torch.equal(a, b) and a.float().abs().sum() > 0
