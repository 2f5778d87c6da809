"""ops.dot_interaction on the GPU (csrc/interaction.hip) against the fp64
oracle of test_dot_interaction.py — exactly (dyadic inputs, torch.equal).

F covers both edges of every MFMA tile choice (16x16x32 up to 16, one
32x32x16 up to 32, three tiles up to 64); D = 7 takes the guarded path, 8 is
under one K step, 24 no multiple of a K step, 72 several steps and a tail,
200 more than one backward column pass with a tail. B = 5 is no multiple of
the waves per block.
"""

import pytest
import torch

from tfmesos_amd import ops
from test_dot_interaction import check, make

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def gpu(x, dout):
    return x.to(DEV), dout.to(DEV)


@pytest.mark.parametrize("diagonal", [False, True])
@pytest.mark.parametrize("D", [7, 8, 24, 72, 200])
@pytest.mark.parametrize("F", [2, 15, 16, 17, 27, 32, 33, 64])
def test_fwd_bwd_exact(F, D, diagonal):
    check(*gpu(*make(5, F, D, diagonal, True)), diagonal, True)


@pytest.mark.parametrize("B,diagonal,keep_first", [
    (5, False, False), (5, True, False), (1, False, True), (67, True, True)])
def test_batch_sizes_and_no_kept_row(B, diagonal, keep_first):
    check(*gpu(*make(B, 27, 72, diagonal, keep_first)), diagonal, keep_first)


@pytest.mark.parametrize("F,D,diagonal", [(16, 7, True), (27, 72, False),
                                          (64, 200, True)])
def test_fp32_out_and_dout(F, D, diagonal):
    x, dout = make(5, F, D, diagonal, True, dout_dtype=torch.float32)
    check(*gpu(x, dout), diagonal, True, torch.float32)


def test_misaligned_x_takes_guarded_path():
    x, dout = gpu(*make(5, 27, 8, False, True))
    buf = torch.zeros(x.numel() + 1, dtype=x.dtype, device=DEV)
    view = buf[1:].view_as(x).copy_(x)
    assert view.data_ptr() % 16 == 2 and view.is_contiguous()
    check(view, dout, False, True)


def test_degenerate_shapes():
    x, _ = gpu(*make(3, 1, 8, False, True))
    assert torch.equal(ops.dot_interaction(x), x[:, 0])
    assert ops.dot_interaction(x, keep_first=False).shape == (3, 0)
    out = ops.dot_interaction(x[:0], diagonal=True)
    assert out.shape == (0, 9) and out.is_cuda


def test_bit_reproducible():
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(67, 27, 128, generator=gen).to(torch.bfloat16).to(DEV)
    dout = torch.randn(67, 128 + 351, generator=gen).to(torch.bfloat16).to(DEV)
    runs = []
    for _ in range(2):
        xr = x.clone().requires_grad_(True)
        out = ops.dot_interaction(xr)
        out.backward(dout)
        runs.append((out.detach(), xr.grad))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
    assert runs[0][0].float().abs().sum() > 0
