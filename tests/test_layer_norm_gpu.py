"""ops.layer_norm on the GPU (csrc/norm.hip) against the fp64 oracle and the
bounds of test_layer_norm.py.

n = 67 leaves a ragged last row group at every width. D = 1, 7, 65, 1001
take the guarded form; 64 | 72, 128 | 136, 256 | 264, 512 | 520 are the two
sides of every lane-group boundary (8 | 16 | 32 | 64 lanes a row | two chunks
a lane); 1000 and 1024 the widest. The row cases pin the plan first: one row,
fewer rows than a wave holds, one block walking many groups, three blocks
with a ragged last lap and the finishing kernel, the default rule.
"""

import pytest
import torch

from tfmesos_amd import ops
from test_layer_norm import BF16, check, make, oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTHS = [1, 7, 65, 1001, 64, 72, 128, 136, 256, 264, 512, 520, 1000, 1024]
VARIANTS = [dict(rms=True), dict(residual=False), dict(bias=False),
            dict(weight=False), dict(rms=True, weight=False, bias=False)]
# (n, D, blocks, the plan the launcher must use)
ROWS = [(1, 64, None, (8, 32, 1)), (1, 1024, None, (64, 4, 1)),
        (5, 64, None, (8, 32, 1)), (5, 1024, None, (64, 4, 2)),
        (300, 64, 1, (8, 32, 1)), (300, 1024, 1, (64, 4, 1)),
        (300, 64, 3, (8, 32, 3)), (300, 1024, 3, (64, 4, 3)),
        (300, 64, None, (8, 32, 10)), (300, 1024, None, (64, 4, 75))]


def on_gpu(inp):
    return {k: v.to(DEV) for k, v in inp.items()}


@pytest.mark.parametrize("D", WIDTHS)
def test_widths(D):
    check(on_gpu(make(67, D)))


@pytest.mark.parametrize("D", [7, 64, 520])
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "-".join(v))
def test_variants(D, variant):
    check(on_gpu(make(67, D)), **variant)


@pytest.mark.parametrize("D", [7, 64, 520])
def test_bf16_parameters(D):
    check({k: v.to(BF16) for k, v in on_gpu(make(67, D)).items()})


@pytest.mark.parametrize("n,D,blocks,plan", ROWS)
def test_rows(n, D, blocks, plan):
    assert ops.layer_norm_plan(n, D, blocks) == plan
    check(on_gpu(make(n, D)), blocks=blocks)


def test_misaligned_operands():
    inp = on_gpu(make(67, 64))
    want = check(inp)
    for k in ("x", "residual", "dy"):      # one element into their storage
        buf = torch.zeros(inp[k].numel() + 1, dtype=BF16, device=DEV)
        inp[k] = buf[1:].view_as(inp[k]).copy_(inp[k])
        assert inp[k].data_ptr() % 16 == 2 and inp[k].is_contiguous()
    got = check(inp)
    for k in ("y", "s", "mean", "rstd", "dx"):  # same map, same order of sums
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("D", [65, 1000])
def test_guard_bands(D):
    inp = on_gpu(make(67, D))
    want = check(inp)
    band, size = 64, 67 * D
    buf = torch.full((3 * size + 4 * band,), 7.0, dtype=BF16, device=DEV)
    y, s, dx = (buf[band + i * (size + band):][:size].view(67, D)
                for i in range(3))
    _, _, mean, rstd = ops.layer_norm_fwd(
        inp["x"], inp["weight"], inp["bias"], 1e-5, inp["residual"], False,
        out=(y, s))
    ops.layer_norm_bwd(inp["dy"], s, mean, rstd, inp["weight"], False,
                       inp["ds"], out=dx)
    for k, v in (("y", y), ("s", s), ("dx", dx)):
        assert torch.equal(v, want[k]), k
    for i in range(4):
        assert (buf[i * (size + band):][:band] == 7).all(), i


def test_offset_rows_need_the_two_pass_variance():
    """s = 256 + 2k, k an integer in [-2, 2]: every value is exact in bf16,
    the sums and the deviations are exact in fp32; E[s^2] - mean^2 is not."""
    gen = torch.Generator().manual_seed(0)
    x = (256 + 2 * torch.randint(-2, 3, (67, 64), generator=gen)).to(BF16)
    _, ref, _ = oracle(x, None, x, None, None, None)
    _, _, mean, rstd = ops.layer_norm_fwd(x.to(DEV), None, None, 1e-5, None,
                                          False)
    assert torch.equal(mean.cpu().double(), ref["mean"])
    rel = (rstd.cpu().double() / ref["rstd"] - 1).abs().max()
    print("rstd rel err / 2^-16 = %.4f" % (rel * 2 ** 16))
    assert rel <= 2.0 ** -16


@pytest.mark.parametrize("rms", [False, True])
def test_fused_equals_two_step(rms):
    i = on_gpu(make(67, 520))
    y, s = ops.layer_norm(i["x"], i["weight"], i["bias"],
                          residual=i["residual"], rms=rms)
    assert torch.equal(s, (i["x"].float() + i["residual"].float()).to(BF16))
    assert torch.equal(y, ops.layer_norm(s, i["weight"], i["bias"], rms=rms))


def test_bit_reproducible():
    inp = on_gpu(make(300, 520))
    assert ops.layer_norm_plan(300, 520, 3) == (64, 4, 3)
    a, b = check(inp, blocks=3), check(inp, blocks=3)
    for k in a:
        assert torch.equal(a[k], b[k]) and a[k].any(), k
