"""The oracle of the exact conv tests, checked without a GPU.

test_conv_exact_gpu.py compares the HIP conv kernels with
_conv_exact.compute_reference (torch fp64 conv2d / conv2d_input /
conv2d_weight) using torch.equal. Here that reference is itself
compared with a naive nested-loop convolution written below, and the
+-1 generator and the max|ref| <= 256 exactness condition are run on
every listed shape, so a bad shape or seed shows up before any GPU run.
"""

import pytest
import torch

import _conv_exact as ce


def naive(c, x, w, b, dy):
    """y, dX, dW straight from the definition, one product at a time."""
    Ho, Wo = ce.out_hw(c)
    y = b.view(1, -1, 1, 1).expand(c.N, c.K, Ho, Wo).clone()
    dx = torch.zeros_like(x)
    dw = torch.zeros_like(w)
    for n in range(c.N):
        for k in range(c.K):
            for ho in range(Ho):
                for wo in range(Wo):
                    g = dy[n, k, ho, wo]
                    for r in range(c.R):
                        hi = ho * c.stride[0] + r - c.pad[0]
                        if hi < 0 or hi >= c.H:
                            continue
                        for s in range(c.S):
                            wi = wo * c.stride[1] + s - c.pad[1]
                            if wi < 0 or wi >= c.W:
                                continue
                            for ch in range(c.C):
                                xv = x[n, ch, hi, wi]
                                wv = w[k, ch, r, s]
                                y[n, k, ho, wo] += xv * wv
                                dx[n, ch, hi, wi] += g * wv
                                dw[k, ch, r, s] += g * xv
    return y, dx, dw


TINY = [
    # padded, stride 2, H != W, output rows that skip input rows
    ce._c("tiny_s2_pad", 2, 3, 6, 5, 4, 3, 3, 2, 1, 1, 1, 1),
    # 1x7 with asymmetric padding
    ce._c("tiny_1x7", 1, 2, 3, 9, 3, 1, 7, 1, (0, 3), 1, 1, 1),
]


@pytest.mark.parametrize("c", TINY, ids=lambda c: c.id)
def test_reference_matches_naive_loops(c):
    x, w, b, dy = ce.inputs(c)
    ref = ce.compute_reference(c, x, w, b, dy)
    y, dx, dw = naive(c, x, w, b, dy)
    assert torch.equal(ref.y, y)
    assert torch.equal(ref.dx, dx)
    assert torch.equal(ref.dw, dw)


@pytest.mark.parametrize("c", ce.CASES, ids=lambda c: c.id)
def test_case_is_exactly_representable(c):
    x, w, b, dy = ce.inputs(c)
    for t in (x, w, dy):
        assert torch.equal(t.abs(), torch.ones_like(t))      # +-1, no zeros
    assert -1 in x and 1 in x
    assert torch.equal(b, b.round()) and b.abs().max() <= 3
    ref = ce.reference(c)
    ce.assert_representable(ref)
    for t in (ref.y, ref.dx, ref.dw):
        # integers within +-256 survive the bf16 round trip unchanged
        assert torch.equal(t, t.round())
        assert torch.equal(t.to(torch.bfloat16).double(), t)
    assert c.N * c.C * c.H * c.W <= 300000 and ref.y.numel() <= 300000
    # the unwritten-output probe needs a non-zero last element
    if "y" in c.probe:
        assert ref.y.numel() % 1024 in (1, 2, 3)
        assert ref.y.flatten()[-1] != 0
    if "dx" in c.probe:
        assert ref.dx.numel() % 1024 in (1, 2, 3)
        assert ref.dx.flatten()[-1] != 0


@pytest.mark.parametrize("n", ce.NARROW, ids=lambda n: "off%d_pad%d" % n)
def test_narrow_case_is_exactly_representable(n):
    c = ce.BY_ID[ce.NARROW_CASE]
    off, pad = n
    ref = ce.reference(c, n)
    ce.assert_representable(ref)
    big = ce.narrow_buffer(c, off, pad)
    assert torch.equal(big.abs(), torch.ones_like(big))
    assert torch.equal(ref.dy, big[:, off:off + c.K])
    # same x and w as the plain case, another dy
    assert torch.equal(ref.x, ce.reference(c).x)
    assert not torch.equal(ref.dy, ce.reference(c).dy)


def test_case_ids_unique_and_launched_slices():
    assert len(ce.BY_ID) == len(ce.CASES)
    assert len(ce.proc_lines()) == 2 * len(ce.CASES) + len(ce.NARROW)
    # KD = 600 at z = 9: 96-tap slices, 7 launched, last one 24 taps
    assert ce.launched_slices(600, 9) == (7, 24)
    assert ce.launched_slices(576, 9) == (9, 64)
    assert ce.launched_slices(540, 8) == (6, 60)
