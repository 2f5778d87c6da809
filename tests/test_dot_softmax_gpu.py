"""ops.dot_softmax_loss on the GPU (csrc/dot_softmax.hip) against the fp64
oracle and the bounds of test_dot_softmax.py.

Each shape is the smallest that reaches the path it names. D = 7 takes the
guarded path, 8 is under one K step, 72 has steps and a tail, 200 and 256 the
widest register tile; 64 | 65 and 128 | 129 are the two sides of the
register-tile dispatch. (B, V) = (5, 130): one owned tile of queries, three
item tiles with a tail, a label in the last ragged tile; (67, 65): owned-tile
tails in both roles, a tile plus one; (130, 5): fewer items than a tile, three
example tiles for role W; (1, 64). The split cases stream six tiles: through
one block (both buffer parities, the direct bf16 store, no reduce), two tiles
a split (fp32 partials and the reduce), and under the default rule.
"""

import pytest
import torch

from tfmesos_amd import ops
from test_dot_softmax import SHAPES, check, make, oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

GRID = [(B, V, D) for D in (7, 8, 72, 200, 256)
        for B, V in ((5, 130), (67, 65), (130, 5), (1, 64))]
GRID += [(67, 65, D) for D in (64, 65, 128, 129)]
# (B, V, splits, the plan the launcher must use)
SPLITS = [(67, 330, 1, (1, 1, 1)), (67, 330, 3, (3, 3, 2)),
          (67, 330, None, (6, 6, 2)), (330, 67, 1, (1, 1, 1)),
          (330, 67, 3, (2, 2, 3)), (330, 67, None, (2, 2, 6))]


def on_gpu(inp):
    return {n: t.to(DEV) for n, t in inp.items()}


@pytest.mark.parametrize("B,V,D", GRID)
def test_grid(B, V, D):
    check(on_gpu(make(B, V, D)))


@pytest.mark.parametrize("B,V,splits,plan", SPLITS)
def test_splits(B, V, splits, plan):
    assert ops.dot_softmax_nsplit(B, V, splits) == plan
    check(on_gpu(make(B, V, 72)), splits)


def test_misaligned_operands():
    x = on_gpu(make(67, 65, 8))
    for n in ("q", "w"):            # one element into their storage
        buf = torch.zeros(x[n].numel() + 1, dtype=torch.bfloat16, device=DEV)
        x[n] = buf[1:].view_as(x[n]).copy_(x[n])
        assert x[n].data_ptr() % 16 == 2 and x[n].is_contiguous()
    check(x)


def test_no_bias():
    check(on_gpu(make(5, 130, 200)), bias=False)


def test_bit_reproducible():
    x = on_gpu(make(67, 130, 128))
    assert ops.dot_softmax_nsplit(67, 130, 2) == (2, 2, 2)
    (la, ga), (lb, gb) = check(x, 2), check(x, 2)
    assert torch.equal(la, lb) and la.any()
    for k in ga:
        assert torch.equal(ga[k], gb[k]) and ga[k].any()


@pytest.mark.parametrize("B,V,D", sorted(set(
    GRID + SHAPES + [(B, V, 72) for B, V, _, _ in SPLITS]
    + [(67, 130, 128)])))
def test_make_keeps_label_probabilities_away_from_one(B, V, D):
    """A property of the inputs, on the CPU oracle: the componentwise
    gradient bound means something only while no label's probability is
    near 1."""
    inp = make(B, V, D)
    loss = oracle(**inp)[0]
    assert (loss >= 0).all() and (loss[inp["labels"] >= 0] > 2.0 ** -6).all()
