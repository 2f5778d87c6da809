"""Block roles of the fused head+tail kernel (csrc/gemm.hip,
mlp_head_tail_kernel): outside the ticket instantiation the dW1 tiles,
the db1 colsum / b1 apply and the classifier grads (dW2 in one block,
db2 and the loss in another) run in blocks of their own, on a grid two
rows longer than the tiles. What can break: a role that is missing or
doubled at a grid with fewer N tiles than roles, an apply that moved to
another block writing outside its view, a role reading an image it no
longer stages, the serial sum order of grads mode below 32 tiles. The
kernel's softmax also runs all 16 class slots without a predicate (pad
classes staged with a -inf bias, the label's dlogit patched in): the
sharp, flat and wild-label inputs reach its edges.

The oracle is the unchanged two-kernel route on plain tensors:
ops.mlp_head_fused followed by ops.gemm_bias_act (grads) or by
ops.mlp_tail_sgd (the SGD step). Every arithmetic operation, MFMA shape
and summation order is the same, so every comparison is EXACT
(torch.equal). Outputs start as 7.0; in SGD mode the four masters and
the four shadows are views into one allocation each, 64-element bands
of 7.0 between them, and the bands must survive.

The shapes' own forward GEMMs take no snapshot (inputs < 256), so the
snapshot comes from a carrier GEMM that does: it is a function of the
classifier alone."""

import pytest
import torch

from tfmesos_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR = 0.05
POISON = 7.0
GUARD = 64
NAMES = ("w1", "b1", "w2", "b2")

# (B, M, H, C)
SHAPES = [
    (1, 33, 4, 1),         # one row, one class, one N tile: roles share blocks
    (128, 40, 32, 16),     # no pad class, one N tile, full batch
    (33, 64, 36, 2),       # two N tiles: exactly as many as classifier jobs
    (100, 33, 100, 10),    # four N tiles, two M tiles
]
# plain: random operands. sharp: h * 16 and w2 * 2, so the non-max
# classes underflow to 0 and p[label] is exactly 1. flat: all-zero w2,
# every logit of a row equal. wild: labels outside [0, C) among valid
# ones (only where C < 16 leaves pad classes for them to name).
CASES = [(s, v) for s in SHAPES for v in ("plain", "sharp", "flat", "wild")
         if not (v == "wild" and s[3] == 16)]
CASE_IDS = ["%s-%s" % ("x".join(map(str, s)), v) for s, v in CASES]
WILD = (-1, None, 15, 16, 1000)      # None: C itself


def _labels(B, C, variant, g):
    y = torch.randint(0, C, (B,), generator=g)
    if variant == "wild":
        wild = torch.tensor([C if v is None else v for v in WILD])
        pick = torch.randint(0, len(wild), (B,), generator=g)
        odd = torch.arange(B) % 2 == 0          # row 0 too: B == 1
        y = torch.where(odd, wild[pick], y)
    return y


def _inputs(shape, variant):
    B, M, H, C = shape
    g = torch.Generator().manual_seed(B + M + H + C)
    x = torch.rand(B, M, generator=g)
    return x.to(DEV, torch.bfloat16), _labels(B, C, variant, g).to(DEV)


def _param_values(shape, variant):
    B, M, H, C = shape
    g = torch.Generator().manual_seed(3 + M + H + C)
    shp = {"w1": (M, H), "b1": (H,), "w2": (H, C), "b2": (C,)}
    vals = {n: torch.randn(*shp[n], generator=g) * 0.1 for n in NAMES}
    if variant == "sharp":
        vals["w2"] = vals["w2"] * 2
    if variant == "flat":
        vals["w2"] = torch.zeros(H, C)
    return vals


def _hidden(x, w1s, b1s, variant):
    h = ops.gemm_bias_act(x, w1s, b1s, act="relu")
    return h * 16 if variant == "sharp" else h      # exact in bf16


class _Store(object):
    """fp32 masters + bf16 shadows, one plain allocation each."""

    def __init__(self, shape, variant):
        vals = _param_values(shape, variant)
        self.m = {n: vals[n].to(DEV) for n in NAMES}
        self.s = {n: self.m[n].to(torch.bfloat16) for n in NAMES}


class _GuardedStore(object):
    """The same values as views into ONE fp32 and ONE bf16 allocation
    filled with 7.0, GUARD or more elements of it around every view."""

    def __init__(self, shape, variant):
        vals = _param_values(shape, variant)
        starts, cur = {}, 0
        for n in NAMES:
            cur = (cur + GUARD + 7) // 8 * 8
            starts[n] = cur
            cur += vals[n].numel()
        total = cur + GUARD
        self.flat_m = torch.full((total,), POISON, device=DEV)
        self.flat_s = torch.full((total,), POISON, device=DEV,
                                 dtype=torch.bfloat16)
        self.live = torch.zeros(total, dtype=torch.bool, device=DEV)
        self.m, self.s = {}, {}
        for n in NAMES:
            a, k = starts[n], vals[n].numel()
            self.live[a:a + k] = True
            self.m[n] = self.flat_m[a:a + k].view(vals[n].shape)
            self.s[n] = self.flat_s[a:a + k].view(vals[n].shape)
            self.m[n].copy_(vals[n])
            self.s[n].copy_(self.m[n].to(torch.bfloat16))

    def assert_guards(self):
        for flat in (self.flat_m, self.flat_s):
            assert bool((flat[~self.live] == POISON).all())


# ------------------------------------------------------------- grads

_OLD_GRADS = {}


def _old_grads(shape, variant, gdt):
    """mlp_head_fused + gemm_bias_act, once per case; never modified."""
    key = (shape, variant, gdt)
    if key not in _OLD_GRADS:
        B, M, H, C = shape
        x, y = _inputs(shape, variant)
        st = _Store(shape, variant)
        h = _hidden(x, st.s["w1"], st.s["b1"], variant)
        dw1 = torch.empty(M, H, device=DEV, dtype=gdt)
        db1 = torch.empty(H, device=DEV, dtype=gdt)
        dw2 = torch.empty(H, C, device=DEV, dtype=gdt)
        db2 = torch.empty(C, device=DEV, dtype=gdt)
        loss, _, dh = ops.mlp_head_fused(h, st.s["w2"], st.s["b2"], y,
                                         dw2=dw2, db2=db2)
        ops.gemm_bias_act(x, dh, trans_a=True, out=dw1, colsum_out=db1)
        torch.cuda.synchronize()
        _OLD_GRADS[key] = (loss, dw1, db1, dw2, db2)
    return _OLD_GRADS[key]


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_grads_equal_head_then_dw1_gemm(case, gdt):
    """All four grads and the loss, every element written (the outputs
    start as 7.0), in both grad dtypes. Every shape here has fewer than
    32 tiles: dW1 through one 16x16x32 accumulator in the tile blocks,
    the serial colsum in the db1 blocks."""
    shape, variant = case
    B, M, H, C = shape
    x, y = _inputs(shape, variant)
    st = _Store(shape, variant)
    h = _hidden(x, st.s["w1"], st.s["b1"], variant)
    out = [torch.full(s, POISON, device=DEV, dtype=gdt)
           for s in ((M, H), (H,), (H, C), (C,))]
    loss = ops.mlp_head_tail_grads(x, h, st.s["w2"], st.s["b2"], y, *out)
    torch.cuda.synchronize()
    want = _old_grads(shape, variant, gdt)
    for n, a, b in zip(("loss", "dw1", "db1", "dw2", "db2"),
                       [loss] + out, want):
        assert a.dtype == b.dtype and a.shape == b.shape, n
        assert torch.equal(a, b), (n, float((a.float() - b.float())
                                            .abs().max()))


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
def test_grads_from_32_tiles_up(gdt):
    """(100, 256, 128, 10): 8 x 4 tiles, the count from which the tile
    blocks keep the small-tile kernel's sum order and the db1 blocks its
    colsum tree."""
    shape = (100, 256, 128, 10)
    B, M, H, C = shape
    x, y = _inputs(shape, "plain")
    st = _Store(shape, "plain")
    h = _hidden(x, st.s["w1"], st.s["b1"], "plain")
    out = [torch.full(s, POISON, device=DEV, dtype=gdt)
           for s in ((M, H), (H,), (H, C), (C,))]
    loss = ops.mlp_head_tail_grads(x, h, st.s["w2"], st.s["b2"], y, *out)
    torch.cuda.synchronize()
    want = _old_grads(shape, "plain", gdt)
    for a, b in zip([loss] + out, want):
        assert torch.equal(a, b)


# ---------------------------------------------------------- SGD step

def _old_step(x, y, st, variant):
    h = _hidden(x, st.s["w1"], st.s["b1"], variant)
    gw2 = torch.empty_like(st.s["w2"])
    gb2 = torch.empty_like(st.s["b2"])
    loss, _, dh = ops.mlp_head_fused(h, st.s["w2"], st.s["b2"], y,
                                     dw2=gw2, db2=gb2)
    ops.mlp_tail_sgd(x, dh, st.m["w1"], st.s["w1"], st.m["b1"], st.s["b1"],
                     gw2, st.m["w2"], st.s["w2"], gb2, st.m["b2"],
                     st.s["b2"], LR)
    return loss


_OLD_STEPS = {}


def _old_after(shape, variant, steps):
    """The oracle's store and losses after `steps` steps: computed once
    per case, shared and never modified."""
    key = (shape, variant, steps)
    if key not in _OLD_STEPS:
        x, y = _inputs(shape, variant)
        st = _Store(shape, variant)
        losses = [_old_step(x, y, st, variant) for _ in range(steps)]
        torch.cuda.synchronize()
        _OLD_STEPS[key] = (st, losses)
    return _OLD_STEPS[key]


_CARRIER = []


def _snapshot(w2s, b2s):
    """A one-launch forward (4 K slices) that takes the snapshot."""
    if not _CARRIER:
        plan = ops._ext().gemm_plan(16, 8, 256, False, False, 1, False, 0)
        assert (plan[0], plan[3]) == ("fwd1", "none")
        g = torch.Generator().manual_seed(16)
        bf = lambda t: t.to(DEV, torch.bfloat16)
        _CARRIER.append((bf(torch.rand(16, 256, generator=g)),
                         bf(torch.randn(256, 8, generator=g) * 0.1),
                         bf(torch.zeros(8))))
    _, snap = ops.mlp_fwd_snap(*_CARRIER[0], w2s, b2s)
    assert snap is not None
    return snap


def _new_step(x, y, st, variant, mode):
    h = _hidden(x, st.s["w1"], st.s["b1"], variant)
    snap = _snapshot(st.s["w2"], st.s["b2"]) if mode == "snapshot" else None
    return ops.mlp_head_tail_sgd(
        x, h, st.s["w2"], st.s["b2"], y, st.m["w1"], st.m["b1"], st.m["w2"],
        st.m["b2"], st.s["w1"], st.s["b1"], LR, snap=snap)


def _assert_stores_equal(a, b):
    for n in NAMES:
        assert torch.equal(a.m[n], b.m[n]), ("master", n)
        assert torch.equal(a.s[n], b.s[n]), ("shadow", n)


@pytest.mark.parametrize("mode", ["snapshot", "ticket"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_three_sgd_steps_equal_head_then_tail(case, mode):
    """Losses, masters and shadows after each of three steps; the applies
    come from different blocks (W1 from the tiles, b1 from the db1
    blocks, W2 and b2 from one classifier block each), and none of them
    may touch the bands between the views."""
    shape, variant = case
    x, y = _inputs(shape, variant)
    old, old_losses = _old_after(shape, variant, 3)
    new = _GuardedStore(shape, variant)
    for i in range(3):
        loss = _new_step(x, y, new, variant, mode)
        assert torch.equal(loss, old_losses[i]), ("loss", i)
    torch.cuda.synchronize()
    _assert_stores_equal(new, old)
    new.assert_guards()


def test_snapshot_step_graph_replay():
    """One captured snapshot step at (33, 64, 36, 2) replayed five times
    behind one eager step == six eager steps of the oracle route."""
    shape, variant = SHAPES[2], "plain"
    x, y = _inputs(shape, variant)
    old, old_losses = _old_after(shape, variant, 6)
    new = _GuardedStore(shape, variant)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _new_step(x, y, new, variant, "snapshot")
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = _new_step(x, y, new, variant, "snapshot")
    for _ in range(5):                 # capture itself runs nothing
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, old_losses[5])
    _assert_stores_equal(new, old)
    new.assert_guards()
