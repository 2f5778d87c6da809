"""Data movement of the fused head+tail kernel (csrc/gemm.hip,
mlp_head_tail_kernel): the snapshot's producer lays the two classifier
images out once (SnapJob) and the snapshot instantiation moves them as
b128 chunks; x, h, b2, the labels and the fp32 masters come through
range-checked buffer loads whose extent is that of the VIEW passed. What
can break: an extent that is too large (a neighbour leaks in), one that
is too small (live data reads as zero), a folded lane predicate, residue
of an earlier classifier in the padded images, a write outside a view.

The oracle is the two-kernel route, ops.mlp_head_fused followed by
ops.mlp_tail_sgd, on plain tensors. Every comparison is EXACT
(torch.equal) over three consecutive steps: the arithmetic, the MFMA
shapes and every summation order are the same, only the way operands
reach LDS and registers differs, so there is no rounding to allow for.

The snapshot is a function of the classifier alone, so the shapes whose
own forward GEMM takes none (inputs < 256: no K slicing) get theirs from
a carrier GEMM on either kernel that takes one."""

import pytest
import torch

from tfmesos_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR = 0.05
NAN = float("nan")
GUARD = 64
NAMES = ("w1", "b1", "w2", "b2")
WILD_LABEL = 0x700001234      # out of range, and so is its low dword

# (B, M, H, C)
SHAPES = [
    (100, 784, 100, 10),   # the benchmark's own tails
    (128, 64, 128, 16),    # nothing padded: every range check at the extent
    (33, 40, 36, 3),       # wave 1 owns one row; second N tile 4 wide; C < 4
    (1, 36, 64, 1),        # M % 8 != 0: element path of x; one row, one class
    (97, 72, 68, 10),      # odd batch; H % 32 == 4
]
IDS = ["x".join(map(str, s)) for s in SHAPES]

# snapshot layout (bf16 elements), csrc/common.h
B2_OFF, KMAJ_OFF, HP, CP, HB = 2048, 2112, 136, 16, 128
ROW_OFF = KMAJ_OFF + CP * HP
SNAP_ELEMS = ROW_OFF + HB * CP


def _inputs(B, M, H, C, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + B + M + H + C)
    x = torch.rand(B, M, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    return x.to(DEV, torch.bfloat16), y.to(DEV)


def _param_values(M, H, C, seed=3):
    g = torch.Generator().manual_seed(seed + M + H + C)
    shp = {"w1": (M, H), "b1": (H,), "w2": (H, C), "b2": (C,)}
    return {n: torch.randn(*shp[n], generator=g) * 0.1 for n in NAMES}


class _Store(object):
    """fp32 masters + bf16 shadows, one plain allocation each."""

    def __init__(self, M, H, C):
        vals = _param_values(M, H, C)
        self.m = {n: vals[n].to(DEV) for n in NAMES}
        self.s = {n: self.m[n].to(torch.bfloat16) for n in NAMES}


class _GuardedStore(object):
    """The same values as views into ONE flat fp32 buffer and ONE flat
    bf16 buffer filled with NaN, at least GUARD sentinels around each
    view. off: elements past a 16-byte boundary at which every view
    starts (2-byte shadows and 4-byte masters may start anywhere)."""

    def __init__(self, M, H, C, off=0):
        vals = _param_values(M, H, C)
        starts, cur = {}, 0
        for n in NAMES:
            cur = (cur + GUARD + 7) // 8 * 8 + off
            starts[n] = cur
            cur += vals[n].numel()
        total = cur + GUARD
        self.flat_m = torch.full((total,), NAN, device=DEV)
        self.flat_s = torch.full((total,), NAN, device=DEV,
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
            assert bool(torch.isnan(flat[~self.live].float()).all())


class _Operands(object):
    """x, h and the labels as views inside larger allocations: NaN before
    and after x and h, out-of-range labels before and after y. x starts
    `xoff`, h `hoff` and y `yoff` elements into its storage."""

    def __init__(self, x, y, H, xoff=0, hoff=0, yoff=0):
        B, M = x.shape
        pad = 40 * max(M, H)
        self.xbuf = torch.full((xoff + B * M + pad,), NAN, device=DEV,
                               dtype=torch.bfloat16)
        self.x = self.xbuf[xoff:xoff + B * M].view(B, M)
        self.x.copy_(x)
        self.hbuf = torch.full((hoff + B * H + pad,), NAN, device=DEV,
                               dtype=torch.bfloat16)
        self.hview = self.hbuf[hoff:hoff + B * H].view(B, H)
        self.ybuf = torch.full((yoff + B + 40,), WILD_LABEL, device=DEV,
                               dtype=torch.int64)
        self.y = self.ybuf[yoff:yoff + B]
        self.y.copy_(y)

    def h(self, h):
        self.hview.copy_(h)
        return self.hview


def _fwd(x, st):
    return ops.gemm_bias_act(x, st.s["w1"], st.s["b1"], act="relu")


def _old_step(x, y, st, lr):
    h = _fwd(x, st)
    gw2 = torch.empty_like(st.s["w2"])
    gb2 = torch.empty_like(st.s["b2"])
    loss, _, dh = ops.mlp_head_fused(h, st.s["w2"], st.s["b2"], y,
                                     dw2=gw2, db2=gb2)
    ops.mlp_tail_sgd(x, dh, st.m["w1"], st.s["w1"], st.m["b1"], st.s["b1"],
                     gw2, st.m["w2"], st.s["w2"], gb2, st.m["b2"],
                     st.s["b2"], lr)
    return loss


_CARRIER = {}


def _carrier(kind):
    """A forward GEMM whose launch takes the snapshot: "fwd1" on the
    one-launch forward (4 K slices, so its 4 waves loop over the 9 chunk
    groups), "reduce" on split-K stripes + the small stripe reduce."""
    if kind not in _CARRIER:
        rows = {"fwd1": 16, "reduce": 130}[kind]
        plan = ops._ext().gemm_plan(rows, 8, 256, False, False, 1, False, 0)
        assert (plan[0], plan[3]) == {"fwd1": ("fwd1", "none"),
                                      "reduce": ("tile_sk", "reduce1")}[kind]
        g = torch.Generator().manual_seed(rows)
        bf = lambda t: t.to(DEV, torch.bfloat16)
        _CARRIER[kind] = (bf(torch.rand(rows, 256, generator=g)),
                          bf(torch.randn(256, 8, generator=g) * 0.1),
                          bf(torch.zeros(8)))
    return _CARRIER[kind]


def _snapshot(kind, w2s, b2s):
    xc, w1c, b1c = _carrier(kind)
    _, snap = ops.mlp_fwd_snap(xc, w1c, b1c, w2s, b2s)
    assert snap is not None and snap.numel() == SNAP_ELEMS
    return snap


def _new_step(op, st, lr, mode):
    """mode "ticket": live shadow + arrival ticket; "own": the snapshot
    of the step's own forward; "fwd1" / "reduce": that of a carrier."""
    snap = None
    if mode == "own":
        h, snap = ops.mlp_fwd_snap(op.x, st.s["w1"], st.s["b1"], st.s["w2"],
                                   st.s["b2"])
        assert snap is not None
    else:
        h = _fwd(op.x, st)
        if mode != "ticket":
            snap = _snapshot(mode, st.s["w2"], st.s["b2"])
    return ops.mlp_head_tail_sgd(
        op.x, op.h(h), st.s["w2"], st.s["b2"], op.y, st.m["w1"], st.m["b1"],
        st.m["w2"], st.m["b2"], st.s["w1"], st.s["b1"], lr, snap=snap)


def _assert_stores_equal(a, b):
    for n in NAMES:
        assert torch.equal(a.m[n], b.m[n]), ("master", n)
        assert torch.equal(a.s[n], b.s[n]), ("shadow", n)


_OLD = {}


def _old_after(shape, steps=3):
    """The oracle's store and losses after `steps` steps: computed once
    per shape, shared and never modified."""
    key = (shape, steps)
    if key not in _OLD:
        B, M, H, C = shape
        x, y = _inputs(*shape)
        st = _Store(M, H, C)
        losses = [_old_step(x, y, st, LR) for _ in range(steps)]
        torch.cuda.synchronize()
        _OLD[key] = (st, losses)
    return _OLD[key]


def _three_steps(shape, mode, off=0, xoff=0, hoff=0):
    B, M, H, C = shape
    x, y = _inputs(*shape)
    old, old_losses = _old_after(shape)
    op = _Operands(x, y, H, xoff=xoff, hoff=hoff, yoff=off)
    new = _GuardedStore(M, H, C, off=off)
    for i in range(3):
        ln = _new_step(op, new, LR, mode)
        assert torch.equal(ln, old_losses[i]), ("loss", i)
    torch.cuda.synchronize()
    _assert_stores_equal(new, old)
    new.assert_guards()


@pytest.mark.parametrize("mode", ["fwd1", "reduce", "ticket"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_three_steps_inside_poisoned_storage(shape, mode):
    """Every operand a view with NaN (labels: wild values) around it,
    masters and shadows between NaN guard bands that must survive."""
    _three_steps(shape, mode)


def test_benchmark_shape_own_forward_snapshot():
    """As the model runs it: the step's own forward takes the snapshot
    (9 K slices: one chunk group per wave, loaded ahead of the GEMM)."""
    _three_steps(SHAPES[0], "own")


@pytest.mark.parametrize("mode", ["fwd1", "ticket"])
@pytest.mark.parametrize("off", [2, 4, 8])
def test_views_offset_into_their_storage(off, mode):
    """Masters, shadows (w2/b2 among them) and labels start 2, 4 and 8
    elements into their storage; h, which the op wants 8-byte aligned,
    4 or 8 elements; x, which it wants 16-byte aligned, 8."""
    _three_steps(SHAPES[2], mode, off=off, xoff=8, hoff=max(off, 4))


def _expected_images(w2s):
    H, C = w2s.shape
    kmaj = torch.zeros(CP, HP, device=DEV, dtype=torch.bfloat16)
    kmaj[:C, :H] = w2s.t()
    rows = torch.zeros(HB, CP, device=DEV, dtype=torch.bfloat16)
    rows[:H, :C] = w2s
    return kmaj.flatten(), rows.flatten()


@pytest.mark.parametrize("kind", ["fwd1", "reduce"])
def test_snapshot_images_hold_no_residue(kind):
    """A (128, 16) classifier of non-zero values, then a (36, 3) one: the
    appended images are the second classifier's, zero-padded, the prefix
    keeps its meaning, and a step that reads them equals the oracle."""
    shape = SHAPES[2]
    B, M, H, C = shape
    big_w = torch.full((128, 16), 3.0, device=DEV, dtype=torch.bfloat16)
    big_b = torch.full((16,), 5.0, device=DEV, dtype=torch.bfloat16)
    snap = _snapshot(kind, big_w, big_b)
    torch.cuda.synchronize()
    kmaj, rows = _expected_images(big_w)
    assert torch.equal(snap[KMAJ_OFF:ROW_OFF], kmaj)
    assert torch.equal(snap[ROW_OFF:], rows)

    st = _Store(M, H, C)
    w2_before, b2_before = st.s["w2"].clone(), st.s["b2"].clone()
    snap = _snapshot(kind, st.s["w2"], st.s["b2"])
    torch.cuda.synchronize()
    assert torch.equal(snap[:H * C].view(H, C), w2_before)
    assert torch.equal(snap[B2_OFF:B2_OFF + C], b2_before)
    kmaj, rows = _expected_images(w2_before)
    assert torch.equal(snap[KMAJ_OFF:ROW_OFF], kmaj)
    assert torch.equal(snap[ROW_OFF:], rows)
    _three_steps(shape, kind)


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[0]],
                         ids=[IDS[2], IDS[0]])
def test_graph_replay(shape):
    """One captured snapshot-mode step replayed five times after three
    eager steps == eight eager steps of the oracle route."""
    B, M, H, C = shape
    mode = "own" if M >= 256 else "fwd1"
    x, y = _inputs(*shape)
    old, _ = _old_after(shape, steps=8)
    op = _Operands(x, y, H)
    new = _GuardedStore(M, H, C)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            _new_step(op, new, LR, mode)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = _new_step(op, new, LR, mode)
    for _ in range(5):                 # capture itself runs nothing
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, _old_after(shape, steps=8)[1][7])
    _assert_stores_equal(new, old)
    new.assert_guards()


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_grads_mode_inside_poisoned_storage(shape, f32):
    """ops.mlp_head_tail_grads shares the range-checked loads: with every
    operand inside NaN storage it returns what it returns on plain
    tensors, and dW2 / db2 / loss equal the head kernel's."""
    B, M, H, C = shape
    x, y = _inputs(*shape)
    st = _Store(M, H, C)
    h = _fwd(x, st)
    dt = torch.float32 if f32 else torch.bfloat16

    def grads(xx, hh, w2, b2, yy):
        out = [torch.full(s, NAN, device=DEV, dtype=dt)
               for s in ((M, H), (H,), (H, C), (C,))]
        loss = ops.mlp_head_tail_grads(xx, hh, w2, b2, yy, *out)
        return [loss] + out

    plain = grads(x, h, st.s["w2"], st.s["b2"], y)
    op = _Operands(x, y, H)
    gs = _GuardedStore(M, H, C)
    poisoned = grads(op.x, op.h(h), gs.s["w2"], gs.s["b2"], op.y)
    gw2 = torch.empty(H, C, device=DEV, dtype=dt)
    gb2 = torch.empty(C, device=DEV, dtype=dt)
    loss, _, _ = ops.mlp_head_fused(h, st.s["w2"], st.s["b2"], y, dw2=gw2,
                                    db2=gb2)
    torch.cuda.synchronize()
    for a, b in zip(plain, poisoned):
        assert torch.equal(a, b)
    assert torch.equal(plain[0], loss)
    assert torch.equal(plain[3], gw2) and torch.equal(plain[4], gb2)
    gs.assert_guards()
