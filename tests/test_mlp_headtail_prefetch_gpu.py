"""The fused head+tail kernel fetches every fp32 master it updates at its
top, through unconditional loads from clamped addresses, and keeps the
values in registers until after the barrier (csrc/gemm.hip,
mlp_head_tail_kernel / small_sgd_fetch). What that can break: a clamped
load whose value leaks, a read or write outside a view, a fallback for
views a vector access cannot take, and the order of master reads and
writes across launches. All comparisons are EXACT against the
two-kernel sequence (ops.mlp_head_fused -> ops.mlp_tail_sgd), built as
in tests/test_mlp_headtail_gpu.py."""

import math

import pytest
import torch

from tfmesos_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR = 0.05

# (B, M, H, C)
SHAPES = [
    (100, 784, 100, 10),   # the benchmark shape
    (33, 40, 36, 3),       # ragged M and N tiles; second wave holds one row
    (7, 33, 4, 1),         # M % 8 != 0; three idle waves; one class
    (128, 64, 128, 16),    # all limits full
]
IDS = ["x".join(map(str, s)) for s in SHAPES]
NAMES = ("w1", "b1", "w2", "b2")
GUARD = 64


def _inputs(B, M, H, C, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + B + M + H + C)
    x = torch.rand(B, M, generator=g)
    h = torch.relu(torch.randn(B, H, generator=g))
    w2 = torch.randn(H, C, generator=g) * 0.1
    b2 = torch.randn(C, generator=g) * 0.1
    y = torch.randint(0, C, (B,), generator=g)
    bf = lambda t: t.to(device=DEV, dtype=torch.bfloat16)
    return bf(x), bf(h), bf(w2), bf(b2), y.to(DEV)


def _param_values(M, H, C, seed=3):
    g = torch.Generator().manual_seed(seed + M + H + C)
    shp = {"w1": (M, H), "b1": (H,), "w2": (H, C), "b2": (C,)}
    return {n: torch.randn(*shp[n], generator=g) * 0.1 for n in NAMES}


class _Store(object):
    """fp32 masters + bf16 shadows, one aligned allocation each."""

    def __init__(self, M, H, C):
        vals = _param_values(M, H, C)
        self.m = {n: vals[n].to(DEV) for n in NAMES}
        self.s = {n: self.m[n].to(torch.bfloat16) for n in NAMES}


class _FlatStore(object):
    """The same values as views into ONE flat fp32 master buffer and ONE
    flat bf16 shadow buffer, as the trainer's store lays them out, each
    view with at least GUARD sentinel elements before and after it.
    skew: every master view starts 4 bytes and every shadow view 2 bytes
    past a 16-byte boundary; else all views are 16-byte aligned. fill:
    the sentinel (NaN poisons whatever leaks out of a neighbour)."""

    def __init__(self, M, H, C, skew=False, fill=-512.0):
        vals = _param_values(M, H, C)
        starts, cur = {}, 0
        for n in NAMES:
            cur = (cur + GUARD + 7) // 8 * 8 + (1 if skew else 0)
            starts[n] = cur
            cur += vals[n].numel()
        total = cur + GUARD
        self.fill = fill
        self.flat_m = torch.full((total,), fill, device=DEV)
        self.flat_s = torch.full((total,), fill, device=DEV,
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
            want_m, want_s = (4, 2) if skew else (0, 0)
            assert self.m[n].data_ptr() % 16 == want_m
            assert self.s[n].data_ptr() % 16 == want_s

    def assert_guards(self):
        for flat in (self.flat_m, self.flat_s):
            g = flat[~self.live].float()
            if self.fill != self.fill:
                assert bool(torch.isnan(g).all())
            else:
                assert bool((g == self.fill).all())


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


def _new_step(x, y, st, lr, snapshot, rehome=None):
    """snapshot=False: live shadow + arrival ticket. True: W2/b2 from
    the snapshot of the fwd launch where it takes one, else the ticket.
    rehome: moves h into another allocation before the fused kernel."""
    snap = None
    if snapshot:
        h, snap = ops.mlp_fwd_snap(x, st.s["w1"], st.s["b1"], st.s["w2"],
                                   st.s["b2"])
    else:
        h = _fwd(x, st)
    if rehome is not None:
        h = rehome(h)
    return ops.mlp_head_tail_sgd(
        x, h, st.s["w2"], st.s["b2"], y, st.m["w1"], st.m["b1"],
        st.m["w2"], st.m["b2"], st.s["w1"], st.s["b1"], lr, snap=snap)


def _assert_stores_equal(a, b):
    for n in NAMES:
        assert torch.equal(a.m[n], b.m[n]), ("master", n)
        assert torch.equal(a.s[n], b.s[n]), ("shadow", n)
        assert torch.equal(a.s[n], a.m[n].to(torch.bfloat16)), ("bf16", n)


_OLD = {}


def _old_after_three(shape):
    """The old path's store and losses after three steps: computed once
    per shape, shared and never modified."""
    if shape not in _OLD:
        B, M, H, C = shape
        x, _, _, _, y = _inputs(*shape)
        st = _Store(M, H, C)
        losses = [_old_step(x, y, st, LR) for _ in range(3)]
        torch.cuda.synchronize()
        _OLD[shape] = (st, losses)
    return _OLD[shape]


MODES = pytest.mark.parametrize("snapshot", [False, True],
                                ids=["ticket", "snapshot"])


@MODES
@pytest.mark.parametrize("skew", [False, True], ids=["aligned", "skewed"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_guarded_flat_store_three_steps(shape, skew, snapshot):
    """Guarded masters (aligned) and misaligned views (skewed): after
    three back-to-back steps the views equal the old path's and every
    sentinel around them is untouched."""
    B, M, H, C = shape
    x, _, _, _, y = _inputs(*shape)
    old, old_losses = _old_after_three(shape)
    new = _FlatStore(M, H, C, skew=skew)
    for i in range(3):
        ln = _new_step(x, y, new, LR, snapshot)
        assert torch.equal(ln, old_losses[i])
    torch.cuda.synchronize()
    _assert_stores_equal(new, old)
    new.assert_guards()


@MODES
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_poisoned_neighbours_do_not_leak(shape, snapshot):
    """NaN after the rows of h and x, a wild label tail, and NaN all
    around W2/b2 (and the other views) in their allocations: a clamped
    load whose value is not dropped shows up in the results."""
    B, M, H, C = shape
    x, _, _, _, y = _inputs(*shape)
    old, old_losses = _old_after_three(shape)
    nan = float("nan")
    xbig = torch.full((B + 40, M), nan, device=DEV, dtype=torch.bfloat16)
    xbig[:B] = x
    ybig = torch.full((B + 40,), 2 ** 40, device=DEV, dtype=torch.int64)
    ybig[:B] = y
    hbig = torch.full((B + 40, H), nan, device=DEV, dtype=torch.bfloat16)

    def rehome(h):
        hbig[:B] = h
        return hbig[:B]

    new = _FlatStore(M, H, C, fill=nan)
    for i in range(3):
        ln = _new_step(xbig[:B], ybig[:B], new, LR, snapshot, rehome)
        assert torch.equal(ln, old_losses[i])
    torch.cuda.synchronize()
    _assert_stores_equal(new, old)
    new.assert_guards()


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[0]],
                         ids=[IDS[1], IDS[0]])
def test_graph_replay_reads_the_previous_steps_store(shape):
    """One captured snapshot-mode step replayed 5 times after 3 eager
    warm-ups == 8 eager old-path steps: the master a step fetches at its
    top is the value the step before it stored."""
    B, M, H, C = shape
    x, _, _, _, y = _inputs(*shape)
    old, new = _Store(M, H, C), _FlatStore(M, H, C)
    for _ in range(8):
        _old_step(x, y, old, LR)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):             # eager warm-ups (allocates the ticket)
            _new_step(x, y, new, LR, True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _new_step(x, y, new, LR, True)
    for _ in range(5):                 # capture itself runs nothing
        graph.replay()
    torch.cuda.synchronize()
    _assert_stores_equal(new, old)
    new.assert_guards()


def _fma32(m, lr, g):
    """fp32 m - lr * g with ONE rounding, as the kernels' v_fma_f32: the
    product of two fp32 values is exact in fp64, so only the final
    fp64 -> fp32 step rounds twice, and only where the fp64 sum lands
    within 2^-53 of an fp32 tie (about 1e-9 per element)."""
    lr32 = torch.tensor(lr, dtype=torch.float32).double().item()
    return (m.double() - lr32 * g.double()).float()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]],
                         ids=[IDS[0], IDS[2]])
def test_tail_sgd_alone_matches_gemm_plus_torch_sgd(shape):
    """ops.mlp_tail_sgd (gemm_small_kernel's apply, masters fetched at
    the top, load-all-then-store-all classifier wave) == the dW1 / db1
    of gemm_bias_act followed by a torch fp32 SGD with the kernel's
    rounding (fused multiply-add, bf16 round-to-nearest-even shadow).
    At the benchmark shape gemm_bias_act runs dW1 on the same small-tile
    kernel, so random data compares exactly. At 7x33x4x1 it runs the
    64x64 kernel, which sums K in another order: there x and dh are
    multiples of 1/64 below 2 in magnitude, so every product is a
    multiple of 2^-12, every partial sum stays below 2^4 * 2^12 = 2^16
    units — exact in fp32 in any order — and the two kernels must agree
    to the bit."""
    B, M, H, C = shape
    g = torch.Generator().manual_seed(77 + B + M)
    if M * H >= 32 * 32 * 32:
        x = torch.rand(B, M, generator=g)
        dh = torch.randn(B, H, generator=g) * 0.01
    else:
        x = torch.randint(0, 64, (B, M), generator=g).float() / 64
        dh = torch.randint(-127, 128, (B, H), generator=g).float() / 64
    dh = dh * (torch.rand(B, H, generator=g) > 0.5)   # relu-masked zeros
    x = x.to(DEV, torch.bfloat16)
    dh = dh.to(DEV, torch.bfloat16)
    gw2 = (torch.randn(H, C, generator=g) * 0.1).to(DEV, torch.bfloat16)
    gb2 = (torch.randn(C, generator=g) * 0.1).to(DEV, torch.bfloat16)
    st = _FlatStore(M, H, C)
    want = {n: st.m[n].clone() for n in NAMES}

    dw1 = torch.empty(M, H, device=DEV, dtype=torch.float32)
    db1 = torch.empty(H, device=DEV, dtype=torch.float32)
    ops.gemm_bias_act(x, dh, trans_a=True, out=dw1, colsum_out=db1)
    grads = {"w1": dw1, "b1": db1, "w2": gw2.float(), "b2": gb2.float()}

    ops.mlp_tail_sgd(x, dh, st.m["w1"], st.s["w1"], st.m["b1"], st.s["b1"],
                     gw2, st.m["w2"], st.s["w2"], gb2, st.m["b2"],
                     st.s["b2"], LR)
    torch.cuda.synchronize()
    for n in NAMES:
        ref = _fma32(want[n], LR, grads[n])
        assert torch.equal(st.m[n], ref), ("master", n)
        assert torch.equal(st.s[n], ref.to(torch.bfloat16)), ("shadow", n)
    st.assert_guards()


def _head_reference(h, w, b, y):
    """As tests/test_kernels_gpu.py composes it: logits GEMM, softmax
    xent (the same 1e-30 clamp), dW2 GEMM."""
    H, C = w.shape
    logits = ops.gemm_bias_act(h, w, b)
    loss, dl = ops.softmax_xent_fused(logits, y)
    dw2 = torch.zeros(H, C, device=DEV, dtype=torch.float32)
    db2 = torch.zeros(C, device=DEV, dtype=torch.float32)
    ops.gemm_bias_act(h, dl, trans_a=True, out=dw2, colsum_out=db2)
    return loss, dl, dw2


def _check_head(h, w, b, y, want_loss=None):
    H, C = w.shape
    dw2 = torch.zeros(H, C, device=DEV, dtype=torch.float32)
    db2 = torch.zeros(C, device=DEV, dtype=torch.float32)
    loss, dl, _ = ops.mlp_head_fused(h, w, b, y, dw2=dw2, db2=db2)
    # the composed GPU pipeline and the CPU path of the same op, at the
    # tolerances of test_mlp_head_fused_matches_composed
    loss_c, dl_c, dw2_c = _head_reference(h, w, b, y)
    dw2_cpu = torch.zeros(H, C)
    db2_cpu = torch.zeros(C)
    _, dl_cpu, _ = ops.mlp_head_fused(h.cpu(), w.cpu(), b.cpu(), y.cpu(),
                                      dw2=dw2_cpu, db2=db2_cpu)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_c)) < 1e-2
    if want_loss is not None:
        assert abs(float(loss) - want_loss) < 1e-2
    for ref_dl, ref_dw2 in ((dl_c.float().cpu(), dw2_c.cpu()),
                            (dl_cpu.float(), dw2_cpu)):
        assert (dl.float().cpu() - ref_dl).abs().max() < 1e-3
        assert (dw2.cpu() - ref_dw2).abs().max() < \
            2e-3 * ref_dw2.abs().max() + 1e-4


def test_softmax_row_label_probability_below_the_clamp():
    """Row 0's label has p = exp(-128) = 0 in fp32: its loss is the
    clamp, -log(1e-30), taken once after the class loop. The CPU path
    has no clamp (that row would cost 128), so the loss is checked
    against the composed pipeline, which has the same one, and against
    the value worked out by hand; dlogits and dW2 against both."""
    B, H, C = 8, 16, 4
    h = torch.ones(B, H)
    w = torch.zeros(H, C)
    w[:, 0], w[:, 1] = 4.0, -4.0          # logits 64 and -64
    b = torch.zeros(C)
    y = torch.zeros(B, dtype=torch.int64)
    y[0] = 1
    bf = lambda t: t.to(DEV, torch.bfloat16)
    _check_head(bf(h), bf(w), bf(b), y.to(DEV),
                want_loss=-math.log(1e-30) / B)


def test_softmax_row_single_class():
    B, H, C = 7, 4, 1
    _, h, w, b, y = _inputs(B, 33, H, C)
    _check_head(h, w, b, y, want_loss=0.0)
