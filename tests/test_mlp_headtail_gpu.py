"""Fused classifier head + dW1 tail (ops.mlp_head_tail_grads /
ops.mlp_head_tail_sgd, csrc/gemm.hip mlp_head_tail_kernel) against the
two-kernel sequence it replaces. The fused kernel keeps every sum in
the order of the old kernels, so all comparisons are EXACT."""

import pytest
import torch

from tfmesos_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (B, M, H, C)
SHAPES = [
    (100, 784, 100, 10),   # the benchmark shape
    (128, 64, 128, 16),    # all limits full
    (33, 40, 36, 3),       # second wave holds one row; ragged M and N tiles
    (7, 33, 4, 1),         # M % 8 != 0 scalar loads; one class; 3 idle waves
    (65, 96, 68, 16),      # wave 2 holds one row; third N tile has 4 columns
]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _inputs(B, M, H, C, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + B + M + H + C)
    x = torch.rand(B, M, generator=g)
    # a relu output with exact zeros (about half of the entries)
    h = torch.relu(torch.randn(B, H, generator=g))
    w2 = torch.randn(H, C, generator=g) * 0.1
    b2 = torch.randn(C, generator=g) * 0.1
    y = torch.randint(0, C, (B,), generator=g)
    bf = lambda t: t.to(device=DEV, dtype=torch.bfloat16)
    return bf(x), bf(h), bf(w2), bf(b2), y.to(DEV)


def _old_grads(x, h, w2, b2, y, gdt):
    B, M = x.shape
    H, C = w2.shape
    dw1 = torch.empty(M, H, device=DEV, dtype=gdt)
    db1 = torch.empty(H, device=DEV, dtype=gdt)
    dw2 = torch.empty(H, C, device=DEV, dtype=gdt)
    db2 = torch.empty(C, device=DEV, dtype=gdt)
    loss, _, dh = ops.mlp_head_fused(h, w2, b2, y, dw2=dw2, db2=db2)
    ops.gemm_bias_act(x, dh, trans_a=True, out=dw1, colsum_out=db1)
    return loss, dw1, db1, dw2, db2


def _new_grads(x, h, w2, b2, y, gdt):
    B, M = x.shape
    H, C = w2.shape
    # poisoned outputs: every element must be written
    dw1 = torch.full((M, H), 7.0, device=DEV, dtype=gdt)
    db1 = torch.full((H,), 7.0, device=DEV, dtype=gdt)
    dw2 = torch.full((H, C), 7.0, device=DEV, dtype=gdt)
    db2 = torch.full((C,), 7.0, device=DEV, dtype=gdt)
    loss = ops.mlp_head_tail_grads(x, h, w2, b2, y, dw1, db1, dw2, db2)
    return loss, dw1, db1, dw2, db2


def _assert_same(got, want, names):
    for n, a, b in zip(names, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, n
        assert torch.equal(a, b), (
            n, float((a.float() - b.float()).abs().max()))


GRAD_NAMES = ("loss", "dw1", "db1", "dw2", "db2")


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_grads_match_head_then_dw1_gemm(shape, gdt):
    """Reference: mlp_head_fused(dw2, db2) then gemm_bias_act(x, dh,
    trans_a=True, out, colsum_out), exact equality. Only the benchmark
    shape has the 32 tiles from which gemm_bias_act runs dW1 on the
    small-tile kernel; below, it uses the 64x64 kernel (K chained
    through one 16x16x32 accumulator, serial colsum), and the fused
    kernel's grads mode reproduces that order instead — without it the
    two fp32 cases with B > 64 were 1 ulp off in dW1."""
    inp = _inputs(*shape)
    want = _old_grads(*inp, gdt)
    got = _new_grads(*inp, gdt)
    torch.cuda.synchronize()
    _assert_same(got, want, GRAD_NAMES)


class _Store(object):
    """fp32 masters + bf16 shadows of the four params, seeded."""

    NAMES = ("w1", "b1", "w2", "b2")

    def __init__(self, M, H, C, seed=3):
        g = torch.Generator().manual_seed(seed + M + H + C)
        shp = {"w1": (M, H), "b1": (H,), "w2": (H, C), "b2": (C,)}
        self.m = {n: (torch.randn(*shp[n], generator=g) * 0.1).to(DEV)
                  for n in self.NAMES}
        self.s = {n: self.m[n].to(torch.bfloat16) for n in self.NAMES}


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


def _new_step(x, y, st, lr, snapshot=False):
    """snapshot=False: live shadow + arrival ticket. True: as the model
    runs it — W2/b2 from the snapshot the fwd GEMM's reduce took, where
    that kernel runs (the benchmark shape); else the ticket again."""
    snap = None
    if snapshot:
        h, snap = ops.mlp_fwd_snap(x, st.s["w1"], st.s["b1"], st.s["w2"],
                                   st.s["b2"])
    else:
        h = _fwd(x, st)
    return ops.mlp_head_tail_sgd(
        x, h, st.s["w2"], st.s["b2"], y, st.m["w1"], st.m["b1"],
        st.m["w2"], st.m["b2"], st.s["w1"], st.s["b1"], lr, snap=snap)


def _assert_stores_equal(a, b):
    for n in _Store.NAMES:
        assert torch.equal(a.m[n], b.m[n]), ("master", n)
        assert torch.equal(a.s[n], b.s[n]), ("shadow", n)
        assert torch.equal(a.s[n], a.m[n].to(torch.bfloat16)), ("bf16", n)


@pytest.mark.parametrize("snapshot", [False, True],
                         ids=["ticket", "snapshot"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_sgd_three_steps_match_head_then_tail(shape, snapshot):
    B, M, H, C = shape
    x, _, _, _, y = _inputs(*shape)
    old, new = _Store(M, H, C), _Store(M, H, C)
    for _ in range(3):   # back to back: the ticket resets itself
        lo = _old_step(x, y, old, 0.05)
        ln = _new_step(x, y, new, 0.05, snapshot)
        assert torch.equal(lo, ln)
    torch.cuda.synchronize()
    _assert_stores_equal(new, old)


def test_sgd_alternating_grids_share_the_ticket():
    big, small = SHAPES[0], SHAPES[2]
    runs = []
    for shape in (big, small, big):
        B, M, H, C = shape
        x, _, _, _, y = _inputs(*shape)
        old, new = _Store(M, H, C), _Store(M, H, C)
        lo = _old_step(x, y, old, 0.05)
        ln = _new_step(x, y, new, 0.05)
        runs.append((lo, ln, old, new))
    torch.cuda.synchronize()
    for lo, ln, old, new in runs:
        assert torch.equal(lo, ln)
        _assert_stores_equal(new, old)


def test_fwd_snap_matches_gemm_and_shadows():
    """mlp_fwd_snap's h equals gemm_bias_act's, and the snapshot equals
    the shadows it was taken from."""
    B, M, H, C = SHAPES[0]
    x, _, _, _, _ = _inputs(*SHAPES[0])
    st = _Store(M, H, C)
    h, snap = ops.mlp_fwd_snap(x, st.s["w1"], st.s["b1"], st.s["w2"],
                               st.s["b2"])
    assert snap is not None
    assert torch.equal(h, _fwd(x, st))
    assert torch.equal(snap[:H * C].view(H, C), st.s["w2"])
    assert torch.equal(snap[2048:2048 + C], st.s["b2"])


@pytest.mark.parametrize("snapshot", [False, True],
                         ids=["ticket", "snapshot"])
def test_sgd_graph_replay_matches_eager_old_path(snapshot):
    B, M, H, C = SHAPES[0]
    x, _, _, _, y = _inputs(*SHAPES[0])
    old, new = _Store(M, H, C), _Store(M, H, C)
    for _ in range(8):
        _old_step(x, y, old, 0.05)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):             # eager warm-ups (allocates the ticket)
            _new_step(x, y, new, 0.05, snapshot)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _new_step(x, y, new, 0.05, snapshot)
    for _ in range(5):                 # capture itself runs nothing
        graph.replay()
    torch.cuda.synchronize()
    _assert_stores_equal(new, old)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[3]],
                         ids=[IDS[0], IDS[2], IDS[3]])
def test_padding_sources_do_not_leak(shape):
    """Rows of the h allocation beyond B, and labels beyond B, feed the
    zero-padded LDS images if a bound is off by one: poison them."""
    B, M, H, C = shape
    x, h, w2, b2, y = _inputs(*shape)
    want = _new_grads(x, h, w2, b2, y, torch.float32)
    hbig = torch.full((128 + 32, H), float("nan"), device=DEV,
                      dtype=torch.bfloat16)
    hbig[:B] = h
    ybig = torch.full((128 + 32,), 2 ** 40, device=DEV, dtype=torch.int64)
    ybig[:B] = y
    got = _new_grads(x, hbig[:B], w2, b2, ybig[:B], torch.float32)
    torch.cuda.synchronize()
    _assert_same(got, want, GRAD_NAMES)
