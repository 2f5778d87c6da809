"""One-launch split-K forward (csrc/gemm.hip gemm_fwd1_kernel,
ops.gemm_bias_act(route="fwd1")) against the split-K stripes + reduce
route it replaces (route="stripes"). The one-launch kernel chains the
same MFMAs per K slice and sums the slices in the same order, so every
comparison is torch.equal; there is no tolerance anywhere."""

import pytest
import torch

from tfmesos_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 7.0

# (M, N, K) -> (kc, nslice) by the binding's formula
SHAPES = [
    (100, 100, 784),   # the benchmark shape; last slice half a k-step deep
    (128, 128, 256),   # limits full; smallest K that slices
    (33, 40, 1024),    # 16 slices; a fragment with 8 live columns
    (7, 4, 260),       # unaligned pitches: guarded loads; mostly padding
    (65, 17, 300),     # odd N: misaligned B rows; last slice 12 deep
    # beyond the issue's table: the three offsets a B chunk straddling N
    # is shifted by (N % 8 = 2, 4 is the benchmark, 6), an odd A pitch
    # with vector B, and a slice longer than the 3 k-steps in flight
    (20, 98, 320),
    (20, 102, 320),
    (20, 24, 263),
    (24, 40, 2560),
]
KC_NSLICE = {
    (100, 100, 784): (96, 9),
    (128, 128, 256): (64, 4),
    (33, 40, 1024): (64, 16),
    (7, 4, 260): (96, 3),
    (65, 17, 300): (96, 4),
    (20, 98, 320): (64, 5),
    (20, 102, 320): (64, 5),
    (20, 24, 263): (96, 3),
    (24, 40, 2560): (160, 16),
}
IDS = ["x".join(map(str, s)) for s in SHAPES]
UNALIGNED = [(100, 100, 784), (7, 4, 260), (65, 17, 300)]


def _slicing(M, N, K):
    """kc / nslice as gemm_bias_act_impl computes them (no colsum)."""
    nx, ny = (N + 63) // 64, (M + 63) // 64
    if nx * ny >= 256 or K < 256:
        return 0, 1
    want = min(K // 64, 256 // (nx * ny), 16)
    if want <= 1:
        return 0, 1
    kc = ((K + want - 1) // want + 31) // 32 * 32
    return kc, (K + kc - 1) // kc


def _inputs(M, N, K, bias_dt):
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K)
    x = torch.rand(M, K, generator=g)
    w = torch.randn(K, N, generator=g) * 0.1
    # w is zero-mean, so relu clips about half of x @ w
    b = None
    if bias_dt is not None:
        b = (torch.randn(N, generator=g) * 0.1).to(device=DEV, dtype=bias_dt)
    bf = lambda t: t.to(device=DEV, dtype=torch.bfloat16)
    return bf(x), bf(w), b


def _run(route, x, w, b, act, out_dt, **kw):
    out = torch.full((x.shape[0], w.shape[1]), POISON, device=DEV,
                     dtype=out_dt)
    r = ops.gemm_bias_act(x, w, b, act=act, out=out, route=route, **kw)
    assert r is out
    return out


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert torch.equal(a, b), float((a.float() - b.float()).abs().max())


def test_slicing_table():
    for s in SHAPES:
        assert _slicing(*s) == KC_NSLICE[s], s


@pytest.mark.parametrize("out_dt", [torch.bfloat16, torch.float32],
                         ids=["obf16", "of32"])
@pytest.mark.parametrize("bias_dt", [None, torch.bfloat16, torch.float32],
                         ids=["nobias", "bbf16", "bf32"])
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_matches_stripes_route(shape, act, bias_dt, out_dt):
    x, w, b = _inputs(*shape, bias_dt)
    want = _run("stripes", x, w, b, act, out_dt)
    got = _run("fwd1", x, w, b, act, out_dt)
    _same(got, want)
    if act == "relu" and shape[0] * shape[1] >= 1000:
        frac = float((want == 0).float().mean())
        assert 0.2 < frac < 0.8, frac   # relu really clips
    if shape[0] <= 128 and shape[1] <= 128:
        _same(_run("auto", x, w, b, act, out_dt), want)


@pytest.mark.parametrize("variant", ["16x16", "16x32", "32x16", "32x32",
                                     "16x16s", "32x32s"])
@pytest.mark.parametrize("shape", SHAPES[:5], ids=IDS[:5])
def test_every_geometry_matches(shape, variant):
    x, w, b = _inputs(*shape, torch.bfloat16)
    want = _run("stripes", x, w, b, "relu", torch.bfloat16)
    got = _run("fwd1", x, w, b, "relu", torch.bfloat16, fwd1_variant=variant)
    _same(got, want)


@pytest.mark.parametrize("shape", UNALIGNED,
                         ids=["x".join(map(str, s)) for s in UNALIGNED])
def test_padding_sources_do_not_leak(shape):
    """Operands taken as leading slices of NaN-filled allocations: what
    lies behind them must never reach a live output."""
    M, N, K = shape
    x, w, b = _inputs(M, N, K, torch.bfloat16)
    clean = _run("fwd1", x, w, b, "relu", torch.float32)

    def padded(t):
        big = torch.full((t.numel() + 4096,), float("nan"), device=DEV,
                         dtype=t.dtype)
        big[:t.numel()] = t.reshape(-1)
        return big[:t.numel()].view(t.shape)

    got = _run("fwd1", padded(x), padded(w), padded(b), "relu",
               torch.float32)
    assert not torch.isnan(got).any()
    _same(got, clean)
    _same(got, _run("stripes", x, w, b, "relu", torch.float32))


@pytest.mark.parametrize("dims", [(100, 784, 100, 10), (33, 1024, 40, 3)],
                         ids=["bench", "33x1024x40x3"])
def test_snapshot_rides_the_one_launch_forward(dims):
    B, P, H, C = dims
    x, w1, b1 = _inputs(B, H, P, torch.bfloat16)
    g = torch.Generator().manual_seed(5)
    w2 = (torch.randn(H, C, generator=g) * 0.1).to(DEV, torch.bfloat16)
    b2 = (torch.randn(C, generator=g) * 0.1).to(DEV, torch.bfloat16)
    # a snapshot buffer left over from another classifier must not pass
    ops.mlp_fwd_snap(x, w1, b1, torch.zeros_like(w2), torch.zeros_like(b2))
    h, snap = ops.mlp_fwd_snap(x, w1, b1, w2, b2)
    assert snap is not None
    assert torch.equal(snap[:H * C].view(H, C), w2)
    assert torch.equal(snap[2048:2048 + C], b2)
    _same(h, ops.gemm_bias_act(x, w1, b1, act="relu", route="stripes"))


def test_graph_replay_follows_the_input():
    x, w, b = _inputs(100, 100, 784, torch.bfloat16)
    out = torch.full((100, 100), POISON, device=DEV, dtype=torch.bfloat16)
    run = lambda: ops.gemm_bias_act(x, w, b, act="relu", out=out,
                                    route="fwd1")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    g = torch.Generator().manual_seed(11)
    for _ in range(5):
        x.copy_(torch.rand(100, 784, generator=g).to(torch.bfloat16))
        out.fill_(POISON)
        graph.replay()
        got = out.clone()
        _same(got, _run("fwd1", x, w, b, "relu", torch.bfloat16))
        _same(got, _run("stripes", x, w, b, "relu", torch.bfloat16))


def test_outside_the_limits():
    # K too short to slice, and a transposed operand: forcing raises
    x, w, b = _inputs(100, 100, 128, torch.bfloat16)
    with pytest.raises(RuntimeError):
        _run("fwd1", x, w, b, "relu", torch.bfloat16)
    x, w, b = _inputs(64, 48, 512, torch.bfloat16)
    with pytest.raises(RuntimeError):
        ops.gemm_bias_act(x, w.t().contiguous(), b, trans_b=True,
                          route="fwd1")
    # larger than the auto gate: auto keeps the stripes kernels
    x, w, b = _inputs(200, 100, 784, torch.bfloat16)
    _same(_run("auto", x, w, b, "relu", torch.bfloat16),
          _run("stripes", x, w, b, "relu", torch.bfloat16))
    # the unsliced and transposed calls still run on their own kernels
    x, w, b = _inputs(100, 100, 128, torch.bfloat16)
    _same(_run("auto", x, w, b, "relu", torch.bfloat16),
          _run("stripes", x, w, b, "relu", torch.bfloat16))
