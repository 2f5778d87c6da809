"""Shared pieces of the exact-arithmetic conv tests (test_conv_exact.py,
test_conv_exact_gpu.py, _conv_exact_proc.py).

Method: every element of x, w and dy is -1 or +1 and the bias is an
integer in [-3, 3], so every product is +-1 and fp32 accumulation is
exact in ANY order (split slices, atomics, MFMA grouping). While
max|ref| <= 256 every expected value is an integer bf16 holds exactly,
so kernel output and fp64 reference are compared with torch.equal — no
tolerance. One dropped or doubled product flips the parity of an
output; a wrong operand flips about half of the outputs it touches.
"""

import collections

import torch

LIMIT = 256          # integers up to 2^8 are exact in bf16 (8-bit mantissa)
SEED = 4242

Case = collections.namedtuple(
    "Case", "id N C H W K R S stride pad zf zd zw probe")


def _c(id, N, C, H, W, K, R, S, stride, pad, zf, zd, zw, probe=()):
    if isinstance(stride, int):
        stride = (stride, stride)
    if isinstance(pad, int):
        pad = (pad, pad)
    return Case(id, N, C, H, W, K, R, S, stride, pad, zf, zd, zw, probe)


# zf / zd / zw: what conv_fwd_slices / conv_bwdd_slices / conv_bwdw_slices
# must return for the shape (1 = unsplit). A retuned heuristic that
# moves a shape off the path it is here to cover fails the assertion
# instead of silently turning a split case into an unsplit one.
# probe: outputs ("y", "dx") whose size hits the stripe-reduce tail
# (M*cols % 1024 in 1..3) — see poison().
CASES = [
    # ---- forward split (KD = R*S*C >= 512, few tiles)
    # M*K = 1025: the reduce kernel's last thread owns ONE element
    _c("fsplit_mk1025", 1, 64, 5, 5, 41, 3, 3, 1, 1, 9, 1, 1, ("y",)),
    # KD = 600 -> 96-tap slices, 7 launched, ragged last slice of 24
    # (bwd-data: KD = 1000, 11 launched, last of 40)
    _c("fsplit_kd600_5x5", 2, 24, 9, 9, 40, 5, 5, 1, 2, 9, 15, 6),
    # C % 8 != 0: scalar gather + split
    _c("fsplit_c60", 1, 60, 7, 7, 24, 3, 3, 1, 1, 8, 1, 2),
    # stride 2, two N tiles (K = 72), second ragged
    _c("fsplit_s2_k72", 2, 64, 9, 9, 72, 3, 3, 2, 0, 9, 10, 1),
    _c("fsplit_kd648", 2, 72, 7, 7, 24, 3, 3, 1, 1, 10, 1, 4),
    # ---- forward unsplit
    _c("stem_c3", 2, 3, 16, 16, 8, 3, 3, 1, 1, 1, 1, 16),
    _c("s2_odd", 2, 8, 15, 15, 16, 3, 3, 2, 0, 1, 1, 4),
    _c("k1x7", 1, 4, 12, 12, 6, 1, 7, 1, (0, 3), 1, 1, 5),
    _c("k7x1", 1, 4, 12, 12, 6, 7, 1, 1, (3, 0), 1, 1, 5),
    # unequal strides and pads: bwd-data generic (STRIDE == 0) path
    _c("uneven_stride_pad", 1, 8, 9, 12, 16, 3, 3, (1, 2), (1, 0),
       1, 1, 2),
    # pointwise, P = 4608 >= 4096: GEMM route fwd and bwd-data, and a
    # 144-slice bwd-weight
    _c("pointwise_p4608", 2, 16, 48, 48, 24, 1, 1, 1, 0, 1, 1, 144),
    # ---- bwd-data split (KD = R*S*K >= 512)
    _c("dsplit_mk1025", 1, 41, 5, 5, 64, 3, 3, 1, 1, 1, 9, 1, ("dx",)),
    _c("dsplit_s2", 2, 24, 9, 9, 64, 3, 3, 2, 0, 1, 9, 1),
    _c("dsplit_s3", 1, 16, 10, 10, 64, 3, 3, 3, 1, 1, 9, 1),
    # K % 8 != 0: scalar dY path, ragged slices
    _c("dsplit_k60", 1, 24, 6, 6, 60, 3, 3, 1, 1, 1, 8, 2),
    # C = 3 weight stager; bwd-weight taps straddle (r,s), two K tiles
    _c("dsplit_c3_k72", 3, 3, 11, 11, 72, 3, 3, 1, 1, 1, 10, 12),
    # ---- bwd-data unsplit
    _c("dplain_c20", 2, 20, 7, 7, 24, 3, 3, 1, 1, 1, 1, 4),
    _c("dplain_s1", 2, 16, 13, 13, 24, 3, 3, 1, 1, 1, 1, 11),
    # ---- bwd-weight
    # Ptot = 16: one slice, plain-store epilogue
    _c("wplain_p16", 1, 16, 4, 4, 24, 3, 3, 1, 1, 1, 1, 1),
    # Ho*Wo = 4: one 32-pixel step crosses eight images; K = 41,
    # ragged Ptot = 80 over 3 slices
    _c("wwalk_8img_k41", 20, 8, 4, 4, 41, 3, 3, 2, 1, 1, 1, 3),
]
BY_ID = {c.id: c for c in CASES}

# narrow-dy cases: (channel offset, extra channels) of the concat-like
# buffer dy is a view of; the first keeps every 8-k chunk 16 B aligned,
# the other two break the row stride / the base alignment
NARROW_CASE = "dplain_s1"
NARROW = [(8, 40), (4, 12), (3, 9)]


def out_hw(c):
    return ((c.H + 2 * c.pad[0] - c.R) // c.stride[0] + 1,
            (c.W + 2 * c.pad[1] - c.S) // c.stride[1] + 1)


def launched_slices(kd, z):
    """(slices, taps in the last slice) the split fwd / bwd-data launch
    really runs for a heuristic value z: the per-slice tap count is
    rounded up to whole 32-tap tiles, which can leave fewer slices with
    a ragged last one."""
    def cdiv(a, b):
        return (a + b - 1) // b
    kc = cdiv(cdiv(kd, z), 32) * 32
    n = cdiv(kd, kc)
    return n, kd - (n - 1) * kc


def pm1(shape, gen):
    """+-1 tensor (no zeros), float64."""
    return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).double()


def inputs(c):
    """x, w (KCRS), bias, dy — float64 CPU, deterministic per case."""
    seed = SEED + CASES.index(c) if c in CASES else SEED - 1
    gen = torch.Generator().manual_seed(seed)
    Ho, Wo = out_hw(c)
    x = pm1((c.N, c.C, c.H, c.W), gen)
    w = pm1((c.K, c.C, c.R, c.S), gen)
    b = torch.randint(-3, 4, (c.K,), generator=gen).double()
    dy = pm1((c.N, c.K, Ho, Wo), gen)
    return x, w, b, dy


def narrow_buffer(c, off, pad):
    """The +-1 concat-like buffer a narrow dy is a channel slice of."""
    gen = torch.Generator().manual_seed(SEED + 1000 + off)
    Ho, Wo = out_hw(c)
    return pm1((c.N, c.K + pad, Ho, Wo), gen)


Ref = collections.namedtuple("Ref", "x w b dy y dx dw")


def compute_reference(c, x, w, b, dy):
    """fp64 y, dX, dW (KCRS) of the conv — the oracle every comparison
    uses (test_conv_exact.py checks it against naive loops)."""
    y = torch.nn.functional.conv2d(x, w, b, stride=c.stride, padding=c.pad)
    dx = torch.nn.grad.conv2d_input(x.shape, w, dy, stride=c.stride,
                                    padding=c.pad)
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=c.stride,
                                     padding=c.pad)
    return Ref(x, w, b, dy, y, dx, dw)


_cache = {}


def reference(c, narrow=None):
    """Memoised reference of a case; narrow=(off, pad) swaps dy for that
    channel slice of narrow_buffer(). Callers must not modify it."""
    key = (c.id, narrow)
    if key not in _cache:
        x, w, b, dy = inputs(c)
        if narrow is not None:
            off, pad = narrow
            dy = narrow_buffer(c, off, pad).narrow(1, off, c.K).contiguous()
        _cache[key] = compute_reference(c, x, w, b, dy)
    return _cache[key]


def assert_representable(ref):
    """The exactness condition — on the fp64 reference alone."""
    for name in ("y", "dx", "dw"):
        m = getattr(ref, name).abs().max().item()
        assert m <= LIMIT, "max|%s| = %g > %d" % (name, m, LIMIT)


# ------------------------------------------------------------- GPU side

def poison(shape, dtype, dev):
    """Fill a few just-freed blocks of an output's size with 7 so the
    caching allocator most likely hands torch::empty one of them: an
    element the kernels never write then reads 7, not a stale 0. Only
    sharpens the test; the assertion stays torch.equal."""
    blocks = [torch.full(shape, 7.0, dtype=dtype, device=dev)
              for _ in range(4)]
    del blocks


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _eq(got, want, what, cid):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (cid, what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(
            "%s: %s differs from the fp64 reference at %d of %d elements "
            "(first %s: got %g want %g)" % (
                cid, what, int(bad.sum()), bad.numel(), idx,
                got[tuple(idx)].item(), want[tuple(idx)].item()))


def check_slices(ext, c):
    Ho, Wo = out_hw(c)
    got = (ext.conv_fwd_slices(c.N, c.K, Ho, Wo, c.C, c.R, c.S),
           ext.conv_bwdd_slices(c.N, c.H, c.W, c.C, c.K, c.R, c.S),
           ext.conv_bwdw_slices(c.N, c.C, c.K, c.R, c.S, Ho, Wo))
    assert got == (c.zf, c.zd, c.zw), \
        "%s: slices (fwd, bwd-data, bwd-weight) %r, case expects %r" % (
            c.id, got, (c.zf, c.zd, c.zw))


def check_case(ops, c, dev, weight_format="kcrs"):
    """Forward (with bias), bwd-data and bwd-weight of one case on the
    HIP kernels vs the fp64 reference, all torch.equal.

    kcrs: dW comes back through autograd as bf16 w.grad.
    krsc: dW is accumulated into a pre-zeroed fp32 dw_out buffer (the
    grad-arena path) and w.grad stays None."""
    bf = torch.bfloat16
    ref = reference(c)
    assert_representable(ref)
    check_slices(ops._ext(), c)
    krsc = weight_format == "krsc"
    x = _cl(ref.x.to(dev, bf)).requires_grad_(True)
    wl = ref.w.permute(0, 2, 3, 1).contiguous() if krsc else ref.w
    w = wl.to(dev, bf).requires_grad_(True)
    b = ref.b.to(dev, torch.float32)
    dy = _cl(ref.dy.to(dev, bf))
    dw_out = torch.zeros(c.K, c.R, c.S, c.C, device=dev) if krsc else None

    if "y" in c.probe:
        assert ref.y.flatten()[-1] != 0
        poison(tuple(ref.y.shape), bf, dev)
    y = ops.conv2d(x, w, b, stride=c.stride, padding=c.pad,
                   weight_format=weight_format, dw_out=dw_out)
    _eq(y, ref.y, "y", c.id)

    if "dx" in c.probe:
        assert ref.dx.flatten()[-1] != 0
        poison(tuple(ref.dx.shape), bf, dev)
    y.backward(dy)
    _eq(x.grad, ref.dx, "dX", c.id)
    if krsc:
        assert w.grad is None, "%s: dw_out path must leave w.grad None" % c.id
        _eq(dw_out, ref.dw.permute(0, 2, 3, 1), "dW (fp32 dw_out)", c.id)
    else:
        assert w.grad.dtype == bf
        _eq(w.grad, ref.dw, "dW (bf16 w.grad)", c.id)


def check_narrow(ops, off, pad, dev):
    """bwd-data and bwd-weight (dw_out) reading dy IN PLACE as a
    channel-narrow view — called on the bindings directly so no layer
    in between can hand the kernels a contiguous copy."""
    bf = torch.bfloat16
    c = BY_ID[NARROW_CASE]
    ref = reference(c, (off, pad))
    assert_representable(ref)
    ext = ops._ext()
    big = _cl(narrow_buffer(c, off, pad).to(dev, bf))
    dy = big.narrow(1, off, c.K)
    assert dy.stride(3) == c.K + pad and dy.stride(1) == 1
    assert (dy.data_ptr() - big.data_ptr()) == 2 * off
    x = _cl(ref.x.to(dev, bf))
    wk = ref.w.permute(0, 2, 3, 1).contiguous().to(dev, bf)
    (sh, sw), (ph, pw) = c.stride, c.pad
    cid = "narrow(off=%d,pad=%d)" % (off, pad)
    dx = ext.conv2d_bwd_data(dy, wk, c.H, c.W, sh, sw, ph, pw)
    _eq(dx, ref.dx, "dX", cid)
    dw_out = torch.zeros(c.K, c.R, c.S, c.C, device=dev)
    ext.conv2d_bwd_weight_out(dy, x, c.R, c.S, sh, sw, ph, pw, dw_out)
    _eq(dw_out, ref.dw.permute(0, 2, 3, 1), "dW (fp32 dw_out)", cid)


def proc_lines():
    """The OK lines _conv_exact_proc.py prints, in order."""
    return (["OK kcrs %s" % c.id for c in CASES] +
            ["OK krsc %s" % c.id for c in CASES] +
            ["OK narrow %d %d" % n for n in NARROW])
