"""Shared pieces of the exact-arithmetic GEMM tests (test_gemm_exact.py,
test_gemm_exact_gpu.py, _gemm_exact_proc.py).

Method: every element of A, B and a relu_bwd mask is -1 or +1, drawn
independently from a seeded CPU generator (so a transposed or swapped
operand flips about half of the outputs it touches); the bias and the
"sub" aux are integers in [-3, 3]. Every product is +-1, so fp32
accumulation is exact in ANY order — MFMA grouping, K slices, the
four-wave split of the small kernel, stripe sums. While max|ref| <= 256
every expected value is an integer bf16 holds exactly, so kernel output
and the fp64 reference are compared with torch.equal — no tolerance.
One dropped or doubled product flips the parity of an output.

Every case carries the gemm_plan / gemm_sgd_plan it is here to cover
and asserts it first, so a retuned gate fails the assertion instead of
silently moving the shape to another kernel.
"""

import collections

import torch

LIMIT = 256          # integers up to 2^8 are exact in bf16 (8-bit mantissa)
SEED = 2718
GUARD = 64           # elements of 7 before and after every output
POISON = 7.0
PAD = 4096           # NaN elements behind every operand

ACTS = {"none": 0, "relu": 1, "relu_bwd": 2, "sub": 3}
ROUTES = {"auto": 0, "stripes": 1, "fwd1": 2}
COMBOS = {"nn": (False, False), "tn": (True, False), "nt": (False, True),
          "tt": (True, True)}

# (act, bias dtype name or None, out dtype name)
EPI_ALL = [(a, b, o) for a in ("none", "relu") for b in (None, "f32", "bf16")
           for o in ("bf16", "f32")]
EPI_TWO = [("relu", "f32", "bf16"), ("none", None, "f32")]
DT = {"f32": torch.float32, "bf16": torch.bfloat16}

Case = collections.namedtuple(
    "Case", "id combo M N K act colsum route epi plan offa offb")


def _g(id, combo, M, N, K, plan, act="none", colsum=False, route="auto",
       epi="two", off=(0, 0)):
    return Case(id, combo, M, N, K, act, colsum, route, epi, plan,
                off[0], off[1])


TILE = ("tile", 0, 1, "none")
SMALL = ("small", 0, 1, "none")


def _combos(prefix, M, N, K, plan, full=None, **kw):
    """One case per transpose combo; `full` names the one that runs all
    twelve epilogues."""
    return [_g("%s_%s_%dx%dx%d" % (prefix, cb, M, N, K), cb, M, N, K, plan,
               epi="all" if cb == full else "two", **kw)
            for cb in ("nn", "tn", "nt", "tt")]


CASES = (
    # ---------------------------------------------- tile kernel, unsplit
    # ld 17 / 65: scalar staging; K < BK: one ragged K tile
    [_g("t_nn_33x65x17", "nn", 33, 65, 17, TILE)]
    # b128 both operands; 2x2 tiles with 6-row / 8-column ragged tiles,
    # K tail of 8
    + _combos("t", 70, 72, 40, TILE, full="nn")
    # [X,K] operand at ld 42: b32 staging, last chunk guarded, 2 live k
    + [_g("t_nt_70x72x42", "nt", 70, 72, 42, TILE),
       _g("t_nn_70x72x42", "nn", 70, 72, 42, TILE)]
    # odd everything, 3 M tiles
    + _combos("t", 130, 72, 43, TILE)
    # relu_bwd is never split: 10 K tiles, tail 12, +-1 mask
    + [_g("t_nt_relubwd_70x72x300", "nt", 70, 72, 300, TILE,
          act="relu_bwd"),
       # sub stays on the tile kernel (act 3 is outside the small gate)
       _g("t_nn_sub_70x72x40", "nn", 70, 72, 40, TILE, act="sub"),
       _g("t_nn_sub_33x65x17", "nn", 33, 65, 17, TILE, act="sub"),
       # colsum: only blockIdx.y == 0 writes; ragged N tile
       _g("t_tn_cs_70x72x40", "tn", 70, 72, 40, TILE, colsum=True),
       # 17x17 = 289 tiles (33x33 32-tiles: beyond the small gate)
       _g("t_nn_1030x1030x40", "nn", 1030, 1030, 40, TILE),
       _g("t_tn_cs_1030x1030x40", "tn", 1030, 1030, 40, TILE, colsum=True)]
    # ------------------------------ split-K + the 1-element stripe reduce
    # kc 96, 4 slices, the last 12 deep
    + [_g("sk1_tn_70x72x300", "tn", 70, 72, 300,
          ("tile_sk", 96, 4, "reduce1")),
       _g("sk1_nt_70x72x300", "nt", 70, 72, 300,
          ("tile_sk", 96, 4, "reduce1")),
       _g("sk1_tt_70x72x300", "tt", 70, 72, 300,
          ("tile_sk", 96, 4, "reduce1")),
       _g("sk1_nn_stripes_70x72x300", "nn", 70, 72, 300,
          ("tile_sk", 96, 4, "reduce1"), route="stripes", epi="all"),
       # the same nn call on auto is the one-launch kernel: anchors it
       # to arithmetic too, not only to the stripes route
       _g("fwd1_nn_auto_70x72x300", "nn", 70, 72, 300,
          ("fwd1", 96, 4, "none"), epi="all"),
       # mn odd, 5 slices
       _g("sk1_nn_stripes_33x65x320", "nn", 33, 65, 320,
          ("tile_sk", 64, 5, "reduce1"), route="stripes"),
       # 16 slices
       _g("sk1_nn_stripes_64x64x2048", "nn", 64, 64, 2048,
          ("tile_sk", 128, 16, "reduce1"), route="stripes")]
    # ------------------------------ split-K + the 4-element stripe reduce
    # mn = 66560, aligned stripes: the vector path
    + [_g("sk4_nt_260x256x256", "nt", 260, 256, 256,
          ("tile_sk", 64, 4, "reduce4"))]
    # mn % 4 == 1: stripes 1 and 2 start off a 16-byte boundary
    + _combos("sk4", 257, 257, 288, ("tile_sk", 96, 3, "reduce4"),
              full="nn")
    # ------------------------------------------- split-K with the colsum
    # 8 slices with mn odd; 10 slices, the last 12 deep
    + [_g("sk4cs_tn_33x65x256", "tn", 33, 65, 256,
          ("tile_sk", 32, 8, "reduce4_cs"), colsum=True),
       _g("sk4cs_tn_64x72x300", "tn", 64, 72, 300,
          ("tile_sk", 32, 10, "reduce4_cs"), colsum=True)]
    # ------------------------------------------------------ small kernel
    # vector A and B; the last N tile's second half is guarded
    + [_g("sm_nn_200x152x104", "nn", 200, 152, 104, SMALL, epi="all"),
       _g("sm_tn_200x152x104", "tn", 200, 152, 104, SMALL),
       # scalar A and B; the four waves get 32, 32, 32, 4 of K
       _g("sm_nn_201x150x100", "nn", 201, 150, 100, SMALL),
       _g("sm_tn_cs_201x150x100", "tn", 201, 150, 100, SMALL, colsum=True),
       # K inside one wave, three waves idle
       _g("sm_nn_199x152x17", "nn", 199, 152, 17, SMALL),
       # the gate's limits: K = 256 (64 per wave), colsum
       _g("sm_tn_cs_256x128x256", "tn", 256, 128, 256, SMALL, colsum=True)]
)

# unaligned bases: the operand is a contiguous view `off` elements into
# its storage (2, 4 and 8 bytes). Every pitch here but the tn A of
# 70x72x40 is a multiple of 8, so only the base decides the level.
_UNALIGNED_BASES = [("t", "nn", 70, 72, 40, TILE), ("t", "tn", 70, 72, 40, TILE),
                    ("sm", "nn", 200, 152, 104, SMALL),
                    ("sm", "tn", 200, 152, 104, SMALL)]
UNALIGNED = [
    _g("%s_%s_%dx%dx%d_off%d_%d" % (p, cb, M, N, K, oa, ob), cb, M, N, K,
       plan, off=(oa, ob))
    for (p, cb, M, N, K, plan) in _UNALIGNED_BASES
    for off in (1, 2, 4)
    for (oa, ob) in ((off, 0), (0, off), (off, off))]

ALL = list(CASES) + UNALIGNED
BY_ID = {c.id: c for c in ALL}

# the cases _gemm_exact_proc.py runs under TFA_GEMM_LA=1: every reduce1
# case (N = 72: ldc % 4 == 0; N = 65: ldc % 4 != 0; 64x64: 16 slices)
# must then plan the last-arriver epilogue; a colsum case must not
LA_CASES = [c for c in CASES if c.plan[3] == "reduce1"]
LA_KEEP = [BY_ID["sk4cs_tn_33x65x256"]]


def la_plan(c):
    return c.plan[:3] + ("last_arriver",) if c in LA_CASES else c.plan


def proc_lines():
    """The OK lines _gemm_exact_proc.py prints, in order."""
    return ["OK %s run%d" % (c.id, r) for c in LA_CASES + LA_KEEP
            for r in (1, 2)]


def variants(c):
    """(act, bias, out) epilogues a case runs."""
    if c.act != "none":
        return [(c.act, None, "bf16")]
    if c.colsum:
        return [("none", None, "bf16"), ("none", None, "f32")]
    return EPI_ALL if c.epi == "all" else EPI_TWO


def pm1(shape, gen):
    """+-1 tensor (no zeros), float64."""
    return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).double()


def stored_shapes(combo, M, N, K):
    ta, tb = COMBOS[combo]
    return ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))


def _gen(key, table):
    return torch.Generator().manual_seed(
        SEED + [x.id for x in table].index(key))


def inputs(c, gen=None):
    """Stored a, b, the integer bias and aux (or None) — float64 CPU,
    deterministic per case."""
    if gen is None:
        gen = _gen(c.id, ALL)
    sa, sb = stored_shapes(c.combo, c.M, c.N, c.K)
    a = pm1(sa, gen)
    b = pm1(sb, gen)
    bias = torch.randint(-3, 4, (c.N,), generator=gen).double()
    aux = None
    if c.act == "relu_bwd":
        aux = pm1((c.M, c.N), gen)
    elif c.act == "sub":
        aux = torch.randint(-3, 4, (c.M, c.N), generator=gen).double()
    return a, b, bias, aux


def reference(a, b, ta, tb, bias=None, act="none", aux=None):
    """fp64 (out, colsum) of the op from the STORED operands — the oracle
    every comparison uses (test_gemm_exact.py checks it against naive
    loops)."""
    x = a.double().t() if ta else a.double()
    y = b.double().t() if tb else b.double()
    out = x @ y
    if bias is not None:
        out = out + bias.double()
    if act == "relu":
        out = out.clamp(min=0)
    elif act == "relu_bwd":
        out = out * (aux.double() > 0)
    elif act == "sub":
        out = out - aux.double()
    return out, y.sum(0)


_cache = {}


def case_refs(c):
    """Memoised (inputs, {variant: (out, colsum)}) of a case. Callers
    must not modify it."""
    if c.id not in _cache:
        a, b, bias, aux = inputs(c)
        ta, tb = COMBOS[c.combo]
        refs = {}
        for v in variants(c):
            act, bdt, _ = v
            key = (act, bdt is not None)
            if key not in refs:
                refs[key] = reference(a, b, ta, tb,
                                      bias if bdt is not None else None,
                                      act, aux)
        _cache[c.id] = ((a, b, bias, aux), refs)
    return _cache[c.id]


def ref_of(c, v):
    return case_refs(c)[1][(v[0], v[1] is not None)]


def assert_conditions(c):
    """The exactness and relu conditions — on the fp64 reference alone."""
    for v in variants(c):
        out, cs = ref_of(c, v)
        if v[2] == "bf16":
            m = out.abs().max().item()
            assert m <= LIMIT, "%s %r: max|out| = %g > %d" % (c.id, v, m, LIMIT)
            if c.colsum:
                m = cs.abs().max().item()
                assert m <= LIMIT, "%s: max|colsum| = %g" % (c.id, m)
        if v[0] == "relu":
            frac = float((out == 0).double().mean())
            assert 0.2 < frac < 0.8, "%s %r: relu clips %g" % (c.id, v, frac)


def expect_vec(ld, off):
    """vec_level of a bf16 operand `off` elements into an allocation
    that is itself at least 16-byte aligned."""
    if (2 * off) % 16 == 0 and ld % 8 == 0:
        return 8
    if (2 * off) % 4 == 0 and ld % 2 == 0:
        return 2
    return 1


# ---------------------------------------------------------- SGD cases

LR, GSCALE = 2.0 ** -4, 2.0 ** -2

SgdCase = collections.namedtuple("SgdCase", "id combo M N K plan shadow nd")

SGD_CASES = (
    # split, mn odd: stripes 1..3 start off a 16-byte boundary
    [SgdCase("sgd_%s_33x65x256" % cb, cb, 33, 65, 256, (64, 4), sh, nd)
     for cb, sh, nd in (("nn", True, 0.5), ("tn", False, 0.0),
                        ("nt", True, 0.0), ("tt", False, 0.5))]
    # split, aligned; last slice 12 deep
    + [SgdCase("sgd_nt_64x72x300_shadow", "nt", 64, 72, 300, (96, 4),
               True, 0.5),
       SgdCase("sgd_nt_64x72x300", "nt", 64, 72, 300, (96, 4), False, 0.0),
       # unsplit: temp grad + the flat SGD apply
       SgdCase("sgd_tn_70x72x40", "tn", 70, 72, 40, (0, 1), True, 0.5)]
)

PairCase = collections.namedtuple("PairCase", "id h1 h2 nd")

PAIR_CASES = [
    # first half 5 slices of 2145: the second half's workspace starts at
    # an odd element offset, its own mn % 4 == 0
    PairCase("pair_wsoff", ("nn", 33, 65, 320, (64, 5)),
             ("nt", 64, 72, 300, (96, 4)), 0.5),
    # one half unsplit
    PairCase("pair_unsplit", ("tn", 70, 72, 40, (0, 1)),
             ("nn", 33, 65, 256, (64, 4)), 0.0),
]
SHADOW_AT = 8        # each shadow sits this far into the OTHER half's A


def sgd_param(M, N, gen):
    """Multiples of 2^-6 in [-4, 4]."""
    return torch.randint(-256, 257, (M, N), generator=gen).double() / 64


def sgd_reference(a, b, ta, tb, p, nd):
    """fp64 updated param; the shadow is its bf16 rounding."""
    g, _ = reference(a, b, ta, tb)
    return p - LR * (GSCALE * g + nd * p.clamp(max=0))


def sgd_inputs(c):
    gen = _gen(c.id, SGD_CASES)
    sa, sb = stored_shapes(c.combo, c.M, c.N, c.K)
    return pm1(sa, gen), pm1(sb, gen), sgd_param(c.M, c.N, gen)


def pair_inputs(c):
    gen = _gen(c.id, PAIR_CASES)
    halves = []
    for (cb, M, N, K, _) in (c.h1, c.h2):
        sa, sb = stored_shapes(cb, M, N, K)
        halves.append((pm1(sa, gen), pm1(sb, gen), sgd_param(M, N, gen)))
    return halves


def assert_fp32_exact(t):
    """An fp64 tensor every fp32 kernel must reproduce bit for bit."""
    assert torch.equal(t.float().double(), t)


# ------------------------------------------------------------- GPU side

def padded(t, dev, dtype=torch.bfloat16, off=0):
    """t as a contiguous view `off` elements into a NaN-filled
    allocation with PAD more NaNs behind it."""
    n = t.numel()
    big = torch.full((off + n + PAD,), float("nan"), device=dev, dtype=dtype)
    assert big.data_ptr() % 16 == 0
    big[off:off + n] = t.reshape(-1).to(dev, dtype)
    v = big[off:off + n].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() - big.data_ptr() == \
        off * big.element_size()
    return v


def guarded(shape, dtype, dev):
    """(buffer of 7s, the contiguous interior view of `shape`)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), POISON, device=dev, dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(shape)


def check_guard(buf, what, cid):
    n = buf.numel() - 2 * GUARD
    assert bool((buf[:GUARD] == POISON).all()), \
        "%s: %s wrote in front of its buffer" % (cid, what)
    assert bool((buf[GUARD + n:] == POISON).all()), \
        "%s: %s wrote behind its buffer" % (cid, what)


def _eq(got, want, what, cid):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (cid, what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want) | (got != got)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(
            "%s: %s differs from the fp64 reference at %d of %d elements "
            "(first %s: got %g want %g; %d still hold the fill value)" % (
                cid, what, int(bad.sum()), bad.numel(), idx,
                got[tuple(idx)].item(), want[tuple(idx)].item(),
                int(((got == POISON) & (want != POISON)).sum())))


def check_case(ops, c, dev, plan=None):
    """One case on the HIP kernels vs the fp64 reference: plan, staging
    levels, every epilogue variant with torch.equal and guard bands."""
    ext = ops._ext()
    ta, tb = COMBOS[c.combo]
    want_plan = plan or c.plan
    got_plan = tuple(ext.gemm_plan(c.M, c.N, c.K, ta, tb, ACTS[c.act],
                                   c.colsum, ROUTES[c.route]))
    assert got_plan == want_plan, "%s: plan %r, case expects %r" % (
        c.id, got_plan, want_plan)
    assert_conditions(c)
    (a64, b64, bias64, aux64), _ = case_refs(c)
    a = padded(a64, dev, off=c.offa)
    b = padded(b64, dev, off=c.offb)
    levels = tuple(ext.gemm_vec_levels(a, b))
    want_levels = (expect_vec(a.shape[1], c.offa),
                   expect_vec(b.shape[1], c.offb))
    assert levels == want_levels, "%s: staging levels %r, expected %r" % (
        c.id, levels, want_levels)
    aux = padded(aux64, dev) if aux64 is not None else None
    for v in variants(c):
        act, bdt, odt = v
        want, want_cs = ref_of(c, v)
        bias = padded(bias64, dev, DT[bdt]) if bdt is not None else None
        obuf, out = guarded((c.M, c.N), DT[odt], dev)
        cbuf = cs = None
        if c.colsum:
            cbuf, cs = guarded((c.N,), DT[odt], dev)
        r = ops.gemm_bias_act(a, b, bias, act=act, trans_a=ta, trans_b=tb,
                              out=out, aux=aux, colsum_out=cs, route=c.route)
        assert r.data_ptr() == out.data_ptr()
        tag = "%s/%s/%s" % (act, bdt, odt)
        _eq(out, want, "out " + tag, c.id)
        check_guard(obuf, "out " + tag, c.id)
        if c.colsum:
            _eq(cs, want_cs, "colsum " + tag, c.id)
            check_guard(cbuf, "colsum " + tag, c.id)


def _sgd_buffers(p64, shadow, dev):
    pbuf, p = guarded(tuple(p64.shape), torch.float32, dev)
    p.copy_(p64.to(dev, torch.float32))
    sbuf = s = None
    if shadow:
        sbuf, s = guarded(tuple(p64.shape), torch.bfloat16, dev)
    return pbuf, p, sbuf, s


def check_sgd(ops, c, dev):
    ext = ops._ext()
    ta, tb = COMBOS[c.combo]
    got_plan = tuple(ext.gemm_sgd_plan(c.M, c.N, c.K))
    assert got_plan == c.plan, "%s: plan %r, case expects %r" % (
        c.id, got_plan, c.plan)
    a64, b64, p64 = sgd_inputs(c)
    want = sgd_reference(a64, b64, ta, tb, p64, c.nd)
    assert_fp32_exact(want)
    a, b = padded(a64, dev), padded(b64, dev)
    pbuf, p, sbuf, s = _sgd_buffers(p64, c.shadow, dev)
    ops.gemm_sgd(a, b, p, LR, shadow=s, grad_scale=GSCALE, neg_decay=c.nd,
                 trans_a=ta, trans_b=tb)
    _eq(p, want, "param", c.id)
    check_guard(pbuf, "param", c.id)
    if c.shadow:
        _eq(s, want.float().to(torch.bfloat16).double(), "shadow", c.id)
        check_guard(sbuf, "shadow", c.id)


def check_pair(ops, c, dev):
    """Both halves vs the fp64 reference computed from the PRE-update
    operands. Each half's shadow lives inside the other half's A
    operand, so a gradient GEMM that ran after the other half's apply
    would read updated, non-+-1 values."""
    ext = ops._ext()
    specs, wants, abig, shadows = [], [], [], []
    ins = pair_inputs(c)
    for (cb, M, N, K, plan), (a64, b64, p64) in zip((c.h1, c.h2), ins):
        got_plan = tuple(ext.gemm_sgd_plan(M, N, K))
        assert got_plan == plan, "%s: plan %r, case expects %r" % (
            c.id, got_plan, plan)
        ta, tb = COMBOS[cb]
        w = sgd_reference(a64, b64, ta, tb, p64, c.nd)
        assert_fp32_exact(w)
        wants.append(w)
        abig.append(padded(a64, dev))
    for i, ((cb, M, N, K, _), (a64, b64, p64)) in enumerate(
            zip((c.h1, c.h2), ins)):
        other = abig[1 - i].view(-1)
        assert SHADOW_AT + M * N <= other.numel()
        s = other[SHADOW_AT:SHADOW_AT + M * N].view(M, N)
        shadows.append(s)
        pbuf, p = guarded((M, N), torch.float32, dev)
        p.copy_(p64.to(dev, torch.float32))
        ta, tb = COMBOS[cb]
        specs.append(((abig[i], padded(b64, dev), p, s, ta, tb), pbuf))
    ops.gemm_sgd_pair(specs[0][0], specs[1][0], LR, grad_scale=GSCALE,
                      neg_decay=c.nd)
    for i in range(2):
        cid = "%s half %d" % (c.id, i + 1)
        _eq(specs[i][0][2], wants[i], "param", cid)
        check_guard(specs[i][1], "param", cid)
        sw = wants[i].float().to(torch.bfloat16).double()
        _eq(shadows[i], sw, "shadow", cid)
        # the rest of the operand the shadow sits in is untouched
        a64 = ins[1 - i][0].reshape(-1)
        rest = abig[1 - i].view(-1).cpu().double()
        n = sw.numel()
        assert torch.equal(rest[:SHADOW_AT], a64[:SHADOW_AT]), cid
        assert torch.equal(rest[SHADOW_AT + n:], a64[SHADOW_AT + n:]), cid
