"""Pooled (bag) embedding pull and push on the GPU — csrc/embedding_bag.hip
and the bag mode of csrc/sparse_apply.hip — against the CPU references of
ops.embedding_bag and the pooled ops.sparse_*.

Inputs follow the dyadic recipe of test_sparse_apply_gpu.py: table values
and bag gradients randint(-32, 33)/16 (exact in bf16), weights from
{0.5, 1, 2}, grad_scale 0.5 or 1; ``mean`` bags have power-of-two lengths
(unweighted) or power-of-two weight sums <= 256 (halves only up to 128),
so every coefficient is a dyadic <= 4 on a 1/256 grid. With at most 1300
contributions per row every partial sum stays below 2**24 grid steps, the
fp32 sums are exact in any order (fused multiply-add or not) and the CPU
reference is the exact answer: forward compares torch.equal; master and
state compare allclose(atol=1e-5), the tolerance the dense and sparse
apply tests use for the same per-element formulas."""

import functools

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import EmbeddingTable

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V = 97
INVALID = [-1, -5, V, V + 3]
N_STATE = {"sgd": 0, "sgd_mom": 1, "adagrad": 1, "adam": 2}
SENTINEL = 7.0      # initial shadow value: a written row cannot keep it
DIMS = [7, 8, 130, 200, 320]
# 0 / 1 / the 64-position window edges, then short bags
SUM_LENS = [0, 1, 63, 64, 65, 130, 0, 2] + [3, 5, 2, 7, 1, 4, 6, 0] * 4
POW2_LENS = [0, 1, 64, 128, 0, 2] + [1, 2, 4, 8, 4, 2, 8, 1, 0] * 4
MODES = [("sum", False), ("mean", True), ("sum", True), ("mean", False)]


def dyadic(gen, *shape):
    return torch.randint(-32, 33, shape, generator=gen).float() / 16


def pow2_weights(gen, length):
    """``length`` weights from {0.5, 1, 2} whose sum is the next power of
    two >= length (<= 256 here); halves only when that sum is <= 128."""
    total = 1
    while total < length:
        total *= 2
    w = torch.ones(length)
    w[:total - length] = 2.0            # total - length < length
    ones = length - (total - length)
    if total <= 128 and ones >= 3:      # 1 + 1 + 1 == 0.5 + 0.5 + 2
        w[length - 3:] = torch.tensor([0.5, 0.5, 2.0])
    return w[torch.randperm(length, generator=gen)]


def make_bags(gen, lens, combiner, weighted, hot=0, hot_id=5, long_bag=False):
    """CSR bags of the given lengths over ids from [0, 60), the four
    invalid ids dropped into random positions, one bag holding the same id
    twice. hot > 0: no random draw hits hot_id, and hot_id is added exactly
    ``hot`` times — as one extra long bag (long_bag) or as ``hot`` extra
    bags of one id each — so it is no dyadic ``mean`` case."""
    lens = list(lens)
    n = sum(lens)
    ids = torch.randint(0, 59 if hot else 60, (n,), generator=gen)
    if hot:
        ids = ids + (ids >= hot_id).long()
    spots = torch.randperm(n, generator=gen)[:len(INVALID)]
    ids[spots] = torch.tensor(INVALID)
    start = 0
    for ln in lens:                      # the first bag of >= 3: id twice
        if ln >= 3:
            ids[start + 2] = ids[start]
            break
        start += ln
    if hot:
        extra = [hot] if long_bag else [1] * hot
        at = len(lens) // 2             # hot bags sit among the others
        cut = sum(lens[:at])
        ids = torch.cat([ids[:cut], torch.full((hot,), hot_id), ids[cut:]])
        lens = lens[:at] + extra + lens[at:]
    offsets = torch.tensor([0] + lens).cumsum(0)
    weights = None
    if weighted and combiner == "mean":
        weights = torch.cat([pow2_weights(gen, ln) for ln in lens]
                            + [torch.zeros(0)])
    elif weighted:
        weights = torch.tensor([0.5, 1.0, 2.0])[
            torch.randint(0, 3, (int(offsets[-1]),), generator=gen)]
    return ids, offsets, weights


def lens_for(combiner, weighted):
    return POW2_LENS if combiner == "mean" and not weighted else SUM_LENS


def gpu(t):
    return None if t is None else t.to(DEV)


# ------------------------------------------------------------------ forward

@functools.lru_cache(maxsize=None)
def fwd_case(D, combiner, weighted):
    gen = torch.Generator().manual_seed(100 + D)
    table = dyadic(gen, V, D)
    ids, offsets, weights = make_bags(gen, lens_for(combiner, weighted),
                                      combiner, weighted)
    ref = ops.embedding_bag(table, ids, offsets, weights, combiner)
    return table, ids, offsets, weights, ref


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
@pytest.mark.parametrize("tdtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("D", DIMS)
def test_forward_matrix(D, tdtype, combiner, weighted):
    """Scalar path (7), under one wave's vector width (8), even but not a
    multiple of 4 (130), the NMF rank (200), more than one 256-column tile
    (320); bags of 0, 1, 63, 64, 65, 130 ids (sum) or power-of-two
    lengths / weight sums (mean), a repeated id, the four invalid ids."""
    table, ids, offsets, weights, ref = fwd_case(D, combiner, weighted)
    lens = offsets[1:] - offsets[:-1]
    assert ref.abs().max() > 0 and (lens == 0).any()
    t = table.to(DEV, tdtype)
    args = (gpu(ids), gpu(offsets), gpu(weights), combiner)
    out = ops.embedding_bag(t, *args)
    assert out.dtype == tdtype and out.shape == (lens.numel(), D)
    assert torch.equal(out.cpu(), ref.to(tdtype))
    if tdtype == torch.bfloat16:
        out32 = ops.embedding_bag(t, *args, out_dtype=torch.float32)
        assert out32.dtype == torch.float32
        assert torch.equal(out32.cpu(), ref)
        out = out32
    assert (out[(lens == 0).to(DEV)] == 0).all()    # empty bags: exact zeros


def test_forward_unaligned_table_view_takes_scalar_path():
    """D % 4 == 0 but the table starts 4 bytes into its storage: a vector
    access would be misaligned."""
    table, ids, offsets, weights, ref = fwd_case(8, "sum", True)
    flat = torch.zeros(V * 8 + 1, device=DEV)
    t = flat[1:].view(V, 8)
    t.copy_(table)
    out = ops.embedding_bag(t, gpu(ids), gpu(offsets), gpu(weights), "sum")
    assert torch.equal(out.cpu(), ref)


# ------------------------------------------------------------- pooled apply

def step(opt, p, ids, g, st, k, sh, gscale, **bag):
    if opt == "sgd":
        ops.sparse_sgd(p, ids, g, 0.1, bf16_out=sh, grad_scale=gscale, **bag)
    elif opt == "sgd_mom":
        ops.sparse_sgd(p, ids, g, 0.1, momentum=0.9, momentum_buf=st[0],
                       bf16_out=sh, grad_scale=gscale, **bag)
    elif opt == "adagrad":
        ops.sparse_adagrad(p, ids, g, st[0], 0.1, bf16_out=sh,
                           grad_scale=gscale, **bag)
    else:
        ops.sparse_adam(p, ids, g, st[0], st[1], k, 0.01, bf16_out=sh,
                        grad_scale=gscale, **bag)


def init_state(opt, D, gen):
    p = torch.rand(V, D, generator=gen)
    st = [torch.rand(V, D, generator=gen) * 0.5 for _ in range(N_STATE[opt])]
    return p, st


@functools.lru_cache(maxsize=None)
def case(opt, D, steps, seed, hot=0, long_bag=False):
    """Pushes and the CPU reference trajectory, computed once per case and
    shared (never modified by the tests). Step k uses another (combiner,
    weighted) mode; hot-id cases are weighted sums."""
    gen = torch.Generator().manual_seed(seed)
    p, st = init_state(opt, D, gen)
    sh = torch.full((V, D), SENTINEL, dtype=torch.bfloat16)
    p0, st0 = p.clone(), [s.clone() for s in st]
    pushes, refs = [], []
    for k in range(1, steps + 1):
        combiner, weighted = ("sum", True) if hot else \
            MODES[(k + DIMS.index(D)) % 4]
        ids, offsets, weights = make_bags(
            gen, lens_for(combiner, weighted)[4:] if hot
            else lens_for(combiner, weighted), combiner, weighted, hot=hot,
            long_bag=long_bag)
        g = dyadic(gen, offsets.numel() - 1, D)
        gscale = 0.5 if k % 2 else 1.0
        bag = dict(offsets=offsets, weights=weights, combiner=combiner)
        step(opt, p, ids, g, st, k, sh, gscale, **bag)
        pushes.append((ids, g, gscale, bag))
        refs.append((p.clone(), [s.clone() for s in st]))
    return p0, st0, pushes, refs


def gpu_bag(bag):
    return dict(offsets=gpu(bag["offsets"]), weights=gpu(bag["weights"]),
                combiner=bag["combiner"])


def run_case(opt, D, gdtype, steps, seed, hot=0, long_bag=False):
    p0, st0, pushes, refs = case(opt, D, steps, seed, hot, long_bag)
    p = p0.to(DEV, copy=True)
    st = [s.to(DEV, copy=True) for s in st0]
    sh = torch.full((V, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    touched = torch.zeros(V, dtype=torch.bool)
    for k, ((ids, g, gscale, bag), (p_ref, st_ref)) in enumerate(
            zip(pushes, refs), 1):
        before = [p.clone(), sh.clone()] + [s.clone() for s in st]
        step(opt, p, ids.to(DEV), g.to(DEV, gdtype), st, k, sh, gscale,
             **gpu_bag(bag))
        now = torch.zeros(V, dtype=torch.bool)
        now[ids[(ids >= 0) & (ids < V)]] = True
        touched |= now
        err = (p.cpu() - p_ref).abs().max().item()
        print("%s D=%d step %d (%s%s): max |master err| %.3g"
              % (opt, D, k, bag["combiner"],
                 "" if bag["weights"] is None else ", weighted", err))
        assert torch.allclose(p.cpu(), p_ref, atol=1e-5)
        for s, s_ref in zip(st, st_ref):
            assert torch.allclose(s.cpu(), s_ref, atol=1e-5)
        # rows this push did not touch: bit-identical, every tensor
        idle = (~now).to(DEV)
        for t, t0 in zip([p, sh] + st, before):
            assert torch.equal(t[idle], t0[idle])
        # shadow == bf16(master) exactly on every row touched so far
        tt = touched.to(DEV)
        assert torch.equal(sh[tt], p[tt].to(torch.bfloat16))
        assert (sh[~tt].float() == SENTINEL).all()
    assert not touched[60:].any() and touched[:60].any()


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("opt", ["sgd", "sgd_mom", "adagrad", "adam"])
def test_apply_matrix(opt, D, gdtype):
    """3 pooled pushes of ~45 bags / a few hundred ids + 4 invalid; the
    (combiner, weighted) mode changes with the step."""
    run_case(opt, D, gdtype, 3, seed=D)


@pytest.mark.parametrize("long_bag", [False, True], ids=["spread", "one_bag"])
@pytest.mark.parametrize("hot", [1300, 512, 513])
@pytest.mark.parametrize("D", [8, 200])
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
def test_hot_id(opt, D, hot, long_bag):
    """One id contributing exactly 512 / 513 / 1300 times (the chunk
    boundary in bag mode: 512 stays one wave, 513 is split, 1300 is two
    full chunks and a remainder), spread over as many one-id bags or
    repeated inside one long bag; weighted sum."""
    run_case(opt, D, torch.bfloat16, 2, seed=1000 + D, hot=hot,
             long_bag=long_bag)


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("opt", ["sgd", "sgd_mom", "adagrad", "adam"])
def test_pooled_equals_row_path_on_expanded_rows(opt, gdtype):
    """The pooled push and an ordinary sparse_* call fed the expanded
    per-position rows c_i * g[bag_of[i]] end bit-identical. The rows are
    exact in fp32 on these inputs (a 1/256-grid c times a 1/16-grid g
    needs at most 17 bits) but not in bf16, so they are passed as fp32."""
    D = 200
    p0, st0, pushes, _ = case(opt, D, 3, seed=D)
    outs = []
    for pooled in (True, False):
        p = p0.to(DEV, copy=True)
        st = [s.to(DEV, copy=True) for s in st0]
        sh = torch.full((V, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
        for k, (ids, g, gscale, bag) in enumerate(pushes, 1):
            if pooled:
                step(opt, p, ids.to(DEV), g.to(DEV, gdtype), st, k, sh,
                     gscale, **gpu_bag(bag))
            else:
                bag_of, c = ops._bag_expand_cpu(ids, bag["offsets"],
                                                bag["weights"],
                                                bag["combiner"])
                rows = c[:, None] * g[bag_of]
                step(opt, p, ids.to(DEV), rows.to(DEV), st, k, sh, gscale)
        outs.append([p, sh] + st)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][0].cpu(), p0)


# ------------------------------------------------------ general-length mean

@functools.lru_cache(maxsize=None)
def odd_mean_case():
    """40 unweighted bags of 3, 5, 7 ids; ids cycle through [0, 60), so a
    row gets at most 4 contributions. Table values are POSITIVE dyadics
    (randint(1, 33)/16): without cancellation a bag mean is at least 1/16
    and a relative bound on the bf16 output means something."""
    gen = torch.Generator().manual_seed(77)
    D = 200
    lens = [3, 5, 7, 5] * 10
    ids = torch.arange(sum(lens)) % 60
    offsets = torch.tensor([0] + lens).cumsum(0)
    table = torch.randint(1, 33, (V, D), generator=gen).float() / 16
    g = dyadic(gen, len(lens), D)
    fwd = ops.embedding_bag(table, ids, offsets, combiner="mean")
    p = table.clone()
    ops.sparse_sgd(p, ids, g, 0.1, offsets=offsets, combiner="mean")
    return table, ids, offsets, g, fwd, p


def test_general_length_mean():
    """c = 1/3, 1/5, 1/7 are not dyadic. Push (sgd lr 0.1, fp32 bag
    gradients): each product c*g errs by at most 2**-24 * 2, a row's sum
    of <= 10 by under 1e-6, so the master errs by under 1e-6 — inside
    atol=1e-5. Forward: one bf16 ulp (rtol 2**-7) on bf16 output against
    the fp32 reference, atol=1e-5 on fp32 output."""
    table, ids, offsets, g, fwd, p_ref = odd_mean_case()
    i, o = ids.to(DEV), offsets.to(DEV)
    p = table.to(DEV, copy=True)
    ops.sparse_sgd(p, i, g.to(DEV), 0.1, offsets=o, combiner="mean")
    print("push: max |master err| %.3g" % (p.cpu() - p_ref).abs().max())
    assert torch.allclose(p.cpu(), p_ref, rtol=0, atol=1e-5)
    assert not torch.equal(p.cpu(), table)
    out32 = ops.embedding_bag(table.to(DEV), i, o, combiner="mean")
    print("fwd fp32: max |err| %.3g" % (out32.cpu() - fwd).abs().max())
    assert torch.allclose(out32.cpu(), fwd, rtol=0, atol=1e-5)
    out16 = ops.embedding_bag(table.to(DEV, torch.bfloat16), i, o,
                              combiner="mean")
    rel = ((out16.cpu().float() - fwd).abs() / fwd.abs()).max()
    print("fwd bf16: max rel err %.3g" % rel)
    assert torch.allclose(out16.cpu().float(), fwd, rtol=2 ** -7, atol=0)


# -------------------------------------------------------------- other cases

def test_bit_reproducible():
    gen = torch.Generator().manual_seed(9)
    D = 200
    p0, st0 = init_state("adam", D, gen)
    ids, offsets, weights = make_bags(gen, SUM_LENS, "mean", True, hot=1300)
    weights = torch.rand(ids.numel(), generator=gen) + 0.5
    ids, offsets, weights = gpu(ids), gpu(offsets), gpu(weights)
    g = torch.randn(offsets.numel() - 1, D, generator=gen).to(
        DEV, torch.bfloat16)
    table = torch.randn(V, D, generator=gen).to(DEV, torch.bfloat16)
    outs = []
    for _ in range(2):
        p = p0.to(DEV, copy=True)
        st = [s.to(DEV, copy=True) for s in st0]
        sh = torch.zeros(V, D, dtype=torch.bfloat16, device=DEV)
        step("adam", p, ids, g, st, 1, sh, 1.0, offsets=offsets,
             weights=weights, combiner="mean")
        fwd = ops.embedding_bag(table, ids, offsets, weights, "mean")
        outs.append([p, sh, fwd] + st)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][0].cpu(), p0)


@pytest.mark.parametrize("opt", ["sgd", "sgd_mom", "adagrad", "adam"])
def test_empty_and_all_invalid_are_noops(opt):
    """B == 0; n == 0 under non-empty all-zero offsets; all ids invalid."""
    gen = torch.Generator().manual_seed(6)
    D = 8
    p0, st0 = init_state(opt, D, gen)
    p = p0.to(DEV, copy=True)
    st = [s.to(DEV, copy=True) for s in st0]
    sh = torch.full((V, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    bad = torch.tensor(INVALID * 3, device=DEV)
    requests = [
        (none, torch.zeros(1, dtype=torch.int64, device=DEV)),
        (none, torch.zeros(5, dtype=torch.int64, device=DEV)),
        (bad, torch.tensor([0, 0, 5, 12], device=DEV)),
    ]
    for ids, offsets in requests:
        B = offsets.numel() - 1
        for combiner in ("sum", "mean"):
            step(opt, p, ids, dyadic(gen, B, D).to(DEV), st, 1, sh, 1.0,
                 offsets=offsets, combiner=combiner)
            out = ops.embedding_bag(sh, ids, offsets, combiner=combiner)
            assert out.shape == (B, D) and out.dtype == torch.bfloat16
            assert (out == 0).all()
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), p0)
    for s, s0 in zip(st, st0):
        assert torch.equal(s.cpu(), s0)
    assert (sh.float() == SENTINEL).all()


@pytest.mark.parametrize("optimizer,hp", [
    ("adagrad", {}), ("sgd", {"fused_apply": False})],
    ids=["adagrad", "sgd_unfused"])
def test_table_on_gpu_matches_cpu_table(optimizer, hp):
    kw = dict(rows=V, dim=200, lr=0.1, seed=2, optimizer=optimizer, **hp)
    tg = EmbeddingTable("t", device=DEV, **kw)
    tc = EmbeddingTable("t", **kw)
    assert tg.fused == (optimizer != "sgd")
    gen = torch.Generator().manual_seed(8)
    for k in range(2):
        combiner, weighted = MODES[k + 1]
        ids, offsets, weights = make_bags(gen, SUM_LENS, combiner, weighted)
        g = dyadic(gen, offsets.numel() - 1, 200).to(torch.bfloat16)
        tg.push_pooled(gpu(ids), gpu(offsets), g.to(DEV), gpu(weights),
                       combiner)
        tc.push_pooled(ids, offsets, g, weights, combiner)
        assert tg.step == tc.step == k + 1
        assert torch.allclose(tg.master.cpu(), tc.master, atol=1e-5)
        assert not torch.equal(tc.master, EmbeddingTable("t", **kw).master)
        pulled = tg.pull_pooled(gpu(ids), gpu(offsets), gpu(weights),
                                combiner)
        assert pulled.dtype == torch.bfloat16
        assert torch.equal(pulled, ops.embedding_bag(
            tg.shadow, gpu(ids), gpu(offsets), gpu(weights), combiner))
        assert torch.equal(tg.shadow, tg.master.to(torch.bfloat16))
    for k in tc.state:
        assert torch.allclose(tg.state[k].cpu(), tc.state[k], atol=1e-5)
