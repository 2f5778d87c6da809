"""FTRL-Proximal on the GPU — SPARSE_FTRL of csrc/sparse_apply.hip and
ftrl_kernel of csrc/apply.hip, both the rule of csrc/ftrl.h — against the
CPU references of ops.sparse_ftrl / ops.fused_ftrl.

Inputs, hyper-parameters, starting state (half the rows never updated) and
tolerance are those of test_sparse_ftrl.py: dyadic gradients whose fp32
sums are exact in any order, so summation order cannot excuse a mismatch;
torch.allclose(atol=1e-5) on master, accum and linear. Bag mode takes the
dyadic bags of test_embedding_bag_gpu.py (power-of-two mean lengths and
weight sums), for the same reason."""

import functools

import pytest
import torch

from test_embedding_bag_gpu import lens_for, make_bags
from test_sparse_ftrl import (HP, INVALID, TABLE_HP, V, check_exact_threshold,
                              dyadic, exact_threshold_case, init_state)

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import EmbeddingTable, HashedEmbeddingTable

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 7.0      # initial shadow value: a written row cannot keep it


def gpu(t):
    return None if t is None else t.to(DEV)


def mixed_ids(gen, n_valid, hot=0, hot_id=5):
    """n_valid ids from [0, 60) — with ``hot`` > 0, exactly ``hot`` of them
    are hot_id and no other draw hits it — plus the four invalid ids, in
    random order."""
    ids = torch.randint(0, 59 if hot else 60, (n_valid - hot,), generator=gen)
    if hot:
        ids = ids + (ids >= hot_id).long()
        ids = torch.cat([ids, torch.full((hot,), hot_id)])
    ids = torch.cat([ids, torch.tensor(INVALID)])
    return ids[torch.randperm(ids.numel(), generator=gen)]


def step(p, ids, g, a, c, sh, gscale, bag=None):
    kw = {}
    if bag is not None:
        kw = dict(offsets=bag[0], weights=bag[1], combiner=bag[2])
    ops.sparse_ftrl(p, ids, g, a, c, bf16_out=sh, grad_scale=gscale, **HP,
                    **kw)


@functools.lru_cache(maxsize=None)
def case(D, n_valid, hot, steps, seed, mode=None):
    """Inputs and the CPU reference trajectory, computed once per case and
    shared (never modified by the tests). mode: (combiner, weighted) of a
    pooled case, whose ids come from make_bags."""
    gen = torch.Generator().manual_seed(seed)
    p, a, c = init_state(D, gen)
    sh = torch.full((V, D), SENTINEL, dtype=torch.bfloat16)
    start = (p.clone(), a.clone(), c.clone())
    pushes, refs = [], []
    for k in range(1, steps + 1):
        bag = None
        if mode is None:
            ids = mixed_ids(gen, n_valid, hot)
            g = dyadic(gen, ids.numel(), D)
        else:
            ids, offsets, weights = make_bags(gen, lens_for(*mode), *mode)
            g = dyadic(gen, offsets.numel() - 1, D)
            bag = (offsets, weights, mode[0])
        gscale = 0.5 if k % 2 else 1.0
        step(p, ids, g, a, c, sh, gscale, bag)
        pushes.append((ids, g, gscale, bag))
        refs.append((p.clone(), a.clone(), c.clone()))
    return start, pushes, refs


def check_push(k, tensors, before, refs, ids, touched):
    """After push k: allclose to the reference, idle rows bit-identical,
    shadow == bf16(master) on touched rows, sentinel elsewhere."""
    p, a, c, sh = tensors
    now = torch.zeros(V, dtype=torch.bool)
    now[ids[(ids >= 0) & (ids < V)]] = True
    touched |= now
    for name, t, ref in zip(("master", "accum", "linear"), (p, a, c), refs):
        err = (t.cpu() - ref).abs().max().item()
        print("push %d %s: max |err| %.3g" % (k, name, err))
        assert torch.allclose(t.cpu(), ref, atol=1e-5), name
    idle = (~now).to(DEV)
    for t, t0 in zip(tensors, before):
        assert torch.equal(t[idle], t0[idle])
    tt = touched.to(DEV)
    assert torch.equal(sh[tt], p[tt].to(torch.bfloat16))
    assert (sh[~tt].float() == SENTINEL).all()


def run_case(D, gdtype, n_valid, hot, steps, seed, mode=None):
    (p0, a0, c0), pushes, refs = case(D, n_valid, hot, steps, seed, mode)
    p, a, c = (t.to(DEV, copy=True) for t in (p0, a0, c0))
    sh = torch.full((V, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    touched = torch.zeros(V, dtype=torch.bool)
    for k, ((ids, g, gscale, bag), ref) in enumerate(zip(pushes, refs), 1):
        before = [t.clone() for t in (p, a, c, sh)]
        if bag is not None:
            bag = (gpu(bag[0]), gpu(bag[1]), bag[2])
        step(p, ids.to(DEV), g.to(DEV, gdtype), a, c, sh, gscale, bag)
        check_push(k, (p, a, c, sh), before, ref, ids, touched)
    assert not touched[60:].any() and touched[:60].any()
    assert (p[touched.to(DEV)] == 0).any()      # l1 at work


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("D", [7, 8, 130, 200, 320])
def test_matrix(D, gdtype):
    """300 ids from [0, 60) + 4 invalid, 5 pushes: scalar path (7), under
    one wave's vector width (8), even but no multiple of 4 (130), the NMF
    rank (200), more than one 256-column step (320)."""
    run_case(D, gdtype, 300, 0, 5, seed=D)


@pytest.mark.parametrize("hot", [512, 513, 1300])
@pytest.mark.parametrize("D", [8, 200])
def test_hot_id(D, hot):
    """One id with exactly 512 (one wave), 513 (split) and 1300 (two full
    chunks and a remainder) contributions among 200 others."""
    run_case(D, torch.bfloat16, hot + 200, hot, 2, seed=1000 + D)


@pytest.mark.parametrize("combiner,weighted", [
    ("sum", False), ("sum", True), ("mean", False), ("mean", True)])
@pytest.mark.parametrize("D", [8, 130])
def test_bag_mode(D, combiner, weighted):
    run_case(D, torch.bfloat16, 0, 0, 3, seed=2000 + D,
             mode=(combiner, weighted))


def _view_at(t, off):
    """A copy of t on the GPU that starts ``off`` elements into its
    storage (off = 1: contiguous, but not 16-byte aligned)."""
    flat = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (off == 0)
    return v


@pytest.mark.parametrize("unaligned", ["table", "grads"])
def test_unaligned_views(unaligned):
    """D % 4 == 0 but master, both states and the shadow one element into
    their storage, or only the fp32 grads: the launcher's alignment rule
    sends both to the scalar path; the result is what is asserted."""
    D = 8
    (p0, a0, c0), pushes, refs = case(D, 300, 0, 2, 11)
    toff, goff = (1, 0) if unaligned == "table" else (0, 1)
    p, a, c = (_view_at(t, toff) for t in (p0, a0, c0))
    sh = _view_at(torch.full((V, D), SENTINEL, dtype=torch.bfloat16), toff)
    touched = torch.zeros(V, dtype=torch.bool)
    for k, ((ids, g, gscale, _), ref) in enumerate(zip(pushes, refs), 1):
        before = [t.clone() for t in (p, a, c, sh)]
        step(p, ids.to(DEV), _view_at(g, goff), a, c, sh, gscale)
        check_push(k, (p, a, c, sh), before, ref, ids, touched)


@pytest.mark.parametrize("hot,D", [(0, 8), (0, 130), (600, 8)],
                         ids=["D8", "D130", "run600"])
def test_exact_thresholding(hot, D):
    """Zero master and state, l1 = 1.01: linear == G and master == 0 exactly
    where |G| <= l1, in master and shadow (test_sparse_ftrl.py), on the
    device; once with a run longer than 512 (summed through the scratch)."""
    gen = torch.Generator().manual_seed(23 + hot)
    l1 = 1.01
    ids, g, G, touched = exact_threshold_case(gen, D, 120, hot)
    p, a, c = (torch.zeros(V, D, device=DEV) for _ in range(3))
    sh = torch.zeros(V, D, dtype=torch.bfloat16, device=DEV)
    ops.sparse_ftrl(p, ids.to(DEV), g.to(DEV, torch.bfloat16), a, c, 0.1,
                    l1=l1, l2=0.01, bf16_out=sh)
    check_exact_threshold(p, c, sh, G.to(DEV), touched.to(DEV), l1)
    assert torch.equal(a, (G * G).to(DEV))


def test_bit_reproducible():
    gen = torch.Generator().manual_seed(9)
    D = 200
    p0, a0, c0 = init_state(D, gen)
    ids = mixed_ids(gen, 1500, 1300).to(DEV)
    g = torch.randn(ids.numel(), D, generator=gen).to(DEV, torch.bfloat16)
    outs = []
    for _ in range(2):
        p, a, c = (t.to(DEV, copy=True) for t in (p0, a0, c0))
        sh = torch.zeros(V, D, dtype=torch.bfloat16, device=DEV)
        step(p, ids, g, a, c, sh, 1.0)
        outs.append([p, a, c, sh])
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert not torch.equal(outs[0][0].cpu(), p0)


def test_empty_and_all_invalid_are_noops():
    gen = torch.Generator().manual_seed(6)
    D = 8
    p0, a0, c0 = init_state(D, gen)
    p, a, c = (t.to(DEV, copy=True) for t in (p0, a0, c0))
    sh = torch.full((V, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    step(p, torch.zeros(0, dtype=torch.int64, device=DEV),
         torch.zeros(0, D, device=DEV), a, c, sh, 1.0)
    step(p, torch.tensor(INVALID * 3, device=DEV),
         dyadic(gen, 12, D).to(DEV), a, c, sh, 1.0)
    torch.cuda.synchronize()
    for t, t0 in ((p, p0), (a, a0), (c, c0)):
        assert torch.equal(t.cpu(), t0)
    assert (sh.float() == SENTINEL).all()


def test_dense_parity():
    """Every row pushed once equals fused_ftrl on the flat buffers."""
    gen = torch.Generator().manual_seed(4)
    D = 200
    start = init_state(D, gen)
    p, a, c = (t.to(DEV, copy=True) for t in start)
    pd, ad, cd = (t.to(DEV, copy=True) for t in start)
    sh = torch.zeros(V, D, dtype=torch.bfloat16, device=DEV)
    shd = torch.zeros(V, D, dtype=torch.bfloat16, device=DEV)
    ids = torch.arange(V, device=DEV)
    for _ in range(2):
        g = dyadic(gen, V, D).to(DEV, torch.bfloat16)
        step(p, ids, g, a, c, sh, 0.5)
        ops.fused_ftrl(pd.view(-1), g.view(-1), ad.view(-1), cd.view(-1),
                       bf16_out=shd.view(-1), grad_scale=0.5, **HP)
    for x, y in ((p, pd), (a, ad), (c, cd)):
        assert torch.allclose(x, y, atol=1e-5)
    assert torch.equal(sh, p.to(torch.bfloat16))
    assert torch.equal(shd, pd.to(torch.bfloat16))


@pytest.mark.parametrize("with_shadow", [False, True],
                         ids=["noshadow", "shadow"])
@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
def test_fused_ftrl_matches_cpu(gdtype, with_shadow):
    """n = 1027: one block's f32x4 bulk and a 3-element scalar tail."""
    n = 1027
    gen = torch.Generator().manual_seed(13)
    p, a, c = (t.view(-1)[:n].clone() for t in init_state(16, gen))
    pg, ag, cg = (t.to(DEV, copy=True) for t in (p, a, c))
    sh = torch.zeros(n, dtype=torch.bfloat16)
    shg = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    for k in range(1, 4):
        g = dyadic(gen, n)
        gscale = 0.5 if k % 2 else 1.0
        ops.fused_ftrl(p, g, a, c, grad_scale=gscale,
                       bf16_out=sh if with_shadow else None, **HP)
        ops.fused_ftrl(pg, g.to(DEV, gdtype), ag, cg, grad_scale=gscale,
                       bf16_out=shg if with_shadow else None, **HP)
        for name, x, y in (("master", pg, p), ("accum", ag, a),
                           ("linear", cg, c)):
            print("fused step %d %s: max |err| %.3g"
                  % (k, name, (x.cpu() - y).abs().max().item()))
            assert torch.allclose(x.cpu(), y, atol=1e-5), name
    assert (pg == 0).any() and (pg != 0).any()
    if with_shadow:
        assert torch.equal(shg, pg.to(torch.bfloat16))
    else:
        assert not shg.any()


def test_table_on_gpu_matches_cpu_table():
    kw = dict(rows=V, dim=200, lr=0.1, seed=2, optimizer="ftrl_proximal",
              **TABLE_HP)
    tg = EmbeddingTable("t", device=DEV, **kw)
    tc = EmbeddingTable("t", **kw)
    assert tg.fused and sorted(tg.state) == ["accum", "linear"]
    assert all(s.device.type == "cuda" for s in tg.state.values())
    gen = torch.Generator().manual_seed(8)
    for _ in range(3):
        ids = mixed_ids(gen, 300)
        g = dyadic(gen, ids.numel(), 200).to(torch.bfloat16)
        tg.push(ids.to(DEV), g.to(DEV))
        tc.push(ids, g)
        assert torch.allclose(tg.master.cpu(), tc.master, atol=1e-5)
        good = ids[(ids >= 0) & (ids < V)].to(DEV)
        assert torch.equal(tg.pull(good), tg.master[good].to(torch.bfloat16))
    for k in tc.state:
        assert torch.allclose(tg.state[k].cpu(), tc.state[k], atol=1e-5)


def test_hashed_table_on_gpu_with_eviction_and_return():
    """GPU hashed table against the CPU hashed table by key; one key is
    removed and named again: initial row, zero state, seeded again."""
    D, cap, seed = 8, 64, 11
    kw = dict(lr=0.1, seed=seed, optimizer="ftrl_proximal", **TABLE_HP)
    tg = HashedEmbeddingTable("h", D, cap, device=DEV, **kw)
    tc = HashedEmbeddingTable("h", D, cap, **kw)
    pool = torch.tensor([7, -3, 2 ** 40 + 1, 12345, 99, 5, 2 ** 61, 41])
    gen = torch.Generator().manual_seed(8)

    def push(keys):
        g = dyadic(gen, keys.numel(), D).to(torch.bfloat16)
        tg.push(keys.to(DEV), g.to(DEV))
        tc.push(keys, g)

    def check():
        assert tg.stats()["size"] == tc.stats()["size"]
        rg = ops.hash_find(tg.index, pool.to(DEV)).cpu()
        rc = ops.hash_find(tc.index, pool)
        assert torch.equal(rg >= 0, rc >= 0)
        have = rc >= 0
        rg, rc = rg[have], rc[have]
        assert torch.allclose(tg.master.cpu()[rg], tc.master[rc], atol=1e-5)
        for k in ("accum", "linear"):
            assert torch.allclose(tg.state[k].cpu()[rg], tc.state[k][rc],
                                  atol=1e-5), k
        assert torch.equal(tg.shadow.cpu()[rg],
                           tg.master.cpu()[rg].to(torch.bfloat16))

    for _ in range(3):
        push(pool[torch.randint(0, pool.numel(), (30,), generator=gen)])
        check()
    gone = torch.tensor([12345])
    r = ops.hash_find(tg.index, gone.to(DEV))
    assert int(r) >= 0 and tg.state["accum"][r].any()
    tg.remove(gone.to(DEV))
    tc.remove(gone)
    assert int(ops.hash_find(tg.index, gone.to(DEV))) == -1
    check()
    # its first push back: a zero gradient shows the state it starts from
    zero = torch.zeros(1, D, dtype=torch.bfloat16)
    tg.push(gone.to(DEV), zero.to(DEV))
    tc.push(gone, zero)
    r = ops.hash_find(tg.index, gone.to(DEV))
    init = ops.hash_init_rows(gone, D, seed)
    assert not tg.state["accum"][r].any() and tg.state["linear"][r].all()
    assert torch.allclose(tg.master[r].cpu(), init, atol=1e-6)
    push(torch.cat([gone, pool[:3], gone]))
    check()
