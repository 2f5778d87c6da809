"""Fused sparse optimizer apply kernels (csrc/sparse_apply.hip) against
the CPU reference of ops.sparse_*.

Inputs follow the dyadic recipe — grads randint(-32, 33)/16 (exact in
bf16; fp32 sums exact in any order), grad_scale 0.5 or 1 — so summation
order cannot excuse a mismatch. The tolerance is the one the dense apply
kernels are held to in test_kernels_gpu.py: torch.allclose(atol=1e-5) on
fp32 master and state (same per-element formulas)."""

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


def dyadic(gen, *shape):
    return torch.randint(-32, 33, shape, generator=gen).float() / 16


def step(opt, p, ids, g, st, k, sh, gscale):
    if opt == "sgd":
        ops.sparse_sgd(p, ids, g, 0.1, bf16_out=sh, grad_scale=gscale)
    elif opt == "sgd_mom":
        ops.sparse_sgd(p, ids, g, 0.1, momentum=0.9, momentum_buf=st[0],
                       bf16_out=sh, grad_scale=gscale)
    elif opt == "adagrad":
        ops.sparse_adagrad(p, ids, g, st[0], 0.1, bf16_out=sh,
                           grad_scale=gscale)
    else:
        ops.sparse_adam(p, ids, g, st[0], st[1], k, 0.01, bf16_out=sh,
                        grad_scale=gscale)


def dense_step(opt, p, g, st, k, sh, gscale):
    if opt == "sgd":
        ops.fused_sgd(p, g, 0.1, bf16_out=sh, grad_scale=gscale)
    elif opt == "sgd_mom":
        ops.fused_sgd(p, g, 0.1, momentum=0.9, momentum_buf=st[0],
                      bf16_out=sh, grad_scale=gscale)
    elif opt == "adagrad":
        ops.fused_adagrad(p, g, st[0], 0.1, bf16_out=sh, grad_scale=gscale)
    else:
        ops.fused_adam(p, g, st[0], st[1], k, 0.01, bf16_out=sh,
                       grad_scale=gscale)


def init_state(opt, D, gen):
    p = torch.rand(V, D, generator=gen)
    st = [torch.rand(V, D, generator=gen) * 0.5 for _ in range(N_STATE[opt])]
    return p, st


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


@functools.lru_cache(maxsize=None)
def case(opt, D, n_valid, hot, steps, seed):
    """Inputs and the CPU reference trajectory, computed once per case
    and shared (never modified by the tests)."""
    gen = torch.Generator().manual_seed(seed)
    p, st = init_state(opt, D, gen)
    sh = torch.full((V, D), SENTINEL, dtype=torch.bfloat16)
    p0, st0 = p.clone(), [s.clone() for s in st]
    pushes, refs = [], []
    for k in range(1, steps + 1):
        ids = mixed_ids(gen, n_valid, hot)
        g = dyadic(gen, ids.numel(), D)
        gscale = 0.5 if k % 2 else 1.0
        step(opt, p, ids, g, st, k, sh, gscale)
        pushes.append((ids, g, gscale))
        refs.append((p.clone(), [s.clone() for s in st]))
    return p0, st0, pushes, refs


def run_case(opt, D, gdtype, n_valid, hot, steps, seed):
    p0, st0, pushes, refs = case(opt, D, n_valid, hot, steps, seed)
    p = p0.to(DEV, copy=True)
    st = [s.to(DEV, copy=True) for s in st0]
    sh = torch.full((V, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    touched = torch.zeros(V, dtype=torch.bool)
    for k, ((ids, g, gscale), (p_ref, st_ref)) in enumerate(
            zip(pushes, refs), 1):
        before = [p.clone(), sh.clone()] + [s.clone() for s in st]
        step(opt, p, ids.to(DEV), g.to(DEV, gdtype), st, k, sh, gscale)
        now = torch.zeros(V, dtype=torch.bool)
        now[ids[(ids >= 0) & (ids < V)]] = True
        touched |= now
        err = (p.cpu() - p_ref).abs().max().item()
        print("%s D=%d step %d: max |master err| %.3g" % (opt, D, k, err))
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
@pytest.mark.parametrize("D", [7, 8, 130, 200, 320])
@pytest.mark.parametrize("opt", ["sgd", "sgd_mom", "adagrad", "adam"])
def test_matrix(opt, D, gdtype):
    """n=300 ids from [0,60) + 4 invalid: scalar path (7), under one
    wave's vector width (8), even but not a multiple of 4 (130), the NMF
    rank (200), more than one 256-column tile (320); 3 steps each."""
    run_case(opt, D, gdtype, 300, 0, 3, seed=D)


@pytest.mark.parametrize("hot", [1300, 512, 513])
@pytest.mark.parametrize("D", [8, 200])
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
def test_hot_id(opt, D, hot):
    """One id repeated 1300 times among 200 others (two full 512-chunks
    plus a remainder), and runs of exactly 512 / 513 contributions (the
    chunk boundary: 512 stays one wave, 513 is split)."""
    run_case(opt, D, torch.bfloat16, hot + 200, hot, 2, seed=1000 + D)


def test_hot_id_scalar_path_fp32():
    run_case("adam", 7, torch.float32, 1500, 1300, 1, seed=3)


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
    """D % 4 == 0 but a base that is not 16-byte aligned: master, both Adam
    moments and the shadow as views one element into their storage (fp32
    grads aligned), or only the grads view misaligned. The launcher's
    alignment rule sends both to the scalar path; what is asserted here is
    the result, against the CPU reference as in run_case (which path ran
    is not visible from Python)."""
    Vs, D, opt = 64, 8, "adam"
    gen = torch.Generator().manual_seed(11)
    p_ref = torch.rand(Vs, D, generator=gen)
    st_ref = [torch.rand(Vs, D, generator=gen) * 0.5 for _ in range(2)]
    sh_ref = torch.full((Vs, D), SENTINEL, dtype=torch.bfloat16)
    toff, goff = (1, 0) if unaligned == "table" else (0, 1)
    p = _view_at(p_ref, toff)
    st = [_view_at(s, toff) for s in st_ref]
    sh = _view_at(sh_ref, toff)
    touched = torch.zeros(Vs, dtype=torch.bool)
    for k in (1, 2):
        ids = mixed_ids(gen, 300)       # its invalid ids are invalid here too
        g = dyadic(gen, ids.numel(), D)
        gscale = 0.5 if k % 2 else 1.0
        step(opt, p_ref, ids, g, st_ref, k, sh_ref, gscale)
        before = [p.clone(), sh.clone()] + [s.clone() for s in st]
        step(opt, p, ids.to(DEV), _view_at(g, goff), st, k, sh, gscale)
        now = torch.zeros(Vs, dtype=torch.bool)
        now[ids[(ids >= 0) & (ids < Vs)]] = True
        touched |= now
        print("unaligned %s step %d: max |master err| %.3g"
              % (unaligned, k, (p.cpu() - p_ref).abs().max().item()))
        assert torch.allclose(p.cpu(), p_ref, atol=1e-5)
        for s, s_ref in zip(st, st_ref):
            assert torch.allclose(s.cpu(), s_ref, atol=1e-5)
        idle = (~now).to(DEV)
        for t, t0 in zip([p, sh] + st, before):
            assert torch.equal(t[idle], t0[idle])
        tt = touched.to(DEV)
        assert torch.equal(sh[tt], p[tt].to(torch.bfloat16))
        assert (sh[~tt].float() == SENTINEL).all()
    assert not touched[60:].any() and touched[:60].any()


def test_bit_reproducible():
    gen = torch.Generator().manual_seed(9)
    D = 200
    p0, st0 = init_state("adam", D, gen)
    ids = mixed_ids(gen, 1500, 1300).to(DEV)
    g = torch.randn(ids.numel(), D, generator=gen).to(DEV, torch.bfloat16)
    outs = []
    for _ in range(2):
        p = p0.to(DEV, copy=True)
        st = [s.to(DEV, copy=True) for s in st0]
        sh = torch.zeros(V, D, dtype=torch.bfloat16, device=DEV)
        step("adam", p, ids, g, st, 1, sh, 1.0)
        outs.append([p, sh] + st)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][0].cpu(), p0)


@pytest.mark.parametrize("opt", ["sgd", "sgd_mom", "adagrad", "adam"])
def test_dense_parity(opt):
    gen = torch.Generator().manual_seed(4)
    D = 200
    p0, st0 = init_state(opt, D, gen)
    ids = torch.arange(V, device=DEV)
    p, pd = p0.to(DEV, copy=True), p0.to(DEV, copy=True)
    st = [s.to(DEV, copy=True) for s in st0]
    std = [s.to(DEV, copy=True) for s in st0]
    sh = torch.zeros(V, D, dtype=torch.bfloat16, device=DEV)
    shd = torch.zeros(V, D, dtype=torch.bfloat16, device=DEV)
    for k in (1, 2):
        g = dyadic(gen, V, D).to(DEV, torch.bfloat16)
        step(opt, p, ids, g, st, k, sh, 0.5)
        dense_step(opt, pd.view(-1), g.view(-1), [s.view(-1) for s in std],
                   k, shd.view(-1), 0.5)
    assert torch.allclose(p, pd, atol=1e-5)
    for s, sd in zip(st, std):
        assert torch.allclose(s, sd, atol=1e-5)
    assert torch.equal(sh, p.to(torch.bfloat16))


@pytest.mark.parametrize("opt", ["sgd", "sgd_mom", "adagrad", "adam"])
def test_empty_and_all_invalid_are_noops(opt):
    gen = torch.Generator().manual_seed(6)
    D = 8
    p0, st0 = init_state(opt, D, gen)
    p = p0.to(DEV, copy=True)
    st = [s.to(DEV, copy=True) for s in st0]
    sh = torch.full((V, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    step(opt, p, torch.zeros(0, dtype=torch.int64, device=DEV),
         torch.zeros(0, D, device=DEV), st, 1, sh, 1.0)
    step(opt, p, torch.tensor(INVALID * 3, device=DEV),
         dyadic(gen, 12, D).to(DEV), st, 1, sh, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), p0)
    for s, s0 in zip(st, st0):
        assert torch.equal(s.cpu(), s0)
    assert (sh.float() == SENTINEL).all()


@pytest.mark.parametrize("optimizer,hp", [
    ("adagrad", {}), ("sgd", {"fused_apply": True}),
    ("adagrad", {"weight_decay": 0.01})],
    ids=["adagrad", "sgd_fused", "adagrad_wd"])
def test_table_on_gpu_matches_cpu_table(optimizer, hp):
    kw = dict(rows=V, dim=200, lr=0.1, seed=2, optimizer=optimizer, **hp)
    tg = EmbeddingTable("t", device=DEV, **kw)
    tc = EmbeddingTable("t", **kw)
    assert tg.fused and all(s.device.type == "cuda"
                            for s in tg.state.values())
    gen = torch.Generator().manual_seed(8)
    for _ in range(2):
        ids = mixed_ids(gen, 300)
        g = dyadic(gen, ids.numel(), 200).to(torch.bfloat16)
        tg.push(ids.to(DEV), g.to(DEV))
        tc.push(ids, g)
        assert torch.allclose(tg.master.cpu(), tc.master, atol=1e-5)
        good = ids[(ids >= 0) & (ids < V)].to(DEV)
        assert torch.equal(tg.pull(good), tg.master[good].to(torch.bfloat16))
    for k in tc.state:
        assert torch.allclose(tg.state[k].cpu(), tc.state[k], atol=1e-5)
