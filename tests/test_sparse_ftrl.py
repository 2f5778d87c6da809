"""FTRL-Proximal ("ftrl_proximal") on the CPU: ops.fused_ftrl / sparse_ftrl
against a naive fp64 oracle, the first-touch seeding, exact thresholding by
l1, argument checks, and the optimizer through EmbeddingTable,
ShardedEmbeddingTable, HashedEmbeddingTable and PStore.

Inputs follow test_sparse_apply_gpu.py's recipe: V = 97, ~300 ids from
[0, 60) plus four invalid ones, grads randint(-32, 33)/16 (the summed
gradient is exact in fp32 in any order), grad_scale alternating 0.5 / 1,
5 pushes; lr 0.1, l1 0.5, l2 0.01, initial_accumulator_value 0.1; half of
the rows start never updated (accum = linear = 0), the other half with
accum = rand*0.5 and linear = rand-0.5. Tolerance: torch.allclose(atol=
1e-5) on master, accum and linear, what the sparse applies are held to."""

import math

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import (EmbeddingTable, HashedEmbeddingTable,
                                   ShardedEmbeddingTable)
from tfmesos_amd.ps.store import PStore

V = 97
INVALID = [-1, -5, V, V + 3]
HP = dict(lr=0.1, l1=0.5, l2=0.01, initial_accumulator_value=0.1)
TABLE_HP = {k: v for k, v in HP.items() if k != "lr"}


def dyadic(gen, *shape):
    return torch.randint(-32, 33, shape, generator=gen).float() / 16


def mixed_ids(gen, n_valid):
    ids = torch.cat([torch.randint(0, 60, (n_valid,), generator=gen),
                     torch.tensor(INVALID)])
    return ids[torch.randperm(ids.numel(), generator=gen)]


def init_state(D, gen, rows=V):
    """master, accum, linear: odd rows never updated, even rows with state."""
    p = torch.rand(rows, D, generator=gen)
    a = torch.rand(rows, D, generator=gen) * 0.5
    c = torch.rand(rows, D, generator=gen) - 0.5
    a[1::2] = 0
    c[1::2] = 0
    return p, a, c


def oracle_elem(p, a, c, g, lr, l1, l2, acc0):
    """The rule on Python floats (fp64), constants rounded to fp32 first."""
    def sign(x):
        return (x > 0) - (x < 0)
    if a == 0 and c == 0:
        c = -(p * (math.sqrt(acc0) / lr + 2 * l2) + sign(p) * l1)
    n_new = a + g * g
    s_old, s_new = math.sqrt(a + acc0), math.sqrt(n_new + acc0)
    z = c + (g - (s_new - s_old) / lr * p)
    p = (sign(z) * l1 - z) / (s_new / lr + 2 * l2) if abs(z) > l1 else 0.0
    return p, n_new, z


def oracle_push(p, a, c, ids, rows, gscale, lr, l1, l2,
                initial_accumulator_value):
    """Naive fp64 sparse FTRL-Proximal on fp64 tensors, in place: a loop
    over the touched rows, duplicates summed first. rows: one fp64 gradient
    row per position of ids."""
    f32 = [float(torch.tensor(x, dtype=torch.float32))
           for x in (lr, l1, l2, initial_accumulator_value, gscale)]
    lr, l1, l2, acc0, gscale = f32
    summed = {}
    for i, r in enumerate(ids.tolist()):
        if 0 <= r < p.shape[0]:
            summed[r] = summed.get(r, 0) + rows[i]
    for r, G in summed.items():
        for d in range(p.shape[1]):
            p[r, d], a[r, d], c[r, d] = oracle_elem(
                float(p[r, d]), float(a[r, d]), float(c[r, d]),
                float(G[d]) * gscale, lr, l1, l2, acc0)
    return set(summed)


def make_bags(gen, n, B):
    """B bags over n positions (some empty), weights in {0.25 .. 1}."""
    cuts = torch.sort(torch.randint(0, n + 1, (B - 1,), generator=gen))[0]
    offsets = torch.cat([torch.tensor([0]), cuts, torch.tensor([n])])
    weights = torch.randint(1, 5, (n,), generator=gen).float() / 4
    return offsets, weights


def bag_rows64(ids, offsets, weights, combiner, bag_grads):
    """Per-position fp64 rows c_i * bag_grads[bag of i]."""
    n = ids.numel()
    rows = torch.zeros(n, bag_grads.shape[1], dtype=torch.float64)
    for b in range(offsets.numel() - 1):
        s, e = int(offsets[b]), int(offsets[b + 1])
        w = [1.0 if weights is None else float(weights[i])
             for i in range(s, e)]
        W = sum(w)
        for i, wi in zip(range(s, e), w):
            ci = wi if combiner == "sum" else (wi / W if W else 0.0)
            rows[i] = ci * bag_grads[b].double()
    return rows


def assert_close(p, a, c, p64, a64, c64):
    for name, x, y in (("master", p, p64), ("accum", a, a64),
                       ("linear", c, c64)):
        err = (x.double() - y).abs().max().item()
        print("%s: max |err| vs fp64 oracle %.3g" % (name, err))
        assert torch.allclose(x, y.float(), atol=1e-5), name


# ------------------------------------------------------------------ the ops

@pytest.mark.parametrize("D", [8, 13])
def test_sparse_ftrl_rows_match_fp64_oracle(D):
    gen = torch.Generator().manual_seed(D)
    p, a, c = init_state(D, gen)
    sh = torch.full((V, D), 7.0, dtype=torch.bfloat16)
    p64, a64, c64 = p.double(), a.double(), c.double()
    touched = set()
    for k in range(1, 6):
        ids = mixed_ids(gen, 300)
        g = dyadic(gen, ids.numel(), D)
        gscale = 0.5 if k % 2 else 1.0
        before = [p.clone(), a.clone(), c.clone(), sh.clone()]
        ops.sparse_ftrl(p, ids, g, a, c, bf16_out=sh, grad_scale=gscale,
                        **HP)
        now = oracle_push(p64, a64, c64, ids, g.double(), gscale, **HP)
        touched |= now
        assert_close(p, a, c, p64, a64, c64)
        idle = torch.ones(V, dtype=torch.bool)
        idle[sorted(now)] = False
        for t, t0 in zip([p, a, c, sh], before):
            assert torch.equal(t[idle], t0[idle])
    tt = sorted(touched)
    assert tt and max(tt) < 60
    assert torch.equal(sh[tt], p[tt].to(torch.bfloat16))
    # l1 = 0.5 produces exact zeros, and not only zeros
    zeros = (p[tt] == 0).float().mean().item()
    assert 0.02 < zeros < 0.98, zeros


@pytest.mark.parametrize("combiner,weighted", [
    ("sum", False), ("sum", True), ("mean", False), ("mean", True)])
def test_sparse_ftrl_bags_match_fp64_oracle(combiner, weighted):
    D, B = 8, 40
    gen = torch.Generator().manual_seed(31)
    p, a, c = init_state(D, gen)
    p64, a64, c64 = p.double(), a.double(), c.double()
    for k in range(1, 4):
        ids = mixed_ids(gen, 150)
        offsets, weights = make_bags(gen, ids.numel(), B)
        weights = weights if weighted else None
        bg = dyadic(gen, B, D)
        gscale = 0.5 if k % 2 else 1.0
        ops.sparse_ftrl(p, ids, bg, a, c, grad_scale=gscale, offsets=offsets,
                        weights=weights, combiner=combiner, **HP)
        rows = bag_rows64(ids, offsets, weights, combiner, bg)
        oracle_push(p64, a64, c64, ids, rows, gscale, **HP)
        assert_close(p, a, c, p64, a64, c64)


@pytest.mark.parametrize("with_shadow", [False, True])
def test_fused_ftrl_matches_fp64_oracle(with_shadow):
    n = 203
    gen = torch.Generator().manual_seed(17)
    p, a, c = (t.view(-1)[:n].clone() for t in init_state(8, gen))
    p64, a64, c64 = (t.double().view(n, 1) for t in (p, a, c))
    sh = torch.zeros(n, dtype=torch.bfloat16) if with_shadow else None
    ids = torch.arange(n)
    for k in range(1, 4):
        g = dyadic(gen, n)
        gscale = 0.5 if k % 2 else 1.0
        ops.fused_ftrl(p, g, a, c, bf16_out=sh, grad_scale=gscale, **HP)
        oracle_push(p64, a64, c64, ids, g.double().view(n, 1), gscale, **HP)
        assert_close(p, a, c, p64.view(-1), a64.view(-1), c64.view(-1))
    if with_shadow:
        assert torch.equal(sh, p.to(torch.bfloat16))


def test_every_row_once_equals_fused_ftrl():
    gen = torch.Generator().manual_seed(4)
    p, a, c = init_state(8, gen)
    pd, ad, cd = p.clone(), a.clone(), c.clone()
    g = dyadic(gen, V, 8)
    ops.sparse_ftrl(p, torch.arange(V), g, a, c, grad_scale=0.5, **HP)
    ops.fused_ftrl(pd.view(-1), g.view(-1), ad.view(-1), cd.view(-1),
                   grad_scale=0.5, **HP)
    assert torch.equal(p, pd) and torch.equal(a, ad) and torch.equal(c, cd)


def test_zero_gradient_keeps_the_weight_and_seeds_linear():
    """A never-updated element's seeded linear term makes its current weight
    the FTRL solution: a zero (summed) gradient moves it by rounding only
    (measured 3e-8), also for weights under l1/quad that plain FTRL would
    zero."""
    gen = torch.Generator().manual_seed(5)
    D = 8
    for ids, g in ((torch.tensor([3, 9]), torch.zeros(2, D)),
                   (torch.tensor([3, 3]), None)):
        p = torch.rand(V, D, generator=gen) - 0.5
        p[3, 0] = 0.0
        p0 = p.clone()
        a, c = torch.zeros(V, D), torch.zeros(V, D)
        if g is None:
            row = dyadic(gen, 1, D)
            g = torch.cat([row, -row])
        ops.sparse_ftrl(p, ids, g, a, c, **HP)
        err = (p - p0).abs().max().item()
        print("zero-gradient push: max |master change| %.3g" % err)
        assert err <= 1e-6
        assert torch.equal(a, torch.zeros(V, D))
        assert p[3, 0] == 0 and c[3, 0] == 0
        assert (c[3, 1:] != 0).all() and (p0[3, 1:] != 0).all()
        idle = torch.ones(V, dtype=torch.bool)
        idle[ids] = False
        assert torch.equal(c[idle], torch.zeros(V, D)[idle])


def exact_threshold_case(gen, D, n_valid, hot=0):
    """Zero master and state, one push with duplicates, l1 = 1.01: z is the
    dyadic summed gradient G exactly. Returns (ids, grads, G [V,D], touched
    mask [V])."""
    ids = torch.randint(0, 60, (n_valid,), generator=gen)
    if hot:
        ids = torch.cat([ids, torch.full((hot,), 5)])
    ids = torch.cat([ids, torch.tensor(INVALID)])
    ids = ids[torch.randperm(ids.numel(), generator=gen)]
    g = dyadic(gen, ids.numel(), D)
    ok = (ids >= 0) & (ids < V)
    G = torch.zeros(V, D).index_add_(0, ids[ok], g[ok])
    touched = torch.zeros(V, dtype=torch.bool)
    touched[ids[ok]] = True
    return ids, g, G, touched


def check_exact_threshold(p, c, sh, G, touched, l1):
    """The bit-for-bit properties of the exact-thresholding case (tensors
    on any one device)."""
    assert torch.equal(c, G)
    zero = G.abs() <= l1
    assert torch.equal(p == 0, zero)
    assert torch.equal(sh == 0, zero)
    nz = ~zero
    assert torch.equal(torch.sign(p[nz]), -torch.sign(G[nz]))
    assert not torch.signbit(p[zero]).any()         # +0.0
    share = zero[touched].float().mean().item()
    print("exact thresholding: %.0f %% of the touched elements are zero"
          % (100 * share))
    assert 0.1 <= share <= 0.9


def test_exact_thresholding():
    gen = torch.Generator().manual_seed(23)
    D, l1 = 8, 1.01
    ids, g, G, touched = exact_threshold_case(gen, D, 120)
    p, a, c = torch.zeros(V, D), torch.zeros(V, D), torch.zeros(V, D)
    sh = torch.zeros(V, D, dtype=torch.bfloat16)
    ops.sparse_ftrl(p, ids, g, a, c, 0.1, l1=l1, l2=0.01, bf16_out=sh)
    check_exact_threshold(p, c, sh, G, touched, l1)
    assert torch.equal(a, G * G)


def test_invalid_arguments():
    p, a, c = torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(4, 4)
    ids, g = torch.tensor([1]), torch.ones(1, 4)
    bad = [dict(lr=0.0), dict(lr=-0.1), dict(lr=0.1, l1=-1.0),
           dict(lr=0.1, l2=-1.0),
           dict(lr=0.1, initial_accumulator_value=0.0),
           dict(lr=0.1, initial_accumulator_value=-0.1)]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.sparse_ftrl(p, ids, g, a, c, **kw)
        with pytest.raises(ValueError):
            ops.fused_ftrl(p.view(-1), torch.ones(16), a.view(-1),
                           c.view(-1), **kw)
    assert torch.equal(p, torch.zeros(4, 4))
    with pytest.raises(ValueError, match="no hyper-parameter"):
        EmbeddingTable("t", rows=4, dim=4, optimizer="ftrl_proximal",
                       weight_decay=0.01)
    with pytest.raises(ValueError, match="unknown sparse optimizer"):
        EmbeddingTable("t", rows=4, dim=4, optimizer="ftrl")
    with pytest.raises(ValueError):
        t = EmbeddingTable("t", rows=4, dim=4, optimizer="ftrl_proximal",
                           l1=-1.0)
        t.push(ids, g)


# --------------------------------------------------------------- the tables

def table(**kw):
    return EmbeddingTable("t", rows=V, dim=8, lr=0.1, seed=3,
                          optimizer="ftrl_proximal", **TABLE_HP, **kw)


def pushes(k, seed=12):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(k):
        ids = mixed_ids(gen, 80)
        out.append((ids, dyadic(gen, ids.numel(), 8).to(torch.bfloat16)))
    return out


def test_table_matches_the_op():
    t = table()
    assert t.fused and sorted(t.state) == ["accum", "linear"]
    assert all(not s.any() for s in t.state.values())
    p = t.master.clone()
    a, c = torch.zeros_like(p), torch.zeros_like(p)
    gen = torch.Generator().manual_seed(2)
    for k, (ids, g) in enumerate(pushes(3), 1):
        t.push(ids, g)
        ops.sparse_ftrl(p, ids, g, a, c, **HP)
        offsets, weights = make_bags(gen, ids.numel(), 20)
        bg = dyadic(gen, 20, 8)
        t.push_pooled(ids, offsets, bg, weights, "mean")
        ops.sparse_ftrl(p, ids, bg, a, c, offsets=offsets, weights=weights,
                        combiner="mean", **HP)
        assert torch.equal(t.master, p) and t.step == 2 * k
        good = ids[(ids >= 0) & (ids < V)]
        assert torch.equal(t.pull(good), p[good].to(torch.bfloat16))
    assert torch.equal(t.state["accum"], a)
    assert torch.equal(t.state["linear"], c)
    assert (t.master == 0).any()


def test_table_state_dict_roundtrip():
    ps = pushes(4)
    a = table()
    for ids, g in ps[:3]:
        a.push(ids, g)
    sd = a.state_dict()
    assert sd["optimizer"] == "ftrl_proximal"
    b = table()
    b.push(*ps[3])
    b.load_state_dict(sd)
    a.push(*ps[3])
    b.push(*ps[3])
    assert torch.equal(b.master, a.master) and b.step == a.step
    assert torch.equal(b.shadow, a.shadow)
    for k in ("accum", "linear"):
        assert torch.equal(b.state[k], a.state[k])
    other = EmbeddingTable("t", rows=V, dim=8, optimizer="adam")
    with pytest.raises(ValueError):
        other.load_state_dict(sd)
    with pytest.raises(ValueError):
        b.load_state_dict(other.state_dict())


@pytest.mark.parametrize("strategy", ["mod", "div"])
def test_sharded_table_equals_unsharded(strategy):
    kw = dict(lr=0.1, seed=3, optimizer="ftrl_proximal", **TABLE_HP)
    whole = EmbeddingTable("t", V, 8, **kw)
    sharded = ShardedEmbeddingTable("t", V, 8, 3, strategy, **kw)
    gen = torch.Generator().manual_seed(6)
    for ids, g in pushes(3):
        whole.push(ids, g)
        sharded.push(ids, g)
        offsets, weights = make_bags(gen, ids.numel(), 20)
        bg = dyadic(gen, 20, 8)
        whole.push_pooled(ids, offsets, bg, weights, "mean")
        sharded.push_pooled(ids, offsets, bg, weights, "mean")
    dense = sharded.to_dense()
    assert dense["optimizer"] == "ftrl_proximal" and dense["step"] == 6
    assert torch.equal(dense["master"], whole.master)
    assert torch.equal(dense["shadow"], whole.shadow)
    for k in ("accum", "linear"):
        assert torch.equal(dense["state"][k], whole.state[k])


@pytest.mark.parametrize("admit_after", [None, 2])
def test_hashed_table_against_dict_over_dense_oracle(admit_after):
    """The hashed table by key against the op on dense rows kept in a dict:
    a key gets its initial row (ops.hash_init_rows) and zero state when it
    is inserted — with admit_after=2, at its second push —, and again when
    it returns after an eviction."""
    D, cap, seed = 8, 64, 11
    kw = {} if admit_after is None else {"admit_after": admit_after}
    t = HashedEmbeddingTable("h", D, cap, lr=0.1, seed=seed,
                             optimizer="ftrl_proximal", **TABLE_HP, **kw)
    pool = torch.tensor([7, -3, 2 ** 40 + 1, 12345, 99, 5, 2 ** 61, 41])
    rows, seen = {}, {}       # key -> [p, a, c] of one row; push counts

    def oracle_push_keys(keys, g):
        for k in dict.fromkeys(keys.tolist()):
            seen[k] = seen.get(k, 0) + 1
            if k not in rows and seen[k] >= (admit_after or 1):
                init = ops.hash_init_rows(torch.tensor([k]), D, seed)
                rows[k] = [init.clone(), torch.zeros(1, D),
                           torch.zeros(1, D)]
        live = [k for k in dict.fromkeys(keys.tolist()) if k in rows]
        for k in live:
            p, a, c = rows[k]
            mine = keys == k
            ops.sparse_ftrl(p, torch.zeros(int(mine.sum()),
                                           dtype=torch.int64),
                            g[mine], a, c, **HP)

    def check():
        keys = torch.tensor(sorted(rows), dtype=torch.int64)
        r = ops.hash_find(t.index, keys)
        assert (r >= 0).all() and t.stats()["size"] == len(rows)
        for i, k in enumerate(keys.tolist()):
            p, a, c = rows[k]
            assert torch.equal(t.master[r[i]], p[0]), k
            assert torch.equal(t.state["accum"][r[i]], a[0]), k
            assert torch.equal(t.state["linear"][r[i]], c[0]), k
            assert torch.equal(t.shadow[r[i]], p[0].to(torch.bfloat16)), k

    gen = torch.Generator().manual_seed(8)
    for _ in range(4):
        keys = pool[torch.randint(0, pool.numel(), (30,), generator=gen)]
        g = dyadic(gen, 30, D).to(torch.bfloat16)
        t.push(keys, g)
        oracle_push_keys(keys, g)
        check()
    # one key leaves and returns: seeded again from its initial row
    gone = 12345
    assert gone in rows and rows[gone][1].any()
    t.remove(torch.tensor([gone]))
    del rows[gone]
    seen[gone] = 0 if admit_after is None else seen[gone]
    check()
    for _ in range(2):
        keys = torch.tensor([gone, 7, gone])
        g = dyadic(gen, 3, D).to(torch.bfloat16)
        t.push(keys, g)
        oracle_push_keys(keys, g)
        check()
    assert gone in rows
    # reserve and the checkpoint carry both state rows
    t.reserve(2 * cap)
    check()
    u = HashedEmbeddingTable("h", D, cap, lr=0.1, optimizer="ftrl_proximal",
                             **TABLE_HP, **kw)
    u.load_state_dict(t.state_dict())
    keys = pool[:5]
    g = dyadic(gen, 5, D).to(torch.bfloat16)
    t.push(keys, g)
    u.push(keys, g)
    n = t.stats()["size"]
    assert torch.equal(u.master[:n], t.master[:n])
    for k in ("accum", "linear"):
        assert torch.equal(u.state[k][:n], t.state[k][:n])


# ---------------------------------------------------------------- the store

def test_pstore_apply_flat_shard_and_checkpoint(tmp_path):
    gen = torch.Generator().manual_seed(9)
    params = [("w", torch.rand(30, 10, generator=gen) - 0.5),
              ("b", torch.rand(10, generator=gen) - 0.5)]
    store = PStore()
    store.init_params(params, optimizer="ftrl_proximal", **HP)
    assert sorted(store.state) == ["accum", "linear"]
    assert not store.state["accum"].any() and not store.state["linear"].any()
    n = store.flat.numel()
    p, a, c = store.flat.clone(), torch.zeros(n), torch.zeros(n)
    sh = store.flat_bf16.clone()
    for k in range(3):
        g = dyadic(gen, n)
        lo, hi = ((0, n), (256, n), (0, 256))[k]
        store.apply_flat(g, grad_scale=0.5, lo=lo, hi=hi)
        ops.fused_ftrl(p[lo:hi], g[lo:hi], a[lo:hi], c[lo:hi],
                       bf16_out=sh[lo:hi], grad_scale=0.5, **HP)
        assert torch.equal(store.flat, p)
        assert torch.equal(store.flat_bf16, sh)
        assert torch.equal(store.state["accum"], a)
        assert torch.equal(store.state["linear"], c)
    assert torch.equal(store.view("b"), p[store.offsets["b"][0]:][:10])
    path = str(tmp_path / "ck.pt")
    store.save(path)
    other = PStore()
    other.init_params(params, optimizer="sgd", lr=0.3)
    other.load(path)
    assert other.opt == "ftrl_proximal" and other.global_step == 3
    g = dyadic(gen, n)
    store.apply_flat(g)
    other.apply_flat(g)
    assert torch.equal(other.flat, store.flat)
    assert torch.equal(other.flat_bf16, store.flat_bf16)
    for k in ("accum", "linear"):
        assert torch.equal(other.state[k], store.state[k])
