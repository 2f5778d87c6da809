"""Row-sharded embedding tables on the CPU: ops.shard_partition and its
companions against a naive Python loop, and ShardedEmbeddingTable against
the unsharded EmbeddingTable."""

import functools

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import EmbeddingTable, ShardedEmbeddingTable

import test_embedding_bag_gpu as recipe     # the dyadic input recipe

V = 97
STRATEGIES = ["mod", "div"]
GEOMETRIES = [(97, 1), (97, 2), (97, 3), (97, 8), (97, 64), (64, 64)]


# ------------------------------------------------------------ the partition

def naive_route(i, rows, S, strategy):
    if not 0 <= i < rows:
        return 0, -1
    for s in range(S):
        gids = list(ops.shard_global_ids(rows, S, s, strategy))
        if i in gids:
            return s, gids.index(i)
    raise AssertionError("id %d is on no shard" % i)


def naive_partition(ids, rows, S, strategy):
    slots = [[] for _ in range(S)]
    for pos, i in enumerate(ids.tolist()):
        s, local = naive_route(i, rows, S, strategy)
        slots[s].append((pos, local))
    flat = [x for sl in slots for x in sl]
    perm = torch.tensor([p for p, _ in flat], dtype=torch.int64)
    local = torch.tensor([lo for _, lo in flat], dtype=torch.int64)
    inv = torch.empty_like(perm)
    for slot, (p, _) in enumerate(flat):
        inv[p] = slot
    starts = torch.tensor([0] + [len(sl) for sl in slots]).cumsum(0)
    return local, perm, inv, starts


def make_ids(n, rows, seed=0):
    gen = torch.Generator().manual_seed(seed + n)
    ids = torch.randint(0, rows, (n,), generator=gen)
    bad = torch.tensor([-1, -5, rows, rows + 3])
    if n >= 8:
        ids[torch.randperm(n, generator=gen)[:4]] = bad
    return ids


def check_partition(part, ids, rows, S, strategy):
    local, perm, inv, starts = naive_partition(ids, rows, S, strategy)
    n = ids.numel()
    assert torch.equal(part.local, local) and torch.equal(part.perm, perm)
    assert torch.equal(part.inv, inv) and torch.equal(part.starts, starts)
    assert part.starts.shape == (S + 1,) and int(part.starts[-1]) == n
    # inverse permutations
    assert torch.equal(part.perm[part.inv], torch.arange(n))
    assert torch.equal(part.inv[part.perm], torch.arange(n))
    # stability: positions increase inside every shard
    for s in range(S):
        seg = part.perm[int(part.starts[s]):int(part.starts[s + 1])]
        assert bool((seg[1:] > seg[:-1]).all())


@pytest.mark.parametrize("n", [0, 1, 65, 1000])
@pytest.mark.parametrize("rows,S", GEOMETRIES)
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_partition_matches_naive_loop(strategy, rows, S, n):
    ids = make_ids(n, rows)
    check_partition(ops.shard_partition(ids, rows, S, strategy), ids, rows,
                    S, strategy)


@pytest.mark.parametrize("rows,S", GEOMETRIES)
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_all_ids_on_one_shard_and_coverage(strategy, rows, S):
    last = torch.tensor(list(ops.shard_global_ids(rows, S, S - 1, strategy)))
    ids = last[torch.arange(70) % last.numel()]
    part = ops.shard_partition(ids, rows, S, strategy)
    check_partition(part, ids, rows, S, strategy)
    assert part.starts.tolist() == [0] * S + [70]
    # the shards cover [0, rows) exactly once, with shard_rows rows each
    seen = []
    for s in range(S):
        gids = list(ops.shard_global_ids(rows, S, s, strategy))
        assert len(gids) == ops.shard_rows(rows, S, s, strategy) >= 1
        seen += gids
    assert sorted(seen) == list(range(rows))
    if strategy == "div":       # the first rows % S shards hold one more
        sizes = [ops.shard_rows(rows, S, s, "div") for s in range(S)]
        assert sizes == sorted(sizes, reverse=True)
        assert max(sizes) - min(sizes) <= 1


def test_partition_argument_errors():
    ids = torch.arange(5)
    for rows, S, strategy in [(97, 0, "mod"), (97, 65, "mod"),
                              (7, 8, "div"), (97, 2, "hash")]:
        with pytest.raises(ValueError):
            ops.shard_partition(ids, rows, S, strategy)
        with pytest.raises(ValueError):
            ops.shard_rows(rows, S, 0, strategy)
        with pytest.raises(ValueError):
            ops.shard_global_ids(rows, S, 0, strategy)
        with pytest.raises(ValueError):
            ShardedEmbeddingTable("t", rows, 4, S, strategy)


def test_permute_rows_bag_offsets_and_coefficients():
    gen = torch.Generator().manual_seed(3)
    ids, offsets, weights = recipe.make_bags(gen, recipe.SUM_LENS, "sum",
                                             True)
    n, B = ids.numel(), offsets.numel() - 1
    part = ops.shard_partition(ids, V, 3, "mod")
    rows = recipe.dyadic(gen, n, 7)
    out = ops.permute_rows(rows, part.perm, torch.bfloat16)
    assert out.dtype == torch.bfloat16
    for j in range(n):
        assert torch.equal(out[j], rows[int(part.perm[j])].to(torch.bfloat16))
    assert ops.permute_rows(rows, part.perm).dtype == torch.float32
    so = ops.shard_bag_offsets(part.perm, part.starts, offsets)
    assert so.shape == (3, B + 1) and so.dtype == torch.int64
    for s in range(3):
        seg = part.perm[int(part.starts[s]):int(part.starts[s + 1])].tolist()
        for b in range(B + 1):
            assert int(so[s, b]) == sum(1 for p in seg if p < int(offsets[b]))
    for combiner in ("sum", "mean"):
        for w in (None, weights):
            c = ops.bag_coefficients(n, offsets, w, combiner)
            assert c.dtype == torch.float32 and c.shape == (n,)
            table = recipe.dyadic(gen, V, 6)
            assert torch.equal(
                ops.embedding_bag(table, ids, offsets, c, "sum"),
                ops.embedding_bag(table, ids, offsets, w, combiner))
    with pytest.raises(ValueError):
        ops.bag_coefficients(n, offsets, weights[:-1])
    with pytest.raises(ValueError):
        ops.bag_coefficients(n, offsets, combiner="max")


# ------------------------------------------- sharded against unsharded tables

OPTIMIZERS = [("adagrad", {}), ("adam", {}), ("sgd", {"momentum": 0.9})]
D = 8


def one_shard_ids(S, strategy):
    """Valid ids that all live on shard S - 1."""
    g = ops.shard_global_ids(V, S, S - 1, strategy)
    return torch.tensor(list(g))[torch.tensor([0, 3, 1, 3, 2, 0, 5])]


@functools.lru_cache(maxsize=None)
def script(S, strategy):
    """Row and pooled requests in all four (combiner, weighted) modes,
    invalid ids in the pushes, and a row and a pooled push that hit no row
    of any shard but the last."""
    gen = torch.Generator().manual_seed(40 + S)
    reqs = []
    for k, (combiner, weighted) in enumerate(recipe.MODES):
        ids, offsets, weights = recipe.make_bags(
            gen, recipe.lens_for(combiner, weighted), combiner, weighted)
        ids = torch.where((ids >= 0) & (ids < V), (ids * 7 + k) % V, ids)
        g = recipe.dyadic(gen, offsets.numel() - 1, D)
        row_ids = torch.cat([torch.randint(0, V, (70,), generator=gen),
                             torch.tensor(recipe.INVALID)])
        row_g = recipe.dyadic(gen, row_ids.numel(), D)
        reqs.append(("push_pooled", ids, offsets, g, weights, combiner))
        reqs.append(("push", row_ids, row_g))
        reqs.append(("pull", row_ids[:70]))
    one = one_shard_ids(S, strategy)
    reqs.append(("push", one, recipe.dyadic(gen, one.numel(), D)))
    reqs.append(("push_pooled", one, torch.tensor([0, 3, 3, 7]),
                 recipe.dyadic(gen, 3, D), None, "mean"))
    reqs.append(("pull", one))
    return reqs


def run_script(table, reqs):
    pulled = []
    for method, *args in reqs:
        out = getattr(table, method)(*args)
        if out is not None:
            pulled.append(out)
    return pulled


def assert_same_state(sharded, plain):
    dense = sharded.to_dense()
    assert dense["step"] == sharded.step == plain.step
    assert torch.equal(dense["master"], plain.master)
    assert torch.equal(dense["shadow"], plain.shadow)
    assert sorted(dense["state"]) == sorted(plain.state)
    for k in plain.state:
        assert torch.equal(dense["state"][k], plain.state[k]), k


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("optimizer,hp", OPTIMIZERS,
                         ids=["adagrad", "adam", "sgd_mom"])
def test_sharded_table_equals_unsharded(optimizer, hp, S, strategy):
    kw = dict(rows=V, dim=D, lr=0.1, seed=4, optimizer=optimizer, **hp)
    plain = EmbeddingTable("t", **kw)
    sharded = ShardedEmbeddingTable("t", num_shards=S, strategy=strategy,
                                    **kw)
    assert_same_state(sharded, plain)         # shard_of: the same init
    for s, t in enumerate(sharded.shards):
        assert t.rows == ops.shard_rows(V, S, s, strategy)
    reqs = script(S, strategy)
    got, want = run_script(sharded, reqs), run_script(plain, reqs)
    assert_same_state(sharded, plain)
    assert sharded.step == sum(1 for r in reqs if r[0].startswith("push"))
    assert not torch.equal(plain.master, EmbeddingTable("t", **kw).master)
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):               # row pulls
        assert a.dtype == torch.bfloat16 and torch.equal(a, b)
    # pooled pulls: bags inside one shard, and any bags when S == 1
    one = one_shard_ids(S, strategy)
    offsets = torch.tensor([0, 3, 3, 7])
    w = torch.tensor([0.5, 1.0, 2.0, 1.0, 1.0, 0.5, 2.0])
    cases = [(one, offsets, None, "sum"), (one, offsets, w, "mean")]
    if S == 1:
        cases += [r[1:3] + r[4:] for r in reqs if r[0] == "push_pooled"]
    for ids, offs, weights, combiner in cases:
        assert torch.equal(sharded.pull_pooled(ids, offs, weights, combiner),
                           plain.pull_pooled(ids, offs, weights, combiner))


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("S", [2, 3, 8])
def test_pooled_pull_across_shards_within_bf16_bound(S, strategy):
    """|got - exact| <= 2**-8 * 1.01 * sum_s |p_s| elementwise, p_s the
    fp32 per-shard partials. Dyadic inputs make the p_s and their sum
    exact. One bf16 rounding errs by up to 2**-8 relative (8 significand
    bits: 17.9375 -> 18.0), so the bound leaves room for exactly ONE
    rounding: the shards answer with their fp32 partials, the sum is
    rounded once, and the error is at most 2**-8 |sum_s p_s|. (Partials
    rounded to bf16 before the sum measured up to 1.65 * 2**-8 sum|p_s|
    on these inputs.)"""
    sharded = ShardedEmbeddingTable("t", V, D, S, strategy, optimizer="adam")
    gen = torch.Generator().manual_seed(50 + S)
    sd = sharded.state_dict()
    dense = recipe.dyadic(gen, V, D)
    for s, shard_sd in enumerate(sd["shards"]):
        gids = torch.tensor(list(ops.shard_global_ids(V, S, s, strategy)))
        shard_sd["master"] = dense[gids]
    sharded.load_state_dict(sd)
    assert torch.equal(sharded.to_dense()["master"], dense)
    differs = 0
    for combiner, weighted in recipe.MODES:
        ids, offsets, weights = recipe.make_bags(
            gen, recipe.lens_for(combiner, weighted), combiner, weighted)
        valid = (ids >= 0) & (ids < V)
        ids = torch.where(valid, (ids * 5) % V, ids)    # spread over V
        part = ops.shard_partition(ids, V, S, strategy)
        shard_of = torch.empty_like(ids)
        for s in range(S):
            seg = part.perm[int(part.starts[s]):int(part.starts[s + 1])]
            shard_of[seg] = s
        partials = [ops.embedding_bag(
            dense, torch.where(shard_of == s, ids, torch.full_like(ids, -1)),
            offsets, weights, combiner) for s in range(S)]
        exact = sum(partials)
        assert torch.equal(exact, ops.embedding_bag(dense, ids, offsets,
                                                    weights, combiner))
        got = sharded.pull_pooled(ids, offsets, weights, combiner)
        assert got.dtype == torch.bfloat16
        err = (got.float() - exact).abs()
        mass = sum(p.abs() for p in partials)
        worst = (err / mass.clamp(min=2.0 ** -20)).max() * 2 ** 8
        print("S=%d %s %s%s: max err / sum|p_s| = %.3f * 2**-8"
              % (S, strategy, combiner, ", weighted" if weighted else "",
                 worst))
        assert bool((err <= 2 ** -8 * 1.01 * mass).all())
        differs += int((err > 0).any())
    assert differs      # the rounding this bound is about did occur


def test_state_dict_round_trip():
    kw = dict(rows=V, dim=D, lr=0.1, seed=4, optimizer="adam")
    a = ShardedEmbeddingTable("t", num_shards=3, strategy="div", **kw)
    reqs = script(3, "div")
    run_script(a, reqs[:6])
    b = ShardedEmbeddingTable("t", num_shards=3, strategy="div",
                              **dict(kw, seed=99))
    b.load_state_dict(a.state_dict())
    assert b.step == a.step == 4
    for x, y in zip(run_script(a, reqs[6:]), run_script(b, reqs[6:])):
        assert torch.equal(x, y)
    da, db = a.to_dense(), b.to_dense()
    assert torch.equal(da["master"], db["master"])
    assert torch.equal(da["shadow"], db["shadow"])
    for k in da["state"]:
        assert torch.equal(da["state"][k], db["state"][k])
    with pytest.raises(ValueError):
        ShardedEmbeddingTable("t", num_shards=2, strategy="div",
                              **kw).load_state_dict(a.state_dict())
    with pytest.raises(ValueError):
        ShardedEmbeddingTable("t", num_shards=3, strategy="mod",
                              **kw).load_state_dict(a.state_dict())
