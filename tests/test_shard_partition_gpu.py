"""Row-sharded embedding tables on the GPU — csrc/partition.hip — against
the CPU references of ops.shard_partition, permute_rows, shard_bag_offsets
and bag_coefficients, and ShardedEmbeddingTable against an unsharded
EmbeddingTable on the same device.

Everything compares torch.equal: the outputs are integers, exact casts of
dyadic values (randint(-32, 33)/16 is exact in bf16) or coefficients on
the dyadic grid of test_embedding_bag_gpu.py's recipe. Sharded and
unsharded tables run the same bit-reproducible kernels, and the stable
partition keeps every row's contributions in request order."""

import functools

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import EmbeddingTable, ShardedEmbeddingTable

import test_embedding_bag_gpu as recipe
import test_shard_dist as dist_test

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V = 97
STRATEGIES = ["mod", "div"]


def gpu(t):
    return None if t is None else t.to(DEV)


# ---------------------------------------------------------- shard_partition

@functools.lru_cache(maxsize=None)
def partition_case(n, S, strategy):
    gen = torch.Generator().manual_seed(1000 * S + n)
    ids = torch.randint(0, V, (n,), generator=gen)
    if n >= 8:
        ids[torch.randperm(n, generator=gen)[:4]] = torch.tensor(
            recipe.INVALID)
    return ids, ops.shard_partition(ids, V, S, strategy)


def assert_partition(got, want):
    for name in ("local", "perm", "inv", "starts"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == torch.int64 and a.shape == b.shape, name
        assert torch.equal(a.cpu(), b), name


@pytest.mark.parametrize("S", [1, 2, 3, 8, 64])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_partition_matches_cpu(n, S):
    """Wave (64) and block (256) window edges, both strategies, the four
    invalid ids; two runs give identical bits."""
    for strategy in STRATEGIES:
        ids, want = partition_case(n, S, strategy)
        got = ops.shard_partition(ids.to(DEV), V, S, strategy)
        assert_partition(got, want)
        again = ops.shard_partition(ids.to(DEV), V, S, strategy)
        for a, b in zip(got, again):
            assert torch.equal(a, b)


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("S", [3, 64])
def test_partition_every_id_on_last_shard(S, strategy):
    last = torch.tensor(list(ops.shard_global_ids(V, S, S - 1, strategy)))
    ids = last[torch.arange(300) % last.numel()]
    got = ops.shard_partition(ids.to(DEV), V, S, strategy)
    assert_partition(got, ops.shard_partition(ids, V, S, strategy))
    assert got.starts.tolist() == [0] * S + [300]
    assert torch.equal(got.perm.cpu(), torch.arange(300))


def test_partition_argument_errors():
    ids = torch.arange(5, device=DEV)
    for rows, S, strategy in [(97, 0, "mod"), (97, 65, "mod"),
                              (7, 8, "div"), (97, 2, "hash")]:
        with pytest.raises(ValueError):
            ops.shard_partition(ids, rows, S, strategy)


# ------------------------------------------------------------- permute_rows

@pytest.mark.parametrize("dtypes", [(torch.float32, torch.bfloat16),
                                    (torch.bfloat16, torch.bfloat16),
                                    (torch.float32, torch.float32)],
                         ids=["f32_bf16", "bf16_bf16", "f32_f32"])
@pytest.mark.parametrize("D", [7, 8, 130])
def test_permute_rows_matches_cpu(D, dtypes):
    """Scalar path (7), vector path (8), even but no multiple of 4 (130);
    n = 0, 1, 65, 257 (more than one block)."""
    src, dst = dtypes
    for n in (0, 1, 65, 257):
        gen = torch.Generator().manual_seed(D + n)
        rows = recipe.dyadic(gen, n, D).to(src)
        perm = torch.randperm(n, generator=gen)
        want = ops.permute_rows(rows, perm, dst)
        got = ops.permute_rows(rows.to(DEV), perm.to(DEV), dst)
        assert got.dtype == dst and got.shape == (n, D)
        assert torch.equal(got.cpu(), want)
        assert n < 2 or not torch.equal(want, rows.to(dst))


def test_permute_rows_unaligned_view_takes_scalar_path():
    """D % 4 == 0 but the rows start 4 bytes into their storage."""
    gen = torch.Generator().manual_seed(5)
    rows = recipe.dyadic(gen, 65, 8)
    perm = torch.randperm(65, generator=gen)
    flat = torch.zeros(65 * 8 + 1, device=DEV)
    view = flat[1:].view(65, 8)
    view.copy_(rows)
    got = ops.permute_rows(view, perm.to(DEV), torch.bfloat16)
    assert torch.equal(got.cpu(), ops.permute_rows(rows, perm,
                                                   torch.bfloat16))


# ------------------------------------- shard_bag_offsets / bag_coefficients

@functools.lru_cache(maxsize=None)
def bag_case(combiner, weighted):
    gen = torch.Generator().manual_seed(30 + len(combiner) + weighted)
    ids, offsets, weights = recipe.make_bags(
        gen, recipe.lens_for(combiner, weighted), combiner, weighted)
    c = ops.bag_coefficients(ids.numel(), offsets, weights, combiner)
    table = recipe.dyadic(gen, V, 8)
    return ids, offsets, weights, c, table


@pytest.mark.parametrize("combiner,weighted", recipe.MODES,
                         ids=["sum", "mean_w", "sum_w", "mean"])
def test_bag_offsets_and_coefficients_match_cpu(combiner, weighted):
    """Bags of 0, 1, 63, 64, 65, 130 ids (or power-of-two lengths / weight
    sums for mean) and short bags. The coefficients fed back as weights
    with combiner "sum" reproduce the original call bit for bit."""
    ids, offsets, weights, c, table = bag_case(combiner, weighted)
    n = ids.numel()
    got_c = ops.bag_coefficients(n, gpu(offsets), gpu(weights), combiner)
    assert got_c.dtype == torch.float32 and torch.equal(got_c.cpu(), c)
    for S in (1, 3, 64):
        for strategy in STRATEGIES:
            want = ops.shard_partition(ids, V, S, strategy)
            part = ops.shard_partition(gpu(ids), V, S, strategy)
            so = ops.shard_bag_offsets(part.perm, part.starts, gpu(offsets))
            assert so.shape == (S, offsets.numel())
            assert torch.equal(so.cpu(), ops.shard_bag_offsets(
                want.perm, want.starts, offsets))
            assert torch.equal(so[:, -1], part.starts[1:] - part.starts[:-1])
    for tdtype in (torch.bfloat16, torch.float32):
        t = table.to(DEV, tdtype)
        assert torch.equal(
            ops.embedding_bag(t, gpu(ids), gpu(offsets), got_c, "sum"),
            ops.embedding_bag(t, gpu(ids), gpu(offsets), gpu(weights),
                              combiner))


def test_bag_coefficients_general_mean_bits():
    """Non-dyadic coefficients (bags of 3, 5, 7; random weights): c as
    weights with "sum" still equals the "mean" call bit for bit."""
    table, ids, offsets, _, _, _ = recipe.odd_mean_case()
    gen = torch.Generator().manual_seed(8)
    w = torch.rand(ids.numel(), generator=gen) + 0.5
    t = table.to(DEV, torch.bfloat16)
    for weights in (None, gpu(w)):
        c = ops.bag_coefficients(ids.numel(), gpu(offsets), weights, "mean")
        assert torch.equal(
            ops.embedding_bag(t, gpu(ids), gpu(offsets), c, "sum"),
            ops.embedding_bag(t, gpu(ids), gpu(offsets), weights, "mean"))
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    assert ops.bag_coefficients(0, torch.zeros(4, dtype=torch.int64,
                                               device=DEV)).shape == (0,)
    assert ops.permute_rows(torch.zeros(0, 8, device=DEV), none).shape == \
        (0, 8)


# --------------------------------------------- sharded against unsharded table

@functools.lru_cache(maxsize=None)
def script(D):
    """Row and pooled pushes in all four (combiner, weighted) modes with the
    invalid ids, a row push and a pooled push that hit only rows 0..5 (one
    shard under "div", not every shard under "mod" with 3), and row pulls."""
    gen = torch.Generator().manual_seed(60 + D)
    reqs = []
    for k, (combiner, weighted) in enumerate(recipe.MODES):
        ids, offsets, weights = recipe.make_bags(
            gen, recipe.lens_for(combiner, weighted), combiner, weighted)
        ids = torch.where((ids >= 0) & (ids < V), (ids * 7 + k) % V, ids)
        g = recipe.dyadic(gen, offsets.numel() - 1, D).to(torch.bfloat16)
        row_ids = torch.cat([torch.randint(0, V, (300,), generator=gen),
                             torch.tensor(recipe.INVALID)])
        row_g = recipe.dyadic(gen, row_ids.numel(), D).to(torch.bfloat16)
        reqs.append(("push_pooled", ids, offsets, g, weights, combiner))
        reqs.append(("push", row_ids, row_g))
        reqs.append(("pull", row_ids))
    few = torch.tensor([0, 2, 4, 2, 0, 4, 4])
    reqs.append(("push", few, recipe.dyadic(gen, 7, D)))
    reqs.append(("push_pooled", few, torch.tensor([0, 3, 3, 7]),
                 recipe.dyadic(gen, 3, D), None, "mean"))
    reqs.append(("pull", few))
    return [tuple(gpu(a) if torch.is_tensor(a) else a for a in r)
            for r in reqs]


def run_script(table, reqs):
    pulled = []
    for method, *args in reqs:
        out = getattr(table, method)(*args)
        if out is not None:
            pulled.append(out)
    return pulled


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("D", [8, 130])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_sharded_table_equals_unsharded_on_gpu(optimizer, S, D, strategy):
    kw = dict(rows=V, dim=D, lr=0.1, seed=4, optimizer=optimizer, device=DEV)
    plain = EmbeddingTable("t", **kw)
    sharded = ShardedEmbeddingTable("t", num_shards=S, strategy=strategy,
                                    **kw)
    master0 = plain.master.clone()
    assert torch.equal(sharded.to_dense()["master"], master0)
    reqs = script(D)
    got, want = run_script(sharded, reqs), run_script(plain, reqs)
    dense = sharded.to_dense()
    assert dense["step"] == plain.step == 10
    assert torch.equal(dense["master"], plain.master)
    assert torch.equal(dense["shadow"], plain.shadow)
    assert sorted(dense["state"]) == sorted(plain.state)
    for k in plain.state:
        assert torch.equal(dense["state"][k], plain.state[k]), k
    assert not torch.equal(plain.master, master0)
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):                 # row pulls, request order
        assert a.dtype == torch.bfloat16 and torch.equal(a, b)
    assert (got[0][-4:] == 0).all()             # invalid ids: zero rows


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("S", [2, 3])
def test_pooled_pull_across_shards_within_bf16_bound_on_gpu(S, strategy):
    """|got - exact| <= 2**-8 * 1.01 * sum_s |p_s| with the exact fp32
    per-shard partials p_s of the dyadic recipe. One bf16 rounding errs by
    up to 2**-8 relative, so the bound leaves room for exactly one: the
    shards answer with fp32 partials and the sum is rounded once (see the
    CPU twin in test_shard_partition.py; partials rounded to bf16 before
    the sum measured up to 1.59 * 2**-8 sum|p_s| here)."""
    D = 8
    gen = torch.Generator().manual_seed(70 + S)
    dense = recipe.dyadic(gen, V, D)
    sharded = ShardedEmbeddingTable("t", V, D, S, strategy, device=DEV,
                                    optimizer="adam")
    sd = sharded.state_dict()
    for s, shard_sd in enumerate(sd["shards"]):
        gids = torch.tensor(list(ops.shard_global_ids(V, S, s, strategy)))
        shard_sd["master"] = dense[gids]
    sharded.load_state_dict(sd)
    differs = 0
    for combiner, weighted in recipe.MODES:
        ids, offsets, weights = recipe.make_bags(
            gen, recipe.lens_for(combiner, weighted), combiner, weighted)
        ids = torch.where((ids >= 0) & (ids < V), (ids * 5) % V, ids)
        part = ops.shard_partition(ids, V, S, strategy)
        shard_of = torch.empty_like(ids)
        for s in range(S):
            seg = part.perm[int(part.starts[s]):int(part.starts[s + 1])]
            shard_of[seg] = s
        partials = [ops.embedding_bag(
            dense, torch.where(shard_of == s, ids, torch.full_like(ids, -1)),
            offsets, weights, combiner) for s in range(S)]
        exact, mass = sum(partials), sum(p.abs() for p in partials)
        got = sharded.pull_pooled(gpu(ids), gpu(offsets), gpu(weights),
                                  combiner)
        assert got.dtype == torch.bfloat16
        err = (got.cpu().float() - exact).abs()
        print("S=%d %s %s%s: max err / sum|p_s| = %.3f * 2**-8"
              % (S, strategy, combiner, ", weighted" if weighted else "",
                 (err / mass.clamp(min=2.0 ** -20)).max() * 2 ** 8))
        assert bool((err <= 2 ** -8 * 1.01 * mass).all())
        differs += int((err > 0).any())
    assert differs      # the rounding this bound is about did occur


# ---------------------------------------------------------------- end to end

@pytest.mark.timeout(400)
def test_sharded_protocol_on_gpu(tmp_path):
    """2 PS ranks + 1 worker, all on cuda:0, over gloo: the helper's script
    once. Each process has its own timeout; nothing is started after the
    three ranks, and a rank that exits nonzero fails the test before the
    local comparison runs."""
    pulls = str(tmp_path / "pulls.pt")
    sums = dist_test.run_world(3, pulls, device=DEV, timeout=120)
    assert sorted(sums) == ["S/0", "S/1", "U/0"]
    dist_test.check_against_local(3, sums, pulls, device=DEV)
