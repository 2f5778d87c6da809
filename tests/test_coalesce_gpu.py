"""Worker-side coalescing on the GPU — csrc/coalesce.hip — against the CPU
references of ops.coalesce_ids and ops.segment_sum_rows, tables fed
coalesced pushes against tables fed the raw ones, and the ``coalesce=`` mode
of SparseWorkerClient end to end.

Everything compares torch.equal. coalesce_ids returns integers. The rows
of the segment_sum_rows cases are dyadic (randint(-32, 33)/16, exact in
bf16): with at most 1300 rows per sum every partial sum stays far below
2**24 steps of the 1/16 grid, so the fp32 sum is exact in ANY order and the
single rounding to bf16 is the reference's. The table-level cases use
randint(-4, 5)/16 over 40 positions: every per-id sum (|sum| <= 10, a
multiple of 1/16) is exact in bf16, so summing before or after the bf16
rounding hands the optimizer the same gradient."""

import functools

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import EmbeddingTable, ShardedEmbeddingTable

import _sparse_coalesce_proc as proc
import test_coalesce as cpu_test
import test_embedding_bag_gpu as recipe

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V = 97
FIELDS = ("uniq", "inverse", "perm", "seg", "count")


# -------------------------------------------------------------- coalesce_ids

@functools.lru_cache(maxsize=None)
def ids_case(n, kind):
    gen = torch.Generator().manual_seed(300 + n)
    if kind == "distinct":
        ids = torch.randperm(n, generator=gen)
    elif kind == "equal":
        ids = torch.full((n,), 11, dtype=torch.int64)
    else:
        ids = torch.randint(0, V, (n,), generator=gen)
        if n >= 8:
            ids[torch.randperm(n, generator=gen)[:4]] = torch.tensor(
                recipe.INVALID)
    return ids, ops.coalesce_ids(ids)


@pytest.mark.parametrize("kind", ["random", "distinct", "equal"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_coalesce_ids_matches_cpu(n, kind):
    """Wave (64) and block (256) window edges; the four invalid ids are
    distinct values like any other; two runs give identical bits."""
    ids, want = ids_case(n, kind)
    got = ops.coalesce_ids(ids.to(DEV))
    again = ops.coalesce_ids(ids.to(DEV))
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == torch.int64 and a.shape == b.shape, name
        assert a.device.type == "cuda", name
        assert torch.equal(a.cpu(), b), name
        assert torch.equal(a, getattr(again, name)), name
    if kind == "random" and n >= 8:
        u = int(want.count)
        assert want.uniq[:2].tolist() == [-5, -1]
        assert want.uniq[u - 2:u].tolist() == [V, V + 3]


# ---------------------------------------------------------- segment_sum_rows

@functools.lru_cache(maxsize=None)
def rows_case(n, D):
    """ids over 23 values (runs of ~3 at n = 65, ~11 at n = 257), dyadic
    fp32 rows and the CPU coalescing."""
    gen = torch.Generator().manual_seed(400 + 7 * n + D)
    ids = torch.randint(0, 23, (n,), generator=gen)
    return ids, recipe.dyadic(gen, n, D), ops.coalesce_ids(ids)


@pytest.mark.parametrize("dtypes", cpu_test.DTYPES, ids=cpu_test.DTYPE_IDS)
@pytest.mark.parametrize("D", [7, 8, 130, 320])
def test_segment_sum_rows_matches_cpu(D, dtypes):
    """Scalar path (7), vector path (8), even but no multiple of 4 (130),
    more than one 256-column tile (320); n = 0, 1, 65, 257 (more than one
    block of output rows at D = 320)."""
    src, dst = dtypes
    for n in (0, 1, 65, 257):
        ids, rows, co = rows_case(n, D)
        rows = rows.to(src)
        u = int(co.count)
        want = ops.segment_sum_rows(rows, co.perm, co.seg, u, dst)
        g = ops.coalesce_ids(ids.to(DEV))
        got = ops.segment_sum_rows(rows.to(DEV), g.perm, g.seg, u, dst)
        assert got.dtype == dst and got.shape == (u, D)
        assert torch.equal(got.cpu(), want)
        assert n < 65 or 1 < u < n


def test_segment_sum_rows_unaligned_view_takes_scalar_path():
    """D % 4 == 0 but the rows start 4 bytes into their storage."""
    ids, rows, co = rows_case(65, 8)
    u = int(co.count)
    flat = torch.zeros(65 * 8 + 1, device=DEV)
    view = flat[1:].view(65, 8)
    view.copy_(rows)
    assert view.data_ptr() % 16 == 4
    got = ops.segment_sum_rows(view, co.perm.to(DEV), co.seg.to(DEV), u,
                               torch.bfloat16)
    assert torch.equal(got.cpu(), ops.segment_sum_rows(
        rows, co.perm, co.seg, u, torch.bfloat16))


@functools.lru_cache(maxsize=None)
def hot_case(kind, D):
    """n = 1500. "one": id 15 at 1300 positions (more than two 512-position
    pieces; its run starts off every window edge), the rest spread over 30
    other ids. "two": ids 4 and 20 at 700 and 600 positions (two long runs
    whose scratch slots must not collide). Dyadic fp32 rows."""
    gen = torch.Generator().manual_seed(500 + D)
    hot = {"one": [(15, 1300)], "two": [(4, 700), (20, 600)]}[kind]
    rest = 1500 - sum(c for _, c in hot)
    others = torch.tensor([i for i in range(31 + len(hot) - 1)
                           if i not in [h for h, _ in hot]][:30])
    ids = torch.cat([others[torch.randint(0, 30, (rest,), generator=gen)]]
                    + [torch.full((c,), h) for h, c in hot])
    ids = ids[torch.randperm(1500, generator=gen)]
    return ids, recipe.dyadic(gen, 1500, D), ops.coalesce_ids(ids)


@pytest.mark.parametrize("kind", ["one", "two"])
@pytest.mark.parametrize("D", [7, 8, 320])
def test_segment_sum_rows_hot_ids(D, kind):
    ids, rows, co = hot_case(kind, D)
    u = int(co.count)
    lens = (co.seg[1:u + 1] - co.seg[:u]).tolist()
    assert sorted(lens)[-1] == (1300 if kind == "one" else 700)
    assert sum(1 for ln in lens if ln > 512) == (1 if kind == "one" else 2)
    g = ops.coalesce_ids(ids.to(DEV))
    for name in FIELDS:
        assert torch.equal(getattr(g, name).cpu(), getattr(co, name)), name
    for dst in (torch.bfloat16, torch.float32):
        want = ops.segment_sum_rows(rows, co.perm, co.seg, u, dst)
        got = ops.segment_sum_rows(rows.to(DEV), g.perm, g.seg, u, dst)
        assert torch.equal(got.cpu(), want)
        again = ops.segment_sum_rows(rows.to(DEV), g.perm, g.seg, u, dst)
        assert torch.equal(got, again)
    # the bf16 rounding did occur: a hot sum needs more than 8 bits
    exact = ops.segment_sum_rows(rows, co.perm, co.seg, u, torch.float32)
    assert not torch.equal(exact.to(torch.bfloat16).float(), exact)


# --------------------------------------------------------------- table level

def make_table(optimizer, S, D=8):
    kw = dict(rows=V, dim=D, lr=0.1, seed=6, optimizer=optimizer, device=DEV)
    if S:
        return ShardedEmbeddingTable("t", num_shards=S, strategy="mod", **kw)
    return EmbeddingTable("t", **kw)


def dense(table):
    if isinstance(table, ShardedEmbeddingTable):
        return table.to_dense()
    return {"master": table.master, "shadow": table.shadow,
            "state": table.state, "step": table.step}


def assert_same_table(a, b):
    a, b = dense(a), dense(b)
    assert a["step"] == b["step"]
    assert torch.equal(a["master"], b["master"])
    assert torch.equal(a["shadow"], b["shadow"])
    assert sorted(a["state"]) == sorted(b["state"])
    for k in a["state"]:
        assert torch.equal(a["state"][k], b["state"][k]), k


@pytest.mark.parametrize("S", [0, 3], ids=["unsharded", "sharded3"])
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_table_fed_coalesced_pushes_equals_raw(optimizer, S):
    """Three pushes of 40 positions over 12 rows: (uniq[:u], per-id sums)
    leaves master, state, shadow and step as the raw (ids, grads) does."""
    raw, co_t = make_table(optimizer, S), make_table(optimizer, S)
    master0 = dense(raw)["master"].clone()
    gen = torch.Generator().manual_seed(600)
    for _ in range(3):
        ids = torch.tensor(proc.ROWS)[torch.randint(0, 12, (40,),
                                                    generator=gen)].to(DEV)
        g = (torch.randint(-4, 5, (40, 8), generator=gen).float() / 16).to(DEV)
        raw.push(ids, g.to(torch.bfloat16))
        co = ops.coalesce_ids(ids)
        u = int(co.count)
        assert u < 40
        co_t.push(co.uniq[:u], ops.segment_sum_rows(g, co.perm, co.seg, u,
                                                    torch.bfloat16))
    assert_same_table(co_t, raw)
    assert dense(raw)["step"] == 3
    assert not torch.equal(dense(raw)["master"], master0)


@pytest.mark.parametrize("S", [0, 3], ids=["unsharded", "sharded3"])
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_table_fed_hot_coalesced_push_equals_cpu_reference(optimizer, S):
    """The hot case: a table fed the GPU's (uniq, summed bf16 rows) ends
    equal to one fed the CPU reference's."""
    ids, rows, co = hot_case("one", 8)
    u = int(co.count)
    want_t, got_t = make_table(optimizer, S), make_table(optimizer, S)
    want_t.push(co.uniq[:u].to(DEV), ops.segment_sum_rows(
        rows, co.perm, co.seg, u, torch.bfloat16).to(DEV))
    g = ops.coalesce_ids(ids.to(DEV))
    got_t.push(g.uniq[:u], ops.segment_sum_rows(rows.to(DEV), g.perm, g.seg,
                                                u, torch.bfloat16))
    assert_same_table(got_t, want_t)


# ---------------------------------------------------------------- end to end

@pytest.mark.timeout(400)
@pytest.mark.parametrize("world", [2, 3], ids=["unsharded_adagrad",
                                               "mod_2ps_adam"])
def test_coalesced_protocol_on_gpu(world, tmp_path):
    """PS rank(s) + 1 worker, all on cuda:0, over gloo: the helper's script
    once with coalesce on. Each process has its own timeout; nothing is
    started after the ranks, and a rank that exits nonzero fails the test
    before the local comparison runs."""
    pulls = str(tmp_path / "pulls.pt")
    sums, seen = cpu_test.run_world(world, pulls, True, device=DEV,
                                    timeout=120)
    assert sorted(sums) == ["T/%d" % s for s in range(world - 1)]
    cpu_test.check_against_local(world, sums, pulls, device=DEV)
    cpu_test.check_seen(world, seen, True)
