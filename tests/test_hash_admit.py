"""Feature admission of hashed embedding tables on the CPU: the count-min
sketch ops.HashAdmission and ops.hash_find_or_admit (a dict plus a numpy
sketch — the reference the HIP kernels of csrc/hash.hip must equal integer
for integer) against a naive dict of EXACT per-key counts written here, the
serving ops that read an absent key's initial row (ops.hash_gather_init,
ops.hash_embedding_bag), and HashedEmbeddingTable(admit_after=).

An ADMIT SCRIPT is (capacity, width, admit_after, [requests], preset) with
preset None or [(sketch row, cell, value)] written into the counters first;
``run_script`` plays it on a device and returns everything observable after
every request. test_hash_admit_gpu.py plays the same scripts on the GPU.

Exact counts are the right oracle only where the sketch cannot overestimate:
at width 1024 every key of each pool used here owns at least one cell that
no other key of the pool shares, so min over its four cells = its own count.
``assert_no_overestimate`` checks that before a script relies on it."""

import functools

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import HashedEmbeddingTable, _ShardRoute

import test_hash_index as index_test
import test_hashed_table as table_test

EMPTY = ops.HASH_EMPTY
CAP = 2 ** 30
WIDTH = 1024
SIZES = index_test.SIZES
DIM, SEED = table_test.DIM, table_test.SEED


def pools():
    return {"pool97": index_test.pool97(),
            "distinct257": index_test.keys_case(257, "distinct")}


def assert_no_overestimate(pool, width):
    """Every key has a cell that no other key of the pool counts in."""
    cells = ops.hash_admit_cells(pool, width)
    assert cells.shape == (4, pool.numel()) and cells.dtype == torch.int64
    assert ((cells >= 0) & (cells < width)).all()
    own = torch.zeros(pool.numel(), dtype=torch.bool)
    for j in range(4):
        own |= torch.bincount(cells[j], minlength=width)[cells[j]] == 1
    assert own.all()


# ----------------------------------------------------------------- scripts

@functools.lru_cache(maxsize=None)
def size_script(name, n, admit_after):
    """Five requests of n positions drawn with repeats from one pool, every
    fifth position of the odd requests HASH_EMPTY, then the first request
    again: keys are counted, admitted at different requests, and hit."""
    pool = pools()[name]
    gen = torch.Generator().manual_seed(31 * n + admit_after)
    reqs = []
    for t in range(5):
        keys = pool[torch.randint(0, pool.numel(), (n,), generator=gen)]
        if t % 2:
            keys = keys.clone()
            keys[::5] = EMPTY
        reqs.append(keys)
    return 512, WIDTH, admit_after, reqs + [reqs[0]], None


def duplicate_script():
    """One absent key at positions 3, 200 and 256 (other waves, another
    block) of one request: counted once, so admit_after=2 admits it at the
    second request, where is_new marks position 3 only."""
    keys = index_test.keys_case(257, "distinct").clone()
    keys[200] = keys[256] = keys[3]
    return 512, WIDTH, 2, [keys, keys, keys], None


def full_script():
    """Capacity 8 and 12 keys, admit_after=2: the second request admits all
    twelve, eight get rows and four go to dropped (not filtered); they are
    dropped again by the third."""
    keys = index_test.pool97()[:12]
    return 8, WIDTH, 2, [keys, torch.cat([keys, keys[9:10]]), keys], None


def covering_keys(key, width):
    """For j = 0..3 the smallest key in 1..9999 that shares sketch cell j
    with ``key``."""
    cand = torch.arange(1, 10000)
    cand = cand[cand != key]
    mine = ops.hash_admit_cells(torch.tensor([key]), width)[:, 0]
    cells = ops.hash_admit_cells(cand, width)
    return torch.stack([cand[cells[j] == mine[j]][0] for j in range(4)])


def early_script():
    """Width 64: four keys that cover the four cells of key 0 are pushed
    once, so the FIRST push of key 0 already finds estimate 2."""
    cover = covering_keys(0, 64)
    return 64, 64, 2, [cover, torch.tensor([0]), torch.tensor([0])], None


def saturation_script():
    """The four cells of key 5 start at CAP - 1, CAP, CAP - 1, CAP (the
    cells of keys 6 and 7 at 0): a request with 5 (three times), 6 and 7."""
    cells = ops.hash_admit_cells(torch.tensor([5]), 64)[:, 0].tolist()
    preset = [(j, c, CAP - 1 + j % 2) for j, c in enumerate(cells)]
    return 64, 64, CAP, [torch.tensor([5, 6, 5, 7, 5])], preset


def contention_script():
    """1000 positions of one key: every lane finds it absent, one counts."""
    keys = index_test.keys_case(1000, "equal")
    return 16, 64, 2, [keys, keys, keys], None


def run_script(script, device="cpu"):
    """Per request: (rows, is_new, row_keys[:size], size, dropped, filtered,
    counters)."""
    capacity, width, admit_after, reqs, preset = script
    index = ops.HashIndex(capacity, device)
    sketch = ops.HashAdmission(width, device)
    for j, c, v in preset or []:
        sketch.counters[j, c] = v
    out = []
    for keys in reqs:
        rows, is_new = ops.hash_find_or_admit(index, sketch, keys.to(device),
                                              admit_after)
        assert rows.dtype == torch.int64 and is_new.dtype == torch.bool
        assert rows.device.type == index.device.type
        size = int(index.size)
        out.append((rows.cpu(), is_new.cpu(),
                    index.row_keys[:size].cpu().clone(), size,
                    int(index.dropped), int(sketch.filtered),
                    sketch.counters.cpu().clone()))
    return out


def run_exact(script):
    """The contract with exact counts: dicts and lists only. Per request
    (rows, is_new, row_keys, size, dropped, filtered) — no counters."""
    capacity, _, admit_after, reqs, preset = script
    assert preset is None
    table, counts, row_keys = {}, {}, []
    dropped = filtered = 0
    out = []
    for keys in reqs:
        keys = keys.tolist()
        first = {}
        for i, k in enumerate(keys):
            if k != EMPTY and k not in table and k not in first:
                first[k] = i
        for k in first:
            counts[k] = counts.get(k, 0) + 1
        is_new = [False] * len(keys)
        for k, i in first.items():
            if counts[k] < admit_after:
                filtered += 1
            elif len(row_keys) < capacity:
                table[k] = len(row_keys)
                row_keys.append(k)
                is_new[i] = True
            else:
                dropped += 1
        rows = [-1 if k == EMPTY else table.get(k, -1) for k in keys]
        out.append((torch.tensor(rows, dtype=torch.int64),
                    torch.tensor(is_new, dtype=torch.bool),
                    torch.tensor(row_keys, dtype=torch.int64),
                    len(row_keys), dropped, filtered))
    return out


def assert_same(got, want):
    """Request by request; ``want`` may lack the counters."""
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for x, y in zip(a, b):
            if isinstance(y, torch.Tensor):
                assert x.dtype == y.dtype and torch.equal(x, y)
            else:
                assert x == y


# ------------------------------------------------------------- index level

@pytest.mark.parametrize("name", sorted(pools()))
def test_pools_cannot_overestimate_at_width_1024(name):
    assert_no_overestimate(pools()[name], WIDTH)


@pytest.mark.parametrize("admit_after", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(pools()))
def test_request_sizes_equal_exact_counts(name, n, admit_after):
    script = size_script(name, n, admit_after)
    got = run_script(script)
    assert_same(got, run_exact(script))
    rows, is_new, row_keys, size, dropped, filtered, counters = got[-1]
    assert dropped == 0 and int(counters.min()) >= 0
    assert len(set(row_keys.tolist())) == size
    if admit_after == 1:    # plain find_or_insert: nothing is ever filtered
        assert filtered == 0
        distinct = set(torch.cat(script[3]).tolist()) - {EMPTY}
        assert set(row_keys.tolist()) == distinct
    elif n >= 63:
        assert filtered > 0 and size > 0


def test_admit_after_one_is_find_or_insert():
    for n in SIZES:
        _, _, _, reqs, _ = size_script("pool97", n, 1)
        plain, index = ops.HashIndex(512), ops.HashIndex(512)
        sketch = ops.HashAdmission(WIDTH)
        for keys in reqs:
            want = ops.hash_find_or_insert(plain, keys)
            got = ops.hash_find_or_admit(index, sketch, keys, 1)
            assert torch.equal(got[0], want[0])
            assert torch.equal(got[1], want[1])
        assert torch.equal(index.row_keys, plain.row_keys)


def test_duplicates_in_one_request_count_once():
    script = duplicate_script()
    got = run_script(script)
    assert_same(got, run_exact(script))
    rows1, is_new1, _, size1, _, filtered1, counters1 = got[0]
    assert (rows1 == -1).all() and not is_new1.any() and size1 == 0
    assert filtered1 == 255 and int(counters1.sum()) == 4 * 255
    rows2, is_new2, _, size2, dropped2, filtered2, _ = got[1]
    assert size2 == 255 and dropped2 == 0 and filtered2 == 255
    assert rows2[3] == rows2[200] == rows2[256] == 3
    assert is_new2[3] and not is_new2[200] and not is_new2[256]
    assert int(is_new2.sum()) == 255 and rows2[255] == 254
    assert torch.equal(got[2][0], rows2) and not got[2][1].any()
    assert torch.equal(got[2][6], got[1][6])    # hits do not count


def test_full_table_drops_admitted_keys():
    script = full_script()
    got = run_script(script)
    assert_same(got, run_exact(script))
    assert got[0][3:6] == (0, 0, 12)
    rows, is_new, _, size, dropped, filtered, _ = got[1]
    assert rows.tolist() == list(range(8)) + [-1] * 5
    assert is_new.tolist() == [True] * 8 + [False] * 5
    assert (size, dropped, filtered) == (8, 4, 12)
    assert got[2][3:6] == (8, 8, 12)


def test_early_admission_through_collisions():
    script = early_script()
    cover = script[3][0]
    assert cover.tolist() == [71, 74, 61, 57]   # what the formula gives
    got = run_script(script)
    rows, is_new, row_keys, size, _, filtered, counters = got[1]
    mine = ops.hash_admit_cells(torch.tensor([0]), 64)[:, 0]
    assert counters[torch.arange(4), mine].tolist() == [2, 2, 2, 2]
    assert rows.tolist() == [0] and is_new.tolist() == [True]
    assert row_keys.tolist() == [0] and size == 1
    assert filtered == 4        # the four covering keys, nothing more
    assert got[2][0].tolist() == [0] and not got[2][1].any()
    # exact counts would have made key 0 wait for its second push
    assert run_exact(script)[1][3] == 0


def test_counters_saturate():
    script = saturation_script()
    (rows, is_new, row_keys, size, dropped, filtered, counters), = \
        run_script(script)
    cells = ops.hash_admit_cells(torch.tensor([5, 6, 7]), 64)
    want = torch.zeros(4, 64, dtype=torch.int64)
    for j, c, v in script[4]:
        want[j, c] = v
    for j in range(4):
        want[j].index_add_(0, cells[j], torch.ones(3, dtype=torch.int64))
    want.clamp_(max=CAP)
    assert torch.equal(counters, want.to(torch.int32))
    assert counters[torch.arange(4), cells[:, 0]].tolist() == [CAP] * 4
    # key 5 reached the estimate CAP = admit_after; 6 and 7 did not
    assert rows.tolist() == [0, -1, 0, -1, 0]
    assert is_new.tolist() == [True, False, False, False, False]
    assert (size, dropped, filtered) == (1, 0, 2)
    assert int(counters.max()) == CAP


def test_one_key_a_thousand_times():
    got = run_script(contention_script())
    assert_same(got, run_exact(contention_script()))
    assert got[0][3:6] == (0, 0, 1) and int(got[0][6].sum()) == 4
    rows, is_new = got[1][:2]
    assert (rows == 0).all() and is_new.tolist() == [True] + [False] * 999
    assert torch.equal(got[2][6], got[1][6]) and int(got[1][6].sum()) == 8


def test_decay_halves_the_counters():
    sketch = ops.HashAdmission(64)
    gen = torch.Generator().manual_seed(3)
    start = torch.randint(0, 1000, (4, 64), generator=gen).to(torch.int32)
    start[0, :3] = torch.tensor([CAP, CAP - 1, 1], dtype=torch.int32)
    sketch.counters.copy_(start)
    sketch.decay()
    assert torch.equal(sketch.counters, start // 2)
    assert sketch.counters[0, :3].tolist() == [CAP // 2, CAP // 2 - 1, 0]


def test_admission_input_checks():
    index, sketch = ops.HashIndex(4), ops.HashAdmission(64)
    keys = torch.tensor([1, 2])
    for bad in (0, CAP + 1):
        with pytest.raises(ValueError):
            ops.hash_find_or_admit(index, sketch, keys, bad)
    with pytest.raises(ValueError):
        ops.hash_find_or_admit(index, None, keys, 1)
    for width in (32, 96, 0):
        with pytest.raises(ValueError):
            ops.HashAdmission(width)
        with pytest.raises(ValueError):
            ops.hash_admit_cells(keys, width)
    assert sketch.counters.shape == (4, 64)
    assert sketch.counters.dtype == torch.int32
    assert sketch.filtered.dtype == torch.int64
    # not the index's home slot: another hash per sketch row
    pool = index_test.pool97()
    cells = ops.hash_admit_cells(pool, 128)
    for j in range(4):
        assert not torch.equal(cells[j], ops.hash_home(pool, 128))
        assert not torch.equal(cells[j], cells[(j + 1) % 4])


# ------------------------------------------------------------- serving ops

def dyadic(gen, *shape):
    return torch.randint(-32, 33, shape, generator=gen).float() / 16


def serving_case(D, device="cpu"):
    """An index that holds the first 60 keys of pool97 in a table of 64
    rows: (index, bf16 table, pool)."""
    gen = torch.Generator().manual_seed(100 + D)
    index = ops.HashIndex(64, device)
    pool = index_test.pool97().to(device)
    ops.hash_find_or_insert(index, pool[:60])
    table = dyadic(gen, 64, D).to(torch.bfloat16).to(device)
    return index, table, pool


def mixed_keys(pool, n, gen):
    """Hits, misses and HASH_EMPTY (every seventh position)."""
    pick = torch.randint(0, pool.numel(), (n,), generator=gen)
    keys = pool[pick.to(pool.device)].clone()
    keys[::7] = EMPTY
    return keys


@pytest.mark.parametrize("D", [7, 8])
def test_gather_init_reads_rows_initial_rows_and_zeros(D):
    index, table, pool = serving_case(D)
    gen = torch.Generator().manual_seed(D)
    keys = mixed_keys(pool, 257, gen)
    rows = ops.hash_find(index, keys)
    stamps = torch.full((64,), -1, dtype=torch.int64)
    got = ops.hash_gather_init(index, table, keys, SEED, 3, 2,
                               last_used=stamps, step=9)
    assert got.dtype == torch.bfloat16 and got.shape == (257, D)
    hit, gone = rows >= 0, keys == EMPTY
    miss = ~hit & ~gone
    assert hit.any() and miss.any() and gone.any()
    assert torch.equal(got[hit], table[rows[hit]])
    assert torch.equal(got[miss], ops.hash_init_rows(
        keys[miss], D, SEED, 3, 2).to(torch.bfloat16))
    assert not got[gone].any()
    # stamps for the hits only
    named = torch.zeros(64, dtype=torch.bool)
    named[rows[hit]] = True
    assert (stamps[named] == 9).all() and (stamps[~named] == -1).all()
    # without stamps, and on nothing
    assert torch.equal(ops.hash_gather_init(index, table, keys, SEED, 3, 2),
                       got)
    assert ops.hash_gather_init(index, table, keys[:0], SEED).shape == (0, D)
    assert torch.equal(ops.hash_gather(index, table, keys)[~miss], got[~miss])


def bag_offsets(lens):
    return torch.cat([torch.tensor([0]), torch.tensor(lens).cumsum(0)])


def extended_oracle(index, table, keys, offsets, weights, combiner, out_dtype,
                    init):
    """ops.embedding_bag over cat([table, bf16 initial rows of the absent
    keys]) with the ids remapped — built here from hash_find alone."""
    rows = ops.hash_find(index, keys)
    ids = rows.clone()
    if init is not None:
        miss = (rows < 0) & (keys != EMPTY)
        extra = ops.hash_init_rows(keys[miss].cpu(), table.shape[1],
                                   *init).to(torch.bfloat16).to(table.device)
        ids[miss] = table.shape[0] + torch.arange(
            int(miss.sum()), device=ids.device)
        table = torch.cat([table, extra])
    return ops.embedding_bag(table, ids, offsets, weights=weights,
                             combiner=combiner, out_dtype=out_dtype)


BAG_LENS = [0, 1, 3, 64, 65, 130, 0, 2]


@pytest.mark.parametrize("init", [None, (SEED, 1, 0), (SEED, 3, 2)],
                         ids=["no_init", "init", "init_shard"])
@pytest.mark.parametrize("D", [7, 8])
def test_hash_embedding_bag_equals_bag_over_extended_table(D, init):
    index, table, pool = serving_case(D)
    gen = torch.Generator().manual_seed(7 * D)
    offsets = bag_offsets(BAG_LENS)
    n = int(offsets[-1])
    keys = mixed_keys(pool, n, gen)
    weights = torch.randint(1, 5, (n,), generator=gen).float() / 4
    for w, combiner, out_dtype in ((None, "sum", None), (weights, "sum", None),
                                   (weights, "mean", torch.float32),
                                   (None, "mean", None)):
        got = ops.hash_embedding_bag(index, table, keys, offsets, w, combiner,
                                     out_dtype, init=init)
        want = extended_oracle(index, table, keys, offsets, w, combiner,
                               out_dtype, init)
        assert got.dtype == (out_dtype or torch.bfloat16)
        assert got.shape == (len(BAG_LENS), D) and torch.equal(got, want)
        assert not got[0].any() and not got[6].any()    # empty bags
    # an initial row does contribute
    a = ops.hash_embedding_bag(index, table, keys, offsets, init=init)
    b = ops.hash_embedding_bag(index, table, keys, offsets)
    assert torch.equal(a, b) == (init is None)
    stamps = torch.full((64,), -1, dtype=torch.int64)
    ops.hash_embedding_bag(index, table, keys, offsets, init=init,
                           last_used=stamps, step=4)
    rows = ops.hash_find(index, keys)
    named = torch.zeros(64, dtype=torch.bool)
    named[rows[rows >= 0]] = True
    assert (stamps[named] == 4).all() and (stamps[~named] == -1).all()


def test_serving_op_input_checks():
    index, table, pool = serving_case(8)
    offsets = torch.tensor([0, 2])
    with pytest.raises(ValueError):
        ops.hash_gather_init(index, table.float(), pool[:2], SEED)
    with pytest.raises(ValueError):
        ops.hash_embedding_bag(index, table.float(), pool[:2], offsets)
    with pytest.raises(ValueError):
        ops.hash_embedding_bag(index, table, pool[:2], offsets,
                               combiner="max")
    with pytest.raises(ValueError):
        ops.hash_embedding_bag(index, table, pool[:2], offsets,
                               out_dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.hash_gather_init(index, table, pool[:2], SEED,
                             last_used=torch.zeros(64, dtype=torch.int32))


# -------------------------------------------------------------- table level

def by_key(table):
    """{key: (master row, shadow row, state rows...)} of the live rows."""
    n = table.stats()["size"]
    keys = table.index.row_keys[:n].tolist()
    cols = [table.master, table.shadow] + [table.state[k]
                                           for k in sorted(table.state)]
    return {k: tuple(c[r].cpu() for c in cols) for r, k in enumerate(keys)}


def assert_equal_by_key(a, b):
    ka, kb = by_key(a), by_key(b)
    assert sorted(ka) == sorted(kb) and a.step == b.step
    for k in ka:
        for x, y in zip(ka[k], kb[k]):
            assert x.dtype == y.dtype and torch.equal(x, y)


def check_admit_one_equals_plain(optimizer, hparams, device="cpu"):
    """Pulls of a plain table insert, pulls of an admitting one serve the
    initial row unstored: the same values, other row numbers."""
    reqs = table_test.script()
    plain = table_test.make_table(optimizer, hparams, device)
    admit = table_test.make_table(optimizer, hparams, device, admit_after=1)
    want = table_test.play(plain, reqs, device)
    got = table_test.play(admit, reqs, device)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # the plain table also holds the keys that were only ever pulled, still
    # at their initial rows with zero state; every pushed key is equal
    ka, kb = by_key(admit), by_key(plain)
    assert admit.step == plain.step and set(ka) < set(kb)
    for k, cols in kb.items():
        if k in ka:
            for x, y in zip(ka[k], cols):
                assert x.dtype == y.dtype and torch.equal(x, y)
        else:
            init = ops.hash_init_rows(torch.tensor([k]), DIM, SEED)[0]
            assert torch.equal(cols[0], init)
            assert torch.equal(cols[1], init.to(torch.bfloat16))
            assert not any(c.any() for c in cols[2:])
    assert admit.stats() == {"size": len(ka), "dropped": 0, "capacity": 128,
                             "filtered": 0}
    assert sorted(plain.stats()) == ["capacity", "dropped", "size"]


@pytest.mark.parametrize("optimizer,hparams", table_test.OPTIMIZERS,
                         ids=table_test.OPT_IDS)
def test_admit_after_one_equals_plain_table(optimizer, hparams):
    check_admit_one_equals_plain(optimizer, hparams)


def check_admit_after_three(device="cpu"):
    pool = index_test.pool97().to(device)
    keys = torch.cat([pool[:10], pool[:4]])     # duplicates count once
    gen = torch.Generator().manual_seed(8)
    g = (torch.randint(-8, 9, (14, DIM), generator=gen).float() / 16).to(
        torch.bfloat16).to(device)
    table = table_test.make_table("adagrad", {}, device, admit_after=3,
                                  track_use=True)
    init = ops.hash_init_rows(keys.cpu(), DIM, SEED).to(torch.bfloat16)
    offsets = torch.tensor([0, 5, 14], device=device)
    for t in (1, 2):
        table.push(keys, g)
        assert table.step == t
        assert table.stats() == {"size": 0, "dropped": 0, "capacity": 128,
                                 "evicted": 0, "filtered": 10 * t}
        assert torch.equal(table.pull(keys).cpu(), init)
        pooled = table.pull_pooled(keys, offsets, None, "sum", torch.float32)
        want = torch.stack([init[:5].float().sum(0), init[5:].float().sum(0)])
        assert torch.allclose(pooled.cpu(), want, rtol=0, atol=1e-6)
        assert not table.master.any() and table.stats()["size"] == 0
    table.push(keys, g)
    # the third push: admitted, initialised, and this push's gradient applied
    fresh = table_test.make_table("adagrad", {}, device)
    fresh.step = 2
    fresh.push(keys, g)
    assert table.stats() == {"size": 10, "dropped": 0, "capacity": 128,
                             "evicted": 0, "filtered": 20}
    assert_equal_by_key(table, fresh)
    assert torch.equal(table.pull(keys), fresh.pull(keys))
    assert not torch.equal(table.pull(keys).cpu(), init)
    assert (table.last_used[:10] == 3).all()
    # a pull never counts: a key that was only ever pulled stays out
    for _ in range(4):
        table.pull(pool[20:30])
        table.pull_pooled(pool[20:30], torch.tensor([0, 10], device=device))
    table.push(pool[20:30], g[:10])
    assert table.stats()["size"] == 10 and table.stats()["filtered"] == 30


def test_admit_after_three_script():
    check_admit_after_three()


def test_serving_table_with_admission_reads_zeros():
    table = table_test.make_table("adam", {}, insert_on_pull=False,
                                  admit_after=2)
    pool = index_test.pool97()
    g = torch.ones(5, DIM, dtype=torch.bfloat16)
    table.push(pool[:5], g)
    assert not table.pull(pool[:5]).any()
    assert not table.pull_pooled(pool[:5], torch.tensor([0, 5])).any()
    table.push(pool[:5], g)
    assert table.pull(pool[:10])[:5].any()
    assert not table.pull(pool[:10])[5:].any()
    assert table.stats() == {"size": 5, "dropped": 0, "capacity": 128,
                             "filtered": 5}


def test_decay_every_and_eviction_interplay():
    pool = index_test.pool97()
    g = torch.ones(4, DIM, dtype=torch.bfloat16)
    table = table_test.make_table("sgd", {}, admit_after=2, admit_width=64,
                                  admit_decay_every=3, track_use=True)
    assert table.sketch.width == 64
    table.push(pool[:4], g)
    table.push(pool[:4], g)
    assert table.stats()["size"] == 4
    before = table.sketch.counters.clone()
    assert int(before.sum()) == 4 * 4 * 2 and int(before.max()) >= 2
    table.push(pool[:4], g)                     # step 3: hits, then decay
    assert torch.equal(table.sketch.counters, before // 2)
    # an evicted key must be admitted again; its counters were not cleared
    table.remove(pool[:2])
    assert table.stats()["size"] == 2
    init = ops.hash_init_rows(pool[:2], DIM, SEED).to(torch.bfloat16)
    assert torch.equal(table.pull(pool[:2]), init)
    table.push(pool[:2], g[:2])                 # estimate 1 + 1 = 2: back
    assert table.stats()["size"] == 4
    table.reserve(256)
    assert table.sketch.width == 64             # reserve leaves the sketch


def test_checkpoint_round_trips_the_sketch():
    pool = index_test.pool97()
    gen = torch.Generator().manual_seed(12)
    kw = dict(admit_after=3, admit_width=256)
    a = table_test.make_table("adagrad", {}, **kw)
    for _ in range(4):
        keys = pool[torch.randint(0, 40, (30,), generator=gen)]
        a.push(keys, torch.ones(30, DIM, dtype=torch.bfloat16) / 8)
    sd = a.state_dict()
    assert torch.equal(sd["admit_counters"], a.sketch.counters)
    assert "admit_counters" not in table_test.make_table(
        "adagrad", {}).state_dict()
    b = HashedEmbeddingTable("b", DIM, 200, lr=0.05, seed=1,
                             optimizer="adagrad", **kw)
    b.load_state_dict(sd)
    assert torch.equal(b.sketch.counters, a.sketch.counters)
    for _ in range(3):
        keys = pool[torch.randint(0, 60, (30,), generator=gen)]
        g = torch.ones(30, DIM, dtype=torch.bfloat16) / 4
        a.push(keys, g)
        b.push(keys, g)
    assert_equal_by_key(a, b)
    assert torch.equal(a.sketch.counters, b.sketch.counters)
    assert 0 < a.stats()["size"] < 60
    # a checkpoint without counters: a zero sketch; another width: an error
    old = {k: v for k, v in sd.items() if k != "admit_counters"}
    b.load_state_dict(old)
    assert not b.sketch.counters.any() and b.stats()["filtered"] == 0
    with pytest.raises(ValueError):
        table_test.make_table("adagrad", {}, admit_after=3,
                              admit_width=128).load_state_dict(sd)
    # a plain table loads it as well
    table_test.make_table("adagrad", {}).load_state_dict(sd)


def test_shards_equal_the_unsharded_table_by_key():
    """Width 1024 and 60 keys per shard at the most: the estimates are the
    exact counts on both sides (asserted), so a shard's sketch over its
    local keys decides as the unsharded one over the global keys."""
    S = 3
    gen = torch.Generator().manual_seed(44)
    pool = torch.randint(0, ops.HASH_KEY_SPACE, (60,), generator=gen)
    assert_no_overestimate(pool, WIDTH)
    for s in range(S):
        assert_no_overestimate(pool[pool % S == s] // S, WIDTH)
    kw = dict(lr=0.05, seed=SEED, optimizer="adam", admit_after=2,
              admit_width=WIDTH)
    whole = HashedEmbeddingTable("t", DIM, 128, **kw)
    shards = [HashedEmbeddingTable.shard_of("t", DIM, s, S, 64, **kw)
              for s in range(S)]
    assert all(t.admit_after == 2 and t.sketch.width == WIDTH
               for t in shards)
    for t in range(5):
        keys = pool[torch.randint(0, 20 + 10 * t, (50,), generator=gen)]
        g = (torch.randint(-8, 9, (50, DIM), generator=gen).float() / 16).to(
            torch.bfloat16)
        route = _ShardRoute(keys, ops.HASH_KEY_SPACE, S, "mod")
        gs = route.to_slots(g)
        parts = torch.zeros(50, DIM, dtype=torch.bfloat16)
        for s, shard in enumerate(shards):
            parts[route.span(s)] = shard.pull(route.ids(s))
            shard.push(route.ids(s), gs[route.span(s)])
        assert torch.equal(route.to_request_order(parts), whole.pull(keys))
        whole.push(keys, g)
    want = by_key(whole)
    got = {}
    for s, shard in enumerate(shards):
        got.update({k * S + s: v for k, v in by_key(shard).items()})
    assert sorted(got) == sorted(want) and 0 < len(want) < 60
    for k in want:
        for x, y in zip(got[k], want[k]):
            assert torch.equal(x, y)
    assert sum(t.stats()["filtered"] for t in shards) == \
        whole.stats()["filtered"] > 0


def test_coalesced_and_uncoalesced_streams_end_identical():
    """What SparseWorkerClient(coalesce=True) sends: the distinct keys and
    their summed gradients. A request counts a key once either way."""
    pool = index_test.pool97()
    gen = torch.Generator().manual_seed(9)
    a = table_test.make_table("adagrad", {}, admit_after=2)
    b = table_test.make_table("adagrad", {}, admit_after=2)
    for t in range(6):
        keys = pool[torch.randint(0, 15 + 5 * t, (40,), generator=gen)]
        g = torch.randint(-4, 5, (40, DIM), generator=gen).float() / 16
        a.push(keys, g.to(torch.bfloat16))
        co = ops.coalesce_ids(keys)
        u = int(co.count)
        b.push(co.uniq[:u], ops.segment_sum_rows(g, co.perm, co.seg, u,
                                                 torch.bfloat16))
        assert torch.equal(a.pull(keys), b.pull(keys))
    assert_equal_by_key(a, b)
    assert a.stats() == b.stats() and a.stats()["filtered"] > 0
    assert torch.equal(a.sketch.counters, b.sketch.counters)


def test_table_argument_checks():
    for kw in (dict(admit_width=64), dict(admit_decay_every=2),
               dict(admit_after=0), dict(admit_after=CAP + 1),
               dict(admit_after=2, admit_decay_every=0),
               dict(admit_after=2, admit_width=100)):
        with pytest.raises(ValueError):
            table_test.make_table("sgd", {}, **kw)
    plain = table_test.make_table("sgd", {})
    assert plain.sketch is None and plain.admit_after is None
    assert table_test.make_table("sgd", {}, capacity=100,
                                 admit_after=1).sketch.width == 256
