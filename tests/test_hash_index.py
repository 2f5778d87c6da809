"""The key index of hashed embedding tables on the CPU: ops.HashIndex and
hash_find / hash_find_or_insert / hash_rebuild (a dict plus tensors — the
reference the HIP index of csrc/hash.hip must equal integer for integer)
against an independent naive dict loop written here, and the row
initialiser ops.hash_init_rows.

A SCRIPT is a capacity and a list of steps ("insert", keys), ("find",
keys), ("reserve", capacity), ("rebuild",); ``run_script`` plays it on a
device and returns everything observable. test_hash_gpu.py plays the same
scripts on the GPU."""

import functools

import pytest
import torch

from tfmesos_amd import ops

I64_MAX = 2 ** 63 - 1
EMPTY = ops.HASH_EMPTY
SPECIAL = [I64_MAX, 0, -1, -(2 ** 40) - 7, 2 ** 40 + 3]
SIZES = [0, 1, 63, 64, 65, 257, 1000]
KINDS = ["distinct", "equal", "pool", "sentinel"]


@functools.lru_cache(maxsize=None)
def pool97():
    """97 distinct keys: the five special ones and 92 random int64."""
    gen = torch.Generator().manual_seed(97)
    rest = torch.randint(-2 ** 62, 2 ** 62, (92,), generator=gen)
    pool = torch.cat([torch.tensor(SPECIAL), rest])
    assert len(set(pool.tolist())) == 97
    return pool


@functools.lru_cache(maxsize=None)
def keys_case(n, kind):
    gen = torch.Generator().manual_seed(1000 + n)
    if kind == "distinct":      # both signs, far apart
        return (torch.randperm(n, generator=gen) - n // 2) * 1000003 + 17
    if kind == "equal":
        return torch.full((n,), -11, dtype=torch.int64)
    keys = pool97()[torch.randint(0, 97, (n,), generator=gen)]
    if kind == "sentinel":      # every third position is the reserved key
        keys = keys.clone()
        keys[::3] = EMPTY
    return keys


def size_script(n, kind):
    """The request, the same request again (all hits) and a lookup that
    mixes its keys with absent ones. Capacity 1024 holds every case."""
    keys = keys_case(n, kind)
    probe = torch.cat([keys, torch.tensor([5, EMPTY, 123456789]), keys[:7]])
    return 1024, [("insert", keys), ("insert", keys), ("find", probe)]


def duplicate_script():
    """A new key at positions 3 and 200 — different waves and, with 257
    positions, more than one block."""
    keys = keys_case(257, "distinct").clone()
    keys[200] = keys[3]
    return 512, [("insert", keys), ("find", keys)]


def mixed_script():
    """Hits and misses in one request: 40 known keys, then a request that
    interleaves 30 of them with 50 new ones (some twice)."""
    k = keys_case(257, "distinct")
    known, new = k[:40], k[100:150]
    gen = torch.Generator().manual_seed(5)
    req = torch.cat([known[:30], new, new[:10]])
    req = req[torch.randperm(req.numel(), generator=gen)]
    return 128, [("insert", known), ("insert", req), ("find", k)]


def overflow_script():
    """Capacity 8, 12 distinct keys (one repeated behind the end); room
    after reserve(16); rebuild keeps every row."""
    k = torch.tensor([50, -3, I64_MAX, 7, 0, 2 ** 40 + 3, -1, 99, 1000, 1001,
                      1002, 1003])
    twice = torch.cat([k, k[9:10]])
    return 8, [("insert", k), ("find", k), ("insert", twice),
               ("reserve", 16), ("find", k), ("insert", k), ("rebuild",),
               ("find", k)]


def run_script(script, device="cpu"):
    """Play a script on ``device``: ([result per step], final). An insert
    step records (rows, is_new, row_keys[:size], size, dropped), the others
    rows or None."""
    capacity, steps = script
    index = ops.HashIndex(capacity, device)
    out = []
    for step in steps:
        if step[0] == "insert":
            rows, is_new = ops.hash_find_or_insert(index, step[1].to(device))
            assert rows.dtype == torch.int64 and is_new.dtype == torch.bool
            assert rows.device.type == index.device.type
            size = int(index.size)
            out.append((rows.cpu(), is_new.cpu(),
                        index.row_keys[:size].cpu().clone(), size,
                        int(index.dropped)))
        elif step[0] == "find":
            out.append(ops.hash_find(index, step[1].to(device)).cpu())
        elif step[0] == "reserve":
            index.reserve(step[1])
            out.append(None)
        else:
            ops.hash_rebuild(index)
            out.append(None)
    size = int(index.size)
    return out, (index.row_keys[:size].cpu().clone(), size,
                 int(index.dropped), index.capacity)


def run_naive(script):
    """The contract, spelled out with a dict and lists only."""
    capacity, steps = script
    table, row_keys, dropped = {}, [], 0
    out = []
    for step in steps:
        if step[0] == "insert":
            rows, is_new, lost = [], [], set()
            for k in step[1].tolist():
                fresh = False
                if k == EMPTY:
                    r = -1
                elif k in table:
                    r = table[k]
                elif len(row_keys) < capacity:
                    r = table[k] = len(row_keys)
                    row_keys.append(k)
                    fresh = True
                else:
                    r = -1
                    lost.add(k)
                rows.append(r)
                is_new.append(fresh)
            dropped += len(lost)
            out.append((torch.tensor(rows, dtype=torch.int64),
                        torch.tensor(is_new, dtype=torch.bool),
                        torch.tensor(row_keys, dtype=torch.int64),
                        len(row_keys), dropped))
        elif step[0] == "find":
            out.append(torch.tensor(
                [-1 if k == EMPTY else table.get(k, -1)
                 for k in step[1].tolist()], dtype=torch.int64))
        elif step[0] == "reserve":
            capacity = step[1]
            out.append(None)
        else:
            out.append(None)
    return out, (torch.tensor(row_keys, dtype=torch.int64), len(row_keys),
                 dropped, capacity)


def assert_same_run(got, want):
    (g_steps, g_final), (w_steps, w_final) = got, want
    assert len(g_steps) == len(w_steps)
    for a, b in zip(g_steps + [g_final], w_steps + [w_final]):
        if b is None:
            assert a is None
        elif isinstance(b, tuple):
            assert len(a) == len(b)
            for x, y in zip(a, b):
                if isinstance(y, torch.Tensor):
                    assert x.dtype == y.dtype and torch.equal(x, y)
                else:
                    assert x == y
        else:
            assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_request_sizes_and_key_kinds(n, kind):
    script = size_script(n, kind)
    got = run_script(script)
    assert_same_run(got, run_naive(script))
    (first, second, _), (row_keys, size, dropped, _) = got
    distinct = set(keys_case(n, kind).tolist()) - {EMPTY}
    assert size == len(distinct) and dropped == 0
    assert set(row_keys.tolist()) == distinct
    assert int(first[1].sum()) == size and not second[1].any()
    assert torch.equal(first[0], second[0])
    if kind == "sentinel" and n:
        assert (first[0][::3] == -1).all() and not first[1][::3].any()


def test_special_keys_are_ordinary_keys():
    index = ops.HashIndex(8)
    rows, is_new = ops.hash_find_or_insert(index, torch.tensor(SPECIAL))
    assert rows.tolist() == [0, 1, 2, 3, 4] and is_new.all()
    assert index.row_keys[:5].tolist() == SPECIAL
    assert ops.hash_find(index, torch.tensor(
        [-1, I64_MAX, EMPTY, 1])).tolist() == [2, 0, -1, -1]


def test_new_key_duplicated_across_waves_gets_one_row():
    script = duplicate_script()
    got = run_script(script)
    assert_same_run(got, run_naive(script))
    rows, is_new, row_keys, size, dropped = got[0][0]
    assert rows[3] == rows[200] == 3
    assert is_new[3] and not is_new[200]
    assert size == 256 and int(is_new.sum()) == 256 and dropped == 0
    # ranks skip the duplicate: position 201 owns row 200
    assert rows[199] == 199 and rows[201] == 200 and rows[256] == 255


def test_mixed_hits_and_misses():
    script = mixed_script()
    got = run_script(script)
    assert_same_run(got, run_naive(script))
    rows, is_new, _, size, dropped = got[0][1]
    assert size == 90 and dropped == 0 and int(is_new.sum()) == 50
    assert int((rows < 40).sum()) == 30 and int((rows >= 40).sum()) == 60
    found = got[0][2]
    assert int((found >= 0).sum()) == 90 and int((found < 0).sum()) == 167


def test_overflow_growth_and_rebuild():
    script = overflow_script()
    got = run_script(script)
    assert_same_run(got, run_naive(script))
    steps, (row_keys, size, dropped, capacity) = got
    rows, is_new, _, size1, dropped1 = steps[0]
    assert rows.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, -1, -1, -1, -1]
    assert is_new.tolist() == [True] * 8 + [False] * 4
    assert (size1, dropped1) == (8, 4)
    assert steps[1].tolist() == rows.tolist()
    # a full table: the four keys are dropped again, the repeat counts once
    rows2, is_new2, _, size2, dropped2 = steps[2]
    assert rows2.tolist() == rows.tolist() + [-1]
    assert not is_new2.any() and (size2, dropped2) == (8, 8)
    assert steps[4].tolist() == rows.tolist()       # reserve moved nothing
    rows3, is_new3, keys3, size3, dropped3 = steps[5]
    assert rows3.tolist() == list(range(12))
    assert is_new3.tolist() == [False] * 8 + [True] * 4
    assert (size3, dropped3) == (12, 8)
    assert steps[7].tolist() == list(range(12))     # after the rebuild
    assert (size, dropped, capacity) == (12, 8, 16)
    assert row_keys.tolist() == script[1][0][1].tolist()


def test_input_checks():
    index = ops.HashIndex(4)
    for bad in (torch.zeros(3, dtype=torch.int32),
                torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError):
            ops.hash_find(index, bad)
        with pytest.raises(ValueError):
            ops.hash_find_or_insert(index, bad)
    with pytest.raises(ValueError):
        ops.HashIndex(0)
    with pytest.raises(ValueError):
        index.reserve(2)
    assert ops.hash_slots(1) == 64 and ops.hash_slots(64) == 128
    assert ops.hash_slots(65) == 256
    home = ops.hash_home(torch.tensor(SPECIAL), 128)
    assert home.dtype == torch.int64 and ((home >= 0) & (home < 128)).all()


# ------------------------------------------------------------- initialiser

def test_init_rows_is_a_pure_function_of_seed_key_and_column():
    keys = pool97()
    full = ops.hash_init_rows(keys, 24, seed=5)
    assert full.dtype == torch.float32 and full.shape == (97, 24)
    gen = torch.Generator().manual_seed(1)
    perm = torch.randperm(97, generator=gen)
    assert torch.equal(ops.hash_init_rows(keys[perm], 24, seed=5), full[perm])
    parts = [ops.hash_init_rows(keys[a:b], 24, seed=5)
             for a, b in ((0, 1), (1, 64), (64, 97))]
    assert torch.equal(torch.cat(parts), full)
    # the column's value does not depend on the row's width...
    wide = ops.hash_init_rows(keys, 96, seed=5)
    assert torch.equal(wide[:, :24] * 2, full)      # ...only on the scale
    assert not torch.equal(ops.hash_init_rows(keys, 24, seed=6), full)
    # distinct keys, distinct rows
    assert len(set(map(tuple, full.tolist()))) == 97


@pytest.mark.parametrize("dim", [7, 8, 130, 320])
def test_init_rows_range_and_spread(dim):
    rows = ops.hash_init_rows(pool97(), dim, seed=0)
    assert float(rows.min()) >= 0.0
    assert float(rows.max()) < dim ** -0.5
    mean = float(rows.mean()) * dim ** 0.5
    assert 0.45 < mean < 0.55       # uniform: 0.5 +- 0.29 / sqrt(97 * dim)


def test_init_rows_of_a_shard_are_the_global_keys_rows():
    """key_mul / key_add: local key l of shard s of S stands for l * S + s."""
    glob = torch.tensor([0, 1, 2, 3, 4, 5, 2 ** 62 - 1, 2 ** 40 + 3])
    want = ops.hash_init_rows(glob, 8, seed=3)
    for s in range(3):
        mine = glob % 3 == s
        got = ops.hash_init_rows(glob[mine] // 3, 8, seed=3, key_mul=3,
                                 key_add=s)
        assert torch.equal(got, want[mine])
