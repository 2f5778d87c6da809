"""Eviction from hashed embedding tables on the CPU: ops.hash_touch,
ops.hash_compact (hole filling) and ops.hash_remove against a naive oracle
that works on Python lists and a dict, and HashedEmbeddingTable's use
stamps, remove / evict and the automatic idle policy against an oracle that
keeps a dict of keys over a dense EmbeddingTable and never reuses a row.

A compaction CASE is (capacity, pattern); ``run_case`` plays it on a device
and returns everything observable, whole tensors included.
test_hash_evict_gpu.py plays the same cases on the GPU."""

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import HashedEmbeddingTable

import test_hash_index as index_test
import test_hashed_table as table_test

EMPTY = ops.HASH_EMPTY
CAPS = [8, 64]
PATTERNS = ["all_kept", "none_kept", "size_zero", "full", "alternating",
            "last_only", "first_evicted", "most_evicted", "few_evicted",
            "beyond_size"]
DIM = table_test.DIM


# ------------------------------------------------------------- compaction

def keep_pattern(name, cap):
    """(size, keep bool [cap]) of a named pattern."""
    size = {"size_zero": 0, "full": cap, "beyond_size": cap // 2}.get(
        name, cap * 3 // 4)
    r = torch.arange(cap)
    keep = {
        "all_kept": r >= 0,
        "none_kept": r < 0,
        "size_zero": r >= 0,
        "full": r % 3 != 0,
        "alternating": r % 2 == 0,
        "last_only": r == size - 1,
        "first_evicted": r != 0,
        "most_evicted": r % 4 == 3,         # movers < evicted
        "few_evicted": r % 4 != 1,
        "beyond_size": (r % 2 == 1) | (r >= size),  # true behind size
    }[name]
    return size, keep


def make_buffers(cap, D, device, aligned=True):
    """master fp32, shadow bf16 and two fp32 states [cap, D] plus stamps,
    every element random (rows behind size too: they must stay as they
    are). Unaligned: views that start one element into their storage."""
    gen = torch.Generator().manual_seed(cap * 1000 + D)
    off = 0 if aligned else 1

    def buf(dtype):
        flat = torch.randn(cap * D + 4, generator=gen).to(dtype).to(device)
        return flat[off:off + cap * D].view(cap, D)

    tables = [buf(torch.float32), buf(torch.bfloat16), buf(torch.float32),
              buf(torch.float32)]
    stamps = torch.randint(0, 50, (cap,), generator=gen).to(device)
    return tables, stamps


def new_keys(count):
    return torch.arange(count) * 1000003 + 10 ** 12


def run_case(cap, pattern, device="cpu", D=DIM, aligned=True, compact=None):
    """Insert ``size`` keys, compact with the pattern, then go on: look up
    every old key, insert new keys (two more than there is room for), look
    everything up again. ``compact`` replaces ops.hash_compact (the naive
    oracle). Returns a dict of CPU tensors and ints."""
    size, keep = keep_pattern(pattern, cap)
    pool = index_test.pool97()
    index = ops.HashIndex(cap, device)
    rows, _ = ops.hash_find_or_insert(index, pool[:size].to(device))
    assert rows.tolist() == list(range(size))
    tables, stamps = make_buffers(cap, D, device, aligned)
    res = (compact or ops.hash_compact)(index, keep.to(device), tables,
                                        stamps)
    assert res is None
    K = int(keep[:size].sum())
    out = {"row_keys": index.row_keys.cpu().clone(),
           "tables": [t.cpu().clone() for t in tables],
           "stamps": stamps.cpu().clone(), "size": int(index.size),
           "evicted": int(index.evicted), "K": K}
    out["find_old"] = ops.hash_find(index, pool[:size].to(device)).cpu()
    fresh = new_keys(cap - K + 2).to(device)
    got_rows, is_new = ops.hash_find_or_insert(index, fresh)
    out["fresh_rows"], out["is_new"] = got_rows.cpu(), is_new.cpu()
    out["dropped"] = int(index.dropped)
    both = torch.cat([pool[:size].to(device), fresh])
    out["find_all"] = ops.hash_find(index, both).cpu()
    out["row_keys_after"] = index.row_keys.cpu().clone()
    return out


def naive_compact(index, keep, tables, stamps):
    """The contract spelled out on Python lists; the mapping is rebuilt as
    a dict from scratch."""
    size = int(index.size)
    keep = keep.tolist()
    row_keys = index.row_keys.tolist()
    cols = [t.tolist() for t in tables] + [stamps.tolist()]
    K = sum(1 for r in range(size) if keep[r])
    holes = [r for r in range(K) if not keep[r]]
    movers = [r for r in range(K, size) if keep[r]]
    assert len(holes) == len(movers)
    for h, m in zip(holes, movers):
        row_keys[h] = row_keys[m]
        for c in cols:
            c[h] = c[m]
    for r in range(K, size):
        row_keys[r] = EMPTY
    index.row_keys.copy_(torch.tensor(row_keys, dtype=torch.int64))
    for t, c in zip(list(tables) + [stamps], cols):
        t.copy_(torch.tensor(c).to(t.dtype))    # bf16 -> float -> bf16: exact
    index.size.fill_(K)
    index.evicted += size - K
    index._map = {row_keys[r]: r for r in range(K)}


def assert_same_case(got, want):
    assert sorted(got) == sorted(want)
    for k, b in want.items():
        a = got[k]
        if isinstance(b, list):
            assert len(a) == len(b)
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and torch.equal(x, y), k
        elif isinstance(b, torch.Tensor):
            assert a.dtype == b.dtype and torch.equal(a, b), k
        else:
            assert a == b, k


def check_case_invariants(cap, pattern, out):
    """What must hold whatever the implementation: survivors found at their
    new rows, evicted keys gone, new keys in rows K, K + 1, ..."""
    size, keep = keep_pattern(pattern, cap)
    K = out["K"]
    pool = index_test.pool97()
    assert out["size"] == K and out["evicted"] == size - K
    assert (out["row_keys"][K:] == EMPTY).all()
    kept = keep[:size]
    assert (out["find_old"][~kept] == -1).all()
    found = out["find_old"][kept]
    assert sorted(found.tolist()) == list(range(K))
    assert torch.equal(out["row_keys"][found], pool[:size][kept])
    # a survivor below K kept its row
    stay = kept & (torch.arange(size) < K)
    assert torch.equal(out["find_old"][stay], torch.arange(size)[stay])
    room = cap - K
    assert out["fresh_rows"].tolist() == list(range(K, cap)) + [-1, -1]
    assert out["is_new"].tolist() == [True] * room + [False] * 2
    assert out["dropped"] == 2
    assert torch.equal(out["find_all"][:size], out["find_old"])
    assert torch.equal(out["find_all"][size:], out["fresh_rows"])


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("cap", CAPS)
def test_compact_matches_naive_oracle(cap, pattern):
    got = run_case(cap, pattern)
    assert_same_case(got, run_case(cap, pattern, compact=naive_compact))
    check_case_invariants(cap, pattern, got)


def test_compact_moves_rows_with_their_keys():
    """Alternating at capacity 8, size 6, spelled out: rows 0 2 4 are kept,
    K = 3, so row 2 stays where it is and hole 1 takes row 4."""
    cap = 8
    before, stamps0 = make_buffers(cap, DIM, "cpu")
    got = run_case(cap, "alternating")
    # kept 0, 2, 4; K = 3; holes [1], movers [4]
    pool = index_test.pool97()
    assert got["row_keys"][:3].tolist() == pool[[0, 4, 2]].tolist()
    for t, b in zip(got["tables"], before):
        assert torch.equal(t[1], b[4])
        b[1] = b[4]
        assert torch.equal(t, b)            # nothing else was written
    assert got["stamps"][1] == stamps0[4]


def test_compact_input_checks():
    index = ops.HashIndex(8)
    tables, stamps = make_buffers(8, DIM, "cpu")
    keep = torch.ones(8, dtype=torch.bool)
    for bad_keep in (keep[:7], keep.long(), torch.ones(9, dtype=torch.bool)):
        with pytest.raises(ValueError):
            ops.hash_compact(index, bad_keep, tables, stamps)
    for bad in (tables[0][:7], tables[0].double(), tables[0][:, :4],
                tables[0].view(-1)):
        with pytest.raises(ValueError):
            ops.hash_compact(index, keep, [tables[0], bad], stamps)
    with pytest.raises(ValueError):
        ops.hash_compact(index, keep, tables + tables[:1], stamps)
    with pytest.raises(ValueError):
        ops.hash_compact(index, keep, tables, stamps[:7])
    with pytest.raises(ValueError):
        ops.hash_touch(torch.zeros(3, dtype=torch.int32), stamps, 1)
    with pytest.raises(ValueError):
        ops.hash_touch(torch.zeros(3, dtype=torch.int64), stamps.int(), 1)
    assert ops.hash_compact(index, keep, [], None) is None


def test_touch_stamps_valid_rows_only():
    stamps = torch.full((8,), 3)
    ops.hash_touch(torch.tensor([5, -1, 0, 8, 5, 2 ** 40]), stamps, 9)
    assert stamps.tolist() == [9, 3, 3, 3, 3, 9, 3, 3]
    ops.hash_touch(torch.zeros(0, dtype=torch.int64), stamps, 11)
    assert stamps.tolist() == [9, 3, 3, 3, 3, 9, 3, 3]


def run_remove(device="cpu"):
    pool = index_test.pool97()
    index = ops.HashIndex(16, device)
    ops.hash_find_or_insert(index, pool[:10].to(device))
    tables, stamps = make_buffers(16, DIM, device)
    gone = torch.tensor([int(pool[3]), int(pool[3]), 424242, EMPTY,
                         int(pool[7]), int(pool[90])])
    assert ops.hash_remove(index, gone.to(device), tables, stamps) is None
    return {"row_keys": index.row_keys.cpu().clone(),
            "tables": [t.cpu().clone() for t in tables],
            "stamps": stamps.cpu().clone(), "size": int(index.size),
            "evicted": int(index.evicted),
            "find": ops.hash_find(index, pool[:12].to(device)).cpu()}


def test_remove_ignores_absent_duplicate_and_reserved_keys():
    out = run_remove()
    pool = index_test.pool97()
    assert out["size"] == 8 and out["evicted"] == 2
    # K = 8: holes [3, 7] take movers [8, 9], pair by pair
    assert out["row_keys"][:8].tolist() == pool[[0, 1, 2, 8, 4, 5, 6,
                                                 9]].tolist()
    assert (out["row_keys"][8:] == EMPTY).all()
    assert out["find"].tolist() == [0, 1, 2, -1, 4, 5, 6, -1, 3, 7, -1, -1]
    before, stamps0 = make_buffers(16, DIM, "cpu")
    for t, b in zip(out["tables"], before):
        b[3], b[7] = b[8].clone(), b[9].clone()
        assert torch.equal(t, b)
    # nothing to remove: nothing moves
    index = ops.HashIndex(4)
    ops.hash_find_or_insert(index, torch.tensor([5, 6]))
    ops.hash_remove(index, torch.tensor([EMPTY, 7]), [], None)
    assert int(index.size) == 2 and int(index.evicted) == 0
    assert ops.hash_find(index, torch.tensor([5, 6, 7])).tolist() == [0, 1, -1]


# -------------------------------------------------------------- the table

class EvictOracle(table_test.Oracle):
    """The dense oracle of test_hashed_table.py with keys that can leave: a
    key that is evicted is deleted from the dict and its dense row is never
    used again; when the key comes back it takes a NEW dense row, set to
    its initial value with zero state. ``stamp[k]`` is the step of the last
    request that named k; after a push that leaves step % evict_every == 0
    every key with step - stamp > max_idle goes."""

    def __init__(self, optimizer, hparams, device="cpu", evict_every=None,
                 max_idle=None, dense_rows=1024):
        super().__init__(optimizer, hparams, device, capacity=dense_rows)
        self.next_row = 0
        self.stamp = {}
        self.evicted = 0
        self.reborn = 0
        self.ever = set()
        self.evict_every, self.max_idle = evict_every, max_idle

    def rows(self, keys, insert=True):
        t = self.table
        for k in keys.tolist():
            if insert and k not in self.row_of:
                r = self.row_of[k] = self.next_row
                self.next_row += 1
                self.reborn += k in self.ever
                self.ever.add(k)
                init = ops.hash_init_rows(torch.tensor([k]), DIM,
                                          table_test.SEED)[0]
                t.master[r] = init.to(self.device)
                t.shadow[r] = init.to(torch.bfloat16).to(self.device)
                for s in t.state.values():
                    s[r] = 0.0
            if k in self.row_of:
                self.stamp[k] = t.step
        return torch.tensor([self.row_of.get(k, -1) for k in keys.tolist()],
                            dtype=torch.int64).to(self.device)

    def drop_idle(self, max_idle):
        step = self.table.step
        for k in [k for k in self.row_of if step - self.stamp[k] > max_idle]:
            del self.row_of[k], self.stamp[k]
            self.evicted += 1

    def _policy(self):
        if self.evict_every and self.table.step % self.evict_every == 0:
            self.drop_idle(self.max_idle)

    def push(self, keys, grads):
        super().push(keys, grads)
        self._policy()

    def push_pooled(self, keys, offsets, grads, weights=None, combiner="sum"):
        super().push_pooled(keys, offsets, grads, weights, combiner)
        self._policy()


def assert_equals_by_key(table, oracle, got=(), want=()):
    """Master, shadow, state and stamps of every key the oracle holds; the
    table holds no other key."""
    n = len(oracle.row_of)
    st = table.stats()
    assert st["size"] == n and st["evicted"] == oracle.evicted
    assert st["dropped"] == 0
    dev = table.device
    keys = torch.tensor(list(oracle.row_of), dtype=torch.int64)
    rows = ops.hash_find(table.index, keys.to(dev))
    assert sorted(rows.tolist()) == list(range(n))
    assert (table.index.row_keys[n:] == EMPTY).all()
    dense = oracle.table
    orow = torch.tensor(list(oracle.row_of.values()),
                        dtype=torch.int64).to(dev)
    assert table.step == dense.step
    assert torch.equal(table.master[rows], dense.master[orow])
    assert torch.equal(table.shadow[rows], dense.shadow[orow])
    assert sorted(table.state) == sorted(dense.state)
    for k in table.state:
        assert torch.equal(table.state[k][rows], dense.state[k][orow]), k
    assert table.last_used[rows].tolist() == [oracle.stamp[k]
                                              for k in oracle.row_of]
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)


def play_policy_script(optimizer, hparams, device="cpu"):
    """test_hashed_table.script() on a table with evict_every=2,
    max_idle=2 and on the oracle."""
    reqs = table_test.script()
    table = table_test.make_table(optimizer, hparams, device, evict_every=2,
                                  max_idle=2)
    oracle = EvictOracle(optimizer, hparams, device, evict_every=2,
                         max_idle=2)
    got = table_test.play(table, reqs, device)
    want = table_test.play(oracle, reqs, device)
    return table, oracle, got, want


@pytest.mark.parametrize("optimizer,hparams", table_test.OPTIMIZERS,
                         ids=table_test.OPT_IDS)
def test_automatic_policy_equals_dict_oracle_by_key(optimizer, hparams):
    table, oracle, got, want = play_policy_script(optimizer, hparams)
    assert_equals_by_key(table, oracle, got, want)
    # the script did evict, and evicted keys did come back
    assert oracle.evicted > 0 and oracle.reborn > 0 and table.step == 7
    assert table.track_use and table.last_used.dtype == torch.int64


@pytest.mark.parametrize("optimizer,hparams", table_test.OPTIMIZERS,
                         ids=table_test.OPT_IDS)
def test_reinserted_key_starts_from_its_initial_row(optimizer, hparams):
    table = table_test.make_table(optimizer, hparams, track_use=True)
    pool = index_test.pool97()
    g = torch.ones(4, DIM, dtype=torch.bfloat16)
    table.push(pool[:4], g)
    table.push(pool[2:6], g)                # step 2; keys 0, 1 idle since 0
    moved = table.pull(pool[:1])            # a pull stamps too: key 0 -> 2
    table.evict(max_idle=0)                 # only stamp 2 survives: key 0
    assert table.stats() == {"size": 1, "dropped": 0, "capacity": 128,
                             "evicted": 5}
    init = ops.hash_init_rows(pool[:6], DIM, table_test.SEED)
    assert not torch.equal(moved, init[:1].to(torch.bfloat16))
    got = table.pull(pool[:6])
    assert torch.equal(got[:1], moved)
    assert torch.equal(got[1:], init[1:].to(torch.bfloat16))
    rows = ops.hash_find(table.index, pool[1:6])
    assert rows.tolist() == [1, 2, 3, 4, 5]
    assert torch.equal(table.master[rows], init[1:])
    for s in table.state.values():
        assert not s[rows].any()


def test_target_size_evicts_least_recently_used_lower_row_first():
    table = table_test.make_table("adagrad", {}, track_use=True)
    k = index_test.pool97()[:6]
    g = torch.ones(6, DIM, dtype=torch.bfloat16)
    table.push(k, g)                        # all stamped 0
    table.push(k[[2, 4]], g[:2])            # rows 2, 4 stamped 1
    table.evict(target_size=7)              # nothing to do
    assert table.stats()["size"] == 6 and table.stats()["evicted"] == 0
    before = table.master.clone()
    table.evict(target_size=3)
    # (stamp, row) ascending: (0,0) (0,1) (0,3) (0,5) (1,2) (1,4); the first
    # three go. keep = F F T F T T, K = 3: holes 0 1 <- movers 4 5
    assert table.index.row_keys[:3].tolist() == k[[4, 5, 2]].tolist()
    assert table.last_used[:3].tolist() == [1, 0, 1]
    assert torch.equal(table.master[:3], before[[4, 5, 2]])
    assert table.stats() == {"size": 3, "dropped": 0, "capacity": 128,
                             "evicted": 3}
    table.evict(target_size=0)
    assert table.stats()["size"] == 0 and table.stats()["evicted"] == 6


def test_both_rules_run_one_compaction(monkeypatch):
    table = table_test.make_table("adagrad", {}, track_use=True)
    k = index_test.pool97()[:8]
    g = torch.ones(8, DIM, dtype=torch.bfloat16)
    table.push(k, g)                        # stamps 0
    table.push(k[2:], g[:6])                # rows 2.. stamped 1
    table.push(k[5:], g[:3])                # rows 5, 6, 7 stamped 2
    calls = []
    real = ops.hash_compact
    monkeypatch.setattr(ops, "hash_compact",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    # step 3: idle > 2 drops rows 0, 1 (stamp 0); of the six survivors the
    # two with the smallest (stamp, row) — rows 2, 3 — go as well
    table.evict(max_idle=2, target_size=4)
    assert len(calls) == 1
    assert table.stats()["size"] == 4 and table.stats()["evicted"] == 4
    assert ops.hash_find(table.index, k).tolist() == [-1, -1, -1, -1, 0, 1,
                                                      2, 3]
    assert table.last_used[:4].tolist() == [1, 2, 2, 2]


def test_evict_value_errors():
    plain = table_test.make_table("adagrad", {})
    with pytest.raises(ValueError):
        plain.evict(max_idle=1)
    assert plain.last_used is None and not plain.track_use
    tracked = table_test.make_table("adagrad", {}, track_use=True)
    with pytest.raises(ValueError):
        tracked.evict()
    with pytest.raises(ValueError):
        tracked.evict(max_idle=-1)
    with pytest.raises(ValueError):
        tracked.evict(target_size=-1)
    for kw in ({"max_idle": 2}, {"evict_every": 2},
               {"max_idle": 0, "evict_every": 2},
               {"max_idle": 2, "evict_every": 0}):
        with pytest.raises(ValueError):
            table_test.make_table("adagrad", {}, **kw)
    auto = table_test.make_table("adagrad", {}, max_idle=3, evict_every=5)
    assert auto.track_use and (auto.max_idle, auto.evict_every) == (3, 5)
    shard = HashedEmbeddingTable.shard_of("t", DIM, 1, 2, 8, max_idle=1,
                                          evict_every=1, track_use=True)
    assert shard.track_use and shard.evict_every == 1


def test_full_table_accepts_a_dropped_key_after_evict():
    table = table_test.make_table("adagrad", {}, capacity=8, track_use=True)
    keys = index_test.pool97()[:9]
    g = torch.ones(9, DIM, dtype=torch.bfloat16) / 4
    table.push(keys, g)                     # rows 0..7 stamped 0, key 8 lost
    assert table.stats() == {"size": 8, "dropped": 1, "capacity": 8,
                             "evicted": 0}
    table.push(keys[4:8], g[:4])            # rows 4..7 stamped 1; step 2
    table.evict(max_idle=1)                 # 2 - 0 > 1: rows 0..3 go
    assert table.stats() == {"size": 4, "dropped": 1, "capacity": 8,
                             "evicted": 4}
    want = ops.hash_init_rows(keys[8:], DIM, table_test.SEED)
    assert torch.equal(table.pull(keys[8:]), want.to(torch.bfloat16))
    assert ops.hash_find(table.index, keys).tolist() == [-1, -1, -1, -1, 0,
                                                         1, 2, 3, 4]
    # and without tracking: remove makes the room
    plain = table_test.make_table("adagrad", {}, capacity=8)
    plain.push(keys, g)
    assert not plain.pull(keys[8:]).any()
    plain.remove(keys[:2])
    want = ops.hash_init_rows(keys[8:], DIM, table_test.SEED)
    assert torch.equal(plain.pull(keys[8:]), want.to(torch.bfloat16))
    assert plain.stats() == {"size": 7, "dropped": 2, "capacity": 8}
    assert ops.hash_find(plain.index, keys).tolist() == [-1, -1, 2, 3, 4, 5,
                                                         0, 1, 6]


def test_untracked_table_is_unchanged():
    table = table_test.make_table("adam", {})
    table_test.play(table, table_test.script()[:4])
    assert sorted(table.stats()) == ["capacity", "dropped", "size"]
    assert sorted(table.state_dict()) == ["keys", "master", "optimizer",
                                          "seed", "state", "step"]
    assert table.last_used is None


@pytest.mark.parametrize("optimizer,hparams", table_test.OPTIMIZERS,
                         ids=table_test.OPT_IDS)
def test_checkpoint_with_stamps_continues_bit_identically(optimizer,
                                                          hparams):
    reqs = table_test.script()
    kw = dict(evict_every=2, max_idle=2)
    a = table_test.make_table(optimizer, hparams, **kw)
    table_test.play(a, reqs[:8])
    sd = a.state_dict()
    n = a.stats()["size"]
    e0 = a.stats()["evicted"]
    assert sd["last_used"].shape == (n,)
    assert torch.equal(sd["last_used"], a.last_used[:n])
    b = HashedEmbeddingTable("t", DIM, 200, lr=0.05, seed=99,
                             optimizer=optimizer, **hparams, **kw)
    b.load_state_dict(sd)
    more = [r for r in reqs[8:] if r[0].startswith("push")][:3]
    table_test.play(a, more)
    table_test.play(b, more)
    m = a.stats()["size"]
    assert a.step == b.step == 7 and b.stats()["size"] == m
    # the policy ran before and after the checkpoint (a load resets the
    # counter, like ``dropped``)
    assert e0 > 0 and a.stats()["evicted"] - e0 == b.stats()["evicted"] > 0
    assert torch.equal(a.index.row_keys[:m], b.index.row_keys[:m])
    assert torch.equal(a.last_used[:m], b.last_used[:m])
    assert torch.equal(a.master[:m], b.master[:m])
    assert torch.equal(a.shadow[:m], b.shadow[:m])
    for k in a.state:
        assert torch.equal(a.state[k][:m], b.state[k][:m]), k


def test_load_of_a_checkpoint_without_stamps():
    plain = table_test.make_table("adagrad", {})
    table_test.play(plain, table_test.script()[:4])
    sd = plain.state_dict()
    assert "last_used" not in sd and sd["step"] == 2
    n = sd["keys"].numel()
    t = table_test.make_table("adagrad", {}, track_use=True)
    t.load_state_dict(sd)
    assert t.last_used[:n].tolist() == [2] * n
    t.evict(max_idle=0)
    assert t.stats()["size"] == n           # nobody is idle yet
    # a tracked checkpoint loads into an untracked table
    plain.load_state_dict(t.state_dict())
    assert plain.stats() == {"size": n, "dropped": 0, "capacity": 128}


def test_reserve_after_evict_carries_the_stamps():
    table = table_test.make_table("adagrad", {}, capacity=8, track_use=True)
    keys = index_test.pool97()[:12]
    g = torch.ones(12, DIM, dtype=torch.bfloat16) / 4
    table.push(keys[:8], g[:8])
    table.push(keys[3:8], g[:5])            # stamped 1; step 2
    table.evict(max_idle=1)
    assert table.stats()["size"] == 5
    rows = ops.hash_find(table.index, keys[3:8])
    master, stamps = table.master[:5].clone(), table.last_used[:5].clone()
    table.reserve(16)
    assert table.last_used.shape == (16,)
    assert torch.equal(table.last_used[:5], stamps)
    assert torch.equal(table.master[:5], master)
    assert torch.equal(ops.hash_find(table.index, keys[3:8]), rows)
    table.push(keys, g)                     # 7 more keys: 12 rows
    assert table.stats() == {"size": 12, "dropped": 0, "capacity": 16,
                             "evicted": 3}
    assert table.last_used[:12].tolist() == [2] * 12
