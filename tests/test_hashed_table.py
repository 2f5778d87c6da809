"""HashedEmbeddingTable on the CPU against a dense oracle: an
``EmbeddingTable(fused_apply=True)`` whose rows are set from
``ops.hash_init_rows`` of the keys in the order a plain dict first sees
them, driven with the dict's row numbers. Both sides run the same row ops
on the same rows, so every comparison is torch.equal. test_hash_gpu.py
plays the same script on the GPU."""

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import (EmbeddingTable, HashedEmbeddingTable,
                                   _ShardRoute)

import test_hash_index as index_test

DIM = 8
CAPACITY = 128
SEED = 21
OPTIMIZERS = [("sgd", {"momentum": 0.9}), ("adagrad", {}), ("adam", {})]
OPT_IDS = ["sgd_momentum", "adagrad", "adam"]


class Oracle(object):
    """Dense table + dict. ``rows(keys, insert)`` is the whole translation:
    a new key takes the next row and the row is set to its initial value."""

    def __init__(self, optimizer, hparams, device="cpu", capacity=CAPACITY,
                 insert_on_pull=True):
        self.table = EmbeddingTable("oracle", capacity, DIM, device=device,
                                    lr=0.05, seed=1, optimizer=optimizer,
                                    fused_apply=True, **hparams)
        self.row_of = {}
        self.device = device
        self.insert_on_pull = insert_on_pull

    def rows(self, keys, insert=True):
        new = []
        for k in keys.tolist():
            if insert and k not in self.row_of:
                self.row_of[k] = len(self.row_of)
                new.append(k)
        if new:
            t = self.table
            r = torch.tensor([self.row_of[k] for k in new]).to(self.device)
            init = ops.hash_init_rows(torch.tensor(new), DIM, SEED)
            t.master[r] = init.to(self.device)
            t.shadow[r] = init.to(torch.bfloat16).to(self.device)
            for s in t.state.values():
                s[r] = 0.0
        return torch.tensor([self.row_of.get(k, -1) for k in keys.tolist()],
                            dtype=torch.int64).to(self.device)

    def pull(self, keys):
        rows = self.rows(keys, self.insert_on_pull)
        if self.device != "cpu":
            return self.table.pull(rows)    # the kernel zero-fills row -1
        out = torch.zeros(rows.numel(), DIM, dtype=torch.bfloat16)
        out[rows >= 0] = self.table.shadow[rows[rows >= 0]]
        return out

    def push(self, keys, grads):
        self.table.push(self.rows(keys), grads)

    def pull_pooled(self, keys, offsets, weights=None, combiner="sum"):
        return self.table.pull_pooled(self.rows(keys, self.insert_on_pull),
                                      offsets, weights, combiner)

    def push_pooled(self, keys, offsets, grads, weights=None, combiner="sum"):
        self.table.push_pooled(self.rows(keys), offsets, grads, weights,
                               combiner)


def make_table(optimizer, hparams, device="cpu", capacity=CAPACITY, **kw):
    return HashedEmbeddingTable("t", DIM, capacity, device=device, lr=0.05,
                                seed=SEED, optimizer=optimizer, **hparams,
                                **kw)


def script():
    """A mixed request sequence over keys that appear gradually (the first
    k keys of a 97-key pool that holds INT64_MAX, 0, -1 and a negative
    key): [(method, args...)]. Gradients and weights are dyadic."""
    pool = index_test.pool97()
    gen = torch.Generator().manual_seed(77)

    def keys(lo, hi, n):
        return pool[torch.randint(lo, hi, (n,), generator=gen)]

    def grads(n):
        return (torch.randint(-8, 9, (n, DIM), generator=gen).float()
                / 16).to(torch.bfloat16)

    def bags(n, B):
        cuts = torch.sort(torch.randint(0, n + 1, (B - 1,),
                                        generator=gen))[0]
        return torch.cat([torch.tensor([0]), cuts, torch.tensor([n])])

    def weights(n):
        return torch.randint(1, 5, (n,), generator=gen).float() / 4

    reqs = []
    k = keys(0, 20, 33)
    reqs += [("pull", k), ("push", k, grads(33))]
    k, o = keys(0, 35, 50), bags(50, 9)
    reqs += [("pull_pooled", k, o, None, "sum"),
             ("push_pooled", k, o, grads(9), None, "sum")]
    k, o, w = keys(10, 50, 65), bags(65, 12), weights(65)
    reqs += [("pull_pooled", k, o, w, "mean"),
             ("push_pooled", k, o, grads(12), w, "mean")]
    k = keys(0, 60, 70)
    reqs += [("push", k, grads(70)), ("pull", k)]
    k, o, w = keys(40, 75, 64), bags(64, 7), weights(64)
    reqs += [("pull_pooled", k, o, w, "sum"),
             ("push_pooled", k, o, grads(7), w, "sum"),
             ("pull_pooled", k, o, None, "mean"),
             ("push_pooled", k, o, grads(7), None, "mean")]
    k = keys(0, 97, 40)
    reqs += [("push", k, grads(40)), ("pull", pool)]
    return reqs


def play(table, reqs, device="cpu"):
    """Run the script on a table or an oracle; the pulled tensors."""
    pulled = []
    for method, *args in reqs:
        args = [a.to(device) if isinstance(a, torch.Tensor) else a
                for a in args]
        res = getattr(table, method)(*args)
        if method.startswith("pull"):
            pulled.append(res)
    return pulled


def assert_equals_oracle(table, oracle, got, want):
    n = len(oracle.row_of)
    assert table.stats() == {"size": n, "dropped": 0,
                             "capacity": table.capacity}
    assert table.index.row_keys[:n].tolist() == list(oracle.row_of)
    dense = oracle.table
    assert table.step == dense.step
    assert torch.equal(table.master[:n], dense.master[:n])
    assert torch.equal(table.shadow[:n], dense.shadow[:n])
    assert sorted(table.state) == sorted(dense.state)
    for k in table.state:
        assert torch.equal(table.state[k], dense.state[k]), k
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("optimizer,hparams", OPTIMIZERS, ids=OPT_IDS)
def test_mixed_sequence_equals_dense_oracle(optimizer, hparams):
    reqs = script()
    table, oracle = make_table(optimizer, hparams), Oracle(optimizer, hparams)
    got, want = play(table, reqs), play(oracle, reqs)
    assert_equals_oracle(table, oracle, got, want)
    assert table.step == 7 and table.stats()["size"] == 97
    # keys did appear gradually, and training moved the rows
    init = ops.hash_init_rows(table.index.row_keys[:97], DIM, SEED)
    assert not torch.equal(table.master[:97], init)
    assert set(table.state) == set(oracle.table.state)


def test_first_pull_returns_the_initial_row():
    table = make_table("adagrad", {})
    keys = torch.tensor([7, -7, 7, ops.HASH_EMPTY])
    want = ops.hash_init_rows(keys, DIM, SEED).to(torch.bfloat16)
    want[3] = 0
    assert torch.equal(table.pull(keys), want)
    assert table.stats()["size"] == 2       # the reserved key has no row


def test_serving_table_never_inserts_on_pull():
    table = make_table("adam", {}, insert_on_pull=False)
    pool = index_test.pool97()
    zeros = torch.zeros(10, DIM, dtype=torch.bfloat16)
    assert torch.equal(table.pull(pool[:10]), zeros)
    offsets = torch.tensor([0, 4, 10])
    assert torch.equal(table.pull_pooled(pool[:10], offsets), zeros[:2])
    assert table.stats()["size"] == 0
    g = torch.ones(5, DIM, dtype=torch.bfloat16)
    table.push(pool[:5], g)
    assert table.stats()["size"] == 5
    rows = table.pull(pool[:10])
    assert torch.equal(rows[:5], table.shadow[:5]) and rows[:5].any()
    assert torch.equal(rows[5:], zeros[5:])
    assert table.stats()["size"] == 5
    # the same requests on the oracle
    oracle = Oracle("adam", {}, insert_on_pull=False)
    oracle.push(pool[:5], g)
    assert torch.equal(rows, oracle.pull(pool[:10]))
    assert torch.equal(table.pull_pooled(pool[:10], offsets, None, "mean"),
                       oracle.pull_pooled(pool[:10], offsets, None, "mean"))


def test_full_table_drops_new_keys_until_reserve():
    table = make_table("adagrad", {}, capacity=8)
    oracle = Oracle("adagrad", {}, capacity=16)
    keys = index_test.pool97()[:12]
    g = torch.ones(12, DIM, dtype=torch.bfloat16) / 4
    table.push(keys, g)
    assert table.stats() == {"size": 8, "dropped": 4, "capacity": 8}
    pulled = table.pull(keys)
    assert not pulled[8:].any() and pulled[:8].any()
    assert table.stats()["dropped"] == 8
    oracle.push(keys[:8], g[:8])
    table.reserve(16)
    assert table.stats() == {"size": 8, "dropped": 8, "capacity": 16}
    assert torch.equal(table.pull(keys[:8]), pulled[:8])
    table.push(keys, g)
    oracle.pull(keys[:8])
    oracle.push(keys, g)
    assert torch.equal(table.master[:12], oracle.table.master[:12])
    assert torch.equal(table.state["accum"][:12],
                       oracle.table.state["accum"][:12])
    assert torch.equal(table.shadow[:12], oracle.table.shadow[:12])
    with pytest.raises(ValueError):
        table.reserve(4)


@pytest.mark.parametrize("optimizer,hparams", OPTIMIZERS, ids=OPT_IDS)
def test_checkpoint_round_trip_continues_bit_identically(optimizer, hparams):
    """state_dict -> load_state_dict into a table of another capacity (and
    another seed: the checkpoint's wins), then three more pushes that bring
    new keys: equal to the table that never stopped."""
    reqs = script()
    a = make_table(optimizer, hparams)
    play(a, reqs[:8])
    sd = a.state_dict()
    n = a.stats()["size"]
    assert sd["keys"].shape == (n,) and sd["master"].shape == (n, DIM)
    assert all(v.shape == (n, DIM) for v in sd["state"].values())
    assert sd["step"] == a.step and sd["seed"] == SEED
    b = HashedEmbeddingTable("t", DIM, n + 40, lr=0.05, seed=99,
                             optimizer=optimizer, **hparams)
    b.load_state_dict(sd)
    more = [r for r in reqs[8:] if r[0].startswith("push")][:3]
    assert len(more) == 3
    play(a, more)
    play(b, more)
    m = a.stats()["size"]
    assert m > n and b.stats()["size"] == m and a.step == b.step
    assert torch.equal(a.index.row_keys[:m], b.index.row_keys[:m])
    assert torch.equal(a.master[:m], b.master[:m])
    assert torch.equal(a.shadow[:m], b.shadow[:m])
    for k in a.state:
        assert torch.equal(a.state[k][:m], b.state[k][:m]), k
    with pytest.raises(ValueError):
        HashedEmbeddingTable("t", DIM, n - 1, optimizer=optimizer,
                             **hparams).load_state_dict(sd)


def shard_requests():
    """Pushes and pulls over keys in [0, 2**62); one push names keys of a
    single shard only (every shard must still step)."""
    gen = torch.Generator().manual_seed(9)
    pool = torch.cat([torch.randint(0, ops.HASH_KEY_SPACE, (40,),
                                    generator=gen),
                      torch.tensor([0, 1, 2, ops.HASH_KEY_SPACE - 1])])
    reqs = []
    for k in range(4):
        keys = pool[torch.randint(0, 44, (50,), generator=gen)]
        if k == 2:
            keys = keys[keys % 3 == 1]
        g = (torch.randint(-8, 9, (keys.numel(), DIM), generator=gen).float()
             / 16).to(torch.bfloat16)
        reqs += [("pull", keys), ("push", keys, g)]
    return pool, reqs


@pytest.mark.parametrize("optimizer,hparams", OPTIMIZERS, ids=OPT_IDS)
def test_three_shards_equal_the_unsharded_table_key_for_key(optimizer,
                                                            hparams):
    pool, reqs = shard_requests()
    whole = make_table(optimizer, hparams)
    shards = [HashedEmbeddingTable.shard_of(
        "t", DIM, s, 3, 64, lr=0.05, seed=SEED, optimizer=optimizer,
        **hparams) for s in range(3)]
    for method, keys, *g in reqs:
        r = _ShardRoute(keys, ops.HASH_KEY_SPACE, 3, "mod")
        if method == "pull":
            buf = torch.empty(r.n, DIM, dtype=torch.bfloat16)
            for s, t in enumerate(shards):
                if r.count(s):
                    buf[r.span(s)] = t.pull(r.ids(s))
            assert torch.equal(r.to_request_order(buf), whole.pull(keys))
        else:
            rows = r.to_slots(g[0])
            for s, t in enumerate(shards):
                t.push(r.ids(s), rows[r.span(s)])
            whole.push(keys, g[0])
    n = whole.stats()["size"]
    keys = whole.index.row_keys[:n]
    assert n == len(set(k for _, ks, *_ in reqs for k in ks.tolist()))
    assert sum(t.stats()["size"] for t in shards) == n
    assert [t.step for t in shards] == [whole.step] * 3 == [4] * 3
    for s, t in enumerate(shards):
        mine = keys % 3 == s
        rows = ops.hash_find(t.index, keys[mine] // 3)
        assert (rows >= 0).all() and mine.any()
        assert torch.equal(t.master[rows], whole.master[:n][mine])
        assert torch.equal(t.shadow[rows], whole.shadow[:n][mine])
        for k in whole.state:
            assert torch.equal(t.state[k][rows], whole.state[k][:n][mine]), k


def test_constructor_checks():
    with pytest.raises(ValueError):
        HashedEmbeddingTable("t", DIM, 8, optimizer="lion")
    with pytest.raises(ValueError):
        HashedEmbeddingTable("t", DIM, 8, optimizer="sgd", beta1=0.5)
    with pytest.raises(ValueError):
        HashedEmbeddingTable.shard_of("t", DIM, 3, 3, 8)
    t = HashedEmbeddingTable.shard_of("t", DIM, 2, 3, 8)
    assert (t.key_mul, t.key_add, t.capacity) == (3, 2, 8)
