"""Hashed embedding tables on the GPU — csrc/hash.hip — against the CPU
reference (a dict): the index ops on every script of test_hash_index.py,
the init kernel against ops.hash_init_rows, hash_gather against find +
embedding_gather, a probe chain longer than one wave, HashedEmbeddingTable
against a dense GPU EmbeddingTable driven with a dict's rows, and the stock
server and client end to end.

Every comparison is torch.equal: the index contract is integer-exact, the
initialiser is specified to the bit, and the row math of a hashed table and
of its dense oracle runs through the same kernels on the same rows."""

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import HashedEmbeddingTable

import test_hash_dist as dist_test
import test_hash_index as index_test
import test_hashed_table as table_test

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTHS = [7, 8, 130, 320]   # scalar path, vector path, even but no multiple
                            # of 4, more than one 256-column tile


# --------------------------------------------------------------- the index

def check_script(script):
    want = index_test.run_script(script)
    got = index_test.run_script(script, DEV)
    index_test.assert_same_run(got, want)
    index_test.assert_same_run(index_test.run_script(script, DEV), got)


@pytest.mark.parametrize("kind", index_test.KINDS)
@pytest.mark.parametrize("n", index_test.SIZES)
def test_index_matches_cpu_on_request_sizes_and_key_kinds(n, kind):
    check_script(index_test.size_script(n, kind))


@pytest.mark.parametrize("name", ["duplicate", "mixed", "overflow"])
def test_index_matches_cpu_on_scripts(name):
    check_script(getattr(index_test, name + "_script")())


def test_index_state_stays_on_the_device():
    index = ops.HashIndex(8, DEV)
    keys = torch.tensor(index_test.SPECIAL, device=DEV)
    rows, is_new = ops.hash_find_or_insert(index, keys)
    for t in (rows, is_new, index.size, index.dropped, index.row_keys,
              index.slot_keys, index.slot_rows):
        assert t.device.type == "cuda"
    assert index.slot_keys.numel() == ops.hash_slots(8) == 64
    assert rows.tolist() == [0, 1, 2, 3, 4] and is_new.all()
    with pytest.raises(ValueError):
        ops.hash_find(index, keys.cpu())


def test_probe_chain_longer_than_one_wave():
    """Capacity 64 (H = 128): 64 keys that all hash to slot 5 fill slots
    5..68, so the chain spans more than the 64 slots one wave reads per
    step; six more such keys are looked up and missed at its end."""
    cand = torch.arange(20000)
    chain = cand[ops.hash_home(cand, 128) == 5]
    assert chain.numel() >= 70      # about 20000 / 128 = 156 expected
    chain = chain[:70]
    cpu, gpu = ops.HashIndex(64), ops.HashIndex(64, DEV)
    assert gpu.slot_keys.numel() == 128
    want = ops.hash_find_or_insert(cpu, chain[:64])
    got = ops.hash_find_or_insert(gpu, chain[:64].to(DEV))
    assert want[0].tolist() == list(range(64))
    assert torch.equal(got[0].cpu(), want[0])
    assert torch.equal(got[1].cpu(), want[1])
    want_rows = ops.hash_find(cpu, chain)
    assert want_rows.tolist() == list(range(64)) + [-1] * 6
    assert torch.equal(ops.hash_find(gpu, chain.to(DEV)).cpu(), want_rows)
    # the wave-per-key probe walks the same chain
    table = torch.arange(64 * 8, device=DEV).view(64, 8).to(torch.bfloat16)
    rows = ops.hash_gather(gpu, table, chain.to(DEV))
    assert torch.equal(rows[:64], table) and not rows[64:].any()
    # a full table drops the other six, the same on both sides
    w = ops.hash_find_or_insert(cpu, chain)
    g = ops.hash_find_or_insert(gpu, chain.to(DEV))
    assert torch.equal(g[0].cpu(), w[0]) and not g[1].any()
    assert int(gpu.dropped) == int(cpu.dropped) == 6
    ops.hash_rebuild(gpu)
    assert torch.equal(ops.hash_find(gpu, chain.to(DEV)).cpu(), want_rows)


# ------------------------------------------------------------ init kernel

def init_case(D, num_states, aligned=True, key_mul=1, key_add=0):
    """Insert 97 keys in two requests (the second mixes known and new keys
    and repeats some); buffers start at 7 so that every row the kernel must
    not touch is seen to be untouched."""
    cap, seed = 128, 13

    def buf(dtype):
        flat = torch.full((cap * D + 4,), 7.0, dtype=dtype, device=DEV)
        off = 0 if aligned else 1
        return flat[off:off + cap * D].view(cap, D)

    master, shadow = buf(torch.float32), buf(torch.bfloat16)
    states = [buf(torch.float32) for _ in range(num_states)]
    index = ops.HashIndex(cap, DEV)
    pool = index_test.pool97().to(DEV)
    if key_mul != 1:
        pool = torch.arange(97, device=DEV) * 1000 + 5   # a shard's local keys
    for req in (pool[:50], torch.cat([pool[30:], pool[40:60]])):
        rows, is_new = ops.hash_find_or_insert(index, req)
        if req.numel() > 50:    # rows 0..49 exist: mark them, they must stay
            master[:50] = 3.0
        ops.hash_init_new_rows(req, rows, is_new, master, shadow, states,
                               seed, key_mul, key_add)
    n = int(index.size)
    keys = index.row_keys[:n].cpu()
    assert n == len(set(pool.tolist()))
    want = ops.hash_init_rows(keys, D, seed, key_mul, key_add)
    assert torch.equal(master[50:n].cpu(), want[50:])
    assert (master[:50] == 3.0).all()
    assert torch.equal(shadow[:n].cpu(), want.to(torch.bfloat16))
    for s in states:
        assert not s[:n].any() and (s[n:] == 7.0).all()
    assert (master[n:] == 7.0).all() and (shadow[n:] == 7.0).all()


@pytest.mark.parametrize("D", WIDTHS)
def test_init_kernel_matches_reference(D):
    init_case(D, 2)


def test_init_kernel_state_counts_shard_keys_and_unaligned_rows():
    init_case(8, 0)
    init_case(8, 1)
    init_case(8, 2, key_mul=3, key_add=2)
    init_case(8, 2, aligned=False)      # D % 4 == 0, bases off by one element


# ------------------------------------------------------------- hash_gather

@pytest.mark.parametrize("D", WIDTHS)
def test_hash_gather_matches_find_then_gather(D):
    gen = torch.Generator().manual_seed(D)
    index = ops.HashIndex(128, DEV)
    pool = index_test.pool97().to(DEV)
    ops.hash_find_or_insert(index, pool[:80])
    table = torch.randn(128, D, generator=gen).to(torch.bfloat16).to(DEV)
    for n in (1, 63, 64, 65, 257):
        keys = pool[torch.randint(0, 97, (n,), generator=gen).to(DEV)].clone()
        keys[::7] = ops.HASH_EMPTY
        rows = ops.hash_find(index, keys)
        want = ops.embedding_gather(table, rows)
        got = ops.hash_gather(index, table, keys)
        assert got.dtype == torch.bfloat16 and got.shape == (n, D)
        assert torch.equal(got, want)
        assert n < 63 or ((rows < 0).any() and (rows >= 0).any())
    assert ops.hash_gather(index, table, keys[:0]).shape == (0, D)


def test_hash_gather_unaligned_table_takes_scalar_path():
    index = ops.HashIndex(16, DEV)
    keys = torch.arange(-5, 15, device=DEV)
    ops.hash_find_or_insert(index, keys[:12])
    flat = torch.randn(16 * 8 + 1).to(torch.bfloat16).to(DEV)
    table = flat[1:].view(16, 8)
    assert table.data_ptr() % 8 == 2
    want = ops.embedding_gather(table, ops.hash_find(index, keys))
    assert torch.equal(ops.hash_gather(index, table, keys), want)


# --------------------------------------------------------------- table level

@pytest.mark.parametrize("optimizer,hparams", table_test.OPTIMIZERS,
                         ids=table_test.OPT_IDS)
def test_table_mixed_sequence_equals_dense_gpu_oracle(optimizer, hparams):
    reqs = table_test.script()
    table = table_test.make_table(optimizer, hparams, DEV)
    oracle = table_test.Oracle(optimizer, hparams, DEV)
    got = table_test.play(table, reqs, DEV)
    want = table_test.play(oracle, reqs, DEV)
    table_test.assert_equals_oracle(table, oracle, got, want)
    assert table.step == 7 and table.stats()["size"] == 97
    assert table.master.device.type == "cuda"


def test_serving_table_on_gpu():
    table = table_test.make_table("adam", {}, DEV, insert_on_pull=False)
    oracle = table_test.Oracle("adam", {}, DEV, insert_on_pull=False)
    pool = index_test.pool97().to(DEV)
    assert not table.pull(pool[:10]).any()
    assert table.stats()["size"] == 0
    g = torch.ones(5, 8, dtype=torch.bfloat16, device=DEV)
    table.push(pool[:5], g)
    oracle.push(pool[:5], g)
    rows = table.pull(pool[:10])
    assert rows[:5].any() and not rows[5:].any()
    assert torch.equal(rows, oracle.pull(pool[:10]))
    offsets = torch.tensor([0, 4, 10], device=DEV)
    assert torch.equal(table.pull_pooled(pool[:10], offsets, None, "mean"),
                       oracle.pull_pooled(pool[:10], offsets, None, "mean"))
    assert table.stats() == {"size": 5, "dropped": 0, "capacity": 128}


def test_full_table_reserve_and_checkpoint_on_gpu():
    table = table_test.make_table("adagrad", {}, DEV, capacity=8)
    oracle = table_test.Oracle("adagrad", {}, DEV, capacity=16)
    keys = index_test.pool97()[:12].to(DEV)
    g = torch.ones(12, 8, dtype=torch.bfloat16, device=DEV) / 4
    table.push(keys, g)
    oracle.push(keys[:8], g[:8])
    assert table.stats() == {"size": 8, "dropped": 4, "capacity": 8}
    assert not table.pull(keys)[8:].any()
    table.reserve(16)
    assert table.stats() == {"size": 8, "dropped": 8, "capacity": 16}
    table.push(keys, g)
    oracle.push(keys, g)
    assert torch.equal(table.master[:12], oracle.table.master[:12])
    assert torch.equal(table.shadow[:12], oracle.table.shadow[:12])
    assert torch.equal(table.state["accum"][:12],
                       oracle.table.state["accum"][:12])
    # checkpoint into a larger table with another seed; both train on
    other = HashedEmbeddingTable("t", 8, 40, device=DEV, lr=0.05, seed=1,
                                 optimizer="adagrad")
    other.load_state_dict(table.state_dict())
    more = index_test.pool97()[6:16].to(DEV)
    for t in (table, other):
        t.push(more, g[:10])
    assert table.stats()["size"] == other.stats()["size"] == 16
    assert torch.equal(table.index.row_keys[:16], other.index.row_keys[:16])
    assert torch.equal(table.master[:16], other.master[:16])
    assert torch.equal(table.shadow[:16], other.shadow[:16])
    assert torch.equal(table.state["accum"][:16], other.state["accum"][:16])


# ---------------------------------------------------------------- end to end

@pytest.mark.timeout(400)
@pytest.mark.parametrize("world", [2, 3], ids=["unsharded_adagrad",
                                               "mod_2ps_adam"])
def test_hashed_table_protocol_on_gpu(world, tmp_path):
    """PS rank(s) + 1 worker, all on cuda:0, over gloo, with coalescing on.
    Each process has its own timeout; nothing is started after the ranks,
    and a rank that exits nonzero fails the test before the local
    comparison runs."""
    prefix = str(tmp_path / "run")
    dist_test.run_world(world, prefix, True, device=DEV, timeout=120)
    dist_test.check_against_local(world, prefix, device=DEV)
