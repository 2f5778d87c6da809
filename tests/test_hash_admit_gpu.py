"""Feature admission on the GPU — the count / decide kernels of
hash_find_or_admit and the two fused serving kernels of csrc/hash.hip —
against the CPU references of ops/__init__.py, on the scripts and cases of
test_hash_admit.py.

Every comparison is torch.equal: the admission contract is integer-exact
(integer atomics commute, decisions are read in a later kernel), the initial
rows are specified to the bit, and the pooled pull accumulates the same
products in the same order as its reference. Every GPU result is also
computed twice and compared with itself."""

import pytest
import torch

from tfmesos_amd import ops

import test_hash_admit as admit_test
import test_hash_admit_dist as dist_test
import test_hash_index as index_test
import test_hashed_table as table_test

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTHS = [7, 8, 130, 320]   # scalar path, vector path, even but no multiple
                            # of 4, more than one 256-column tile
SEED = admit_test.SEED
EMPTY = ops.HASH_EMPTY


# ------------------------------------------------------- hash_find_or_admit

def check_script(script):
    want = admit_test.run_script(script)
    got = admit_test.run_script(script, DEV)
    admit_test.assert_same(got, want)           # counters included
    admit_test.assert_same(admit_test.run_script(script, DEV), got)


@pytest.mark.parametrize("admit_after", [1, 2, 3])
@pytest.mark.parametrize("n", admit_test.SIZES)
@pytest.mark.parametrize("name", sorted(admit_test.pools()))
def test_admit_matches_cpu_on_request_sizes(name, n, admit_after):
    check_script(admit_test.size_script(name, n, admit_after))


@pytest.mark.parametrize("name", ["duplicate", "full", "early", "saturation",
                                  "contention"])
def test_admit_matches_cpu_on_scripts(name):
    check_script(getattr(admit_test, name + "_script")())


def test_sketch_lives_on_the_device_and_decays():
    sketch = ops.HashAdmission(64, DEV)
    index = ops.HashIndex(8, DEV)
    keys = torch.tensor(index_test.SPECIAL, device=DEV)
    rows, is_new = ops.hash_find_or_admit(index, sketch, keys, 2)
    for t in (rows, is_new, sketch.counters, sketch.filtered):
        assert t.device.type == "cuda"
    assert (rows == -1).all() and int(sketch.filtered) == 5
    before = sketch.counters.clone()
    sketch.decay()
    assert torch.equal(sketch.counters, before // 2)
    with pytest.raises(ValueError):
        ops.hash_find_or_admit(index, ops.HashAdmission(64), keys, 2)


# --------------------------------------------------------- hash_gather_init

def both_cases(D):
    """The same index and table on the CPU and on the GPU."""
    return admit_test.serving_case(D), admit_test.serving_case(D, DEV)


@pytest.mark.parametrize("D", WIDTHS)
def test_gather_init_matches_cpu(D):
    (ci, ct, pool), (gi, gt, _) = both_cases(D)
    gen = torch.Generator().manual_seed(D)
    for n in (1, 63, 64, 65, 257):
        keys = admit_test.mixed_keys(pool, n, gen)
        cs = torch.full((64,), -1, dtype=torch.int64)
        gs = cs.to(DEV)
        want = ops.hash_gather_init(ci, ct, keys, SEED, 3, 2, last_used=cs,
                                    step=n)
        got = ops.hash_gather_init(gi, gt, keys.to(DEV), SEED, 3, 2,
                                   last_used=gs, step=n)
        assert got.dtype == torch.bfloat16 and got.shape == (n, D)
        assert torch.equal(got.cpu(), want)
        assert torch.equal(gs.cpu(), cs)        # stamps: the hits only
        again = ops.hash_gather_init(gi, gt, keys.to(DEV), SEED, 3, 2)
        assert torch.equal(again, got)
        rows = ops.hash_find(ci, keys)
        miss = (rows < 0) & (keys != EMPTY)
        assert n < 63 or (miss.any() and (rows >= 0).any())
        assert (cs >= 0).sum() == rows[rows >= 0].unique().numel()
    assert ops.hash_gather_init(gi, gt, keys[:0].to(DEV), SEED).shape == (0, D)


def test_gather_init_unaligned_table_takes_scalar_path():
    index = ops.HashIndex(16, DEV)
    keys = torch.arange(-5, 15, device=DEV)
    ops.hash_find_or_insert(index, keys[:12])
    flat = torch.randn(16 * 8 + 1).to(torch.bfloat16).to(DEV)
    table = flat[1:].view(16, 8)
    assert table.data_ptr() % 8 == 2
    got = ops.hash_gather_init(index, table, keys, SEED)
    assert torch.equal(got[:12], table[:12])
    assert torch.equal(got[12:].cpu(), ops.hash_init_rows(
        keys[12:].cpu(), 8, SEED).to(torch.bfloat16))


def test_gather_init_probe_chain_longer_than_one_wave():
    """The 70-key chain of test_probe_chain_longer_than_one_wave: 64 keys
    that share home slot 5 fill the table, six more miss at its end."""
    cand = torch.arange(20000)
    chain = cand[ops.hash_home(cand, 128) == 5][:70]
    assert chain.numel() == 70
    gpu = ops.HashIndex(64, DEV)
    ops.hash_find_or_insert(gpu, chain[:64].to(DEV))
    table = torch.arange(64 * 8, device=DEV).view(64, 8).to(torch.bfloat16)
    stamps = torch.zeros(64, dtype=torch.int64, device=DEV)
    got = ops.hash_gather_init(gpu, table, chain.to(DEV), SEED,
                               last_used=stamps, step=3)
    assert torch.equal(got[:64], table) and (stamps == 3).all()
    assert torch.equal(got[64:].cpu(), ops.hash_init_rows(
        chain[64:], 8, SEED).to(torch.bfloat16))
    offsets = torch.tensor([0, 35, 70], device=DEV)
    pooled = ops.hash_embedding_bag(gpu, table, chain.to(DEV), offsets,
                                    out_dtype=torch.float32,
                                    init=(SEED, 1, 0))
    want = admit_test.extended_oracle(gpu, table, chain.to(DEV), offsets,
                                      None, "sum", torch.float32,
                                      (SEED, 1, 0))
    assert torch.equal(pooled, want)


# ------------------------------------------------------- hash_embedding_bag

@pytest.mark.parametrize("init", [None, (SEED, 1, 0), (SEED, 3, 2)],
                         ids=["no_init", "init", "init_shard"])
@pytest.mark.parametrize("D", WIDTHS)
def test_hash_embedding_bag_matches_oracle_and_cpu(D, init):
    (ci, ct, pool), (gi, gt, _) = both_cases(D)
    gen = torch.Generator().manual_seed(7 * D)
    offsets = admit_test.bag_offsets(admit_test.BAG_LENS)
    n = int(offsets[-1])
    keys = admit_test.mixed_keys(pool, n, gen)
    weights = torch.randint(1, 5, (n,), generator=gen).float() / 4
    gk, go, gw = keys.to(DEV), offsets.to(DEV), weights.to(DEV)
    for w, combiner, out_dtype in ((None, "sum", None), (gw, "sum", None),
                                   (gw, "mean", torch.float32),
                                   (None, "mean", None),
                                   (None, "sum", torch.float32)):
        got = ops.hash_embedding_bag(gi, gt, gk, go, w, combiner, out_dtype,
                                     init=init)
        assert got.dtype == (out_dtype or torch.bfloat16)
        assert got.shape == (len(admit_test.BAG_LENS), D)
        # the two-launch sequence over the extended table, on the GPU
        oracle = admit_test.extended_oracle(gi, gt, gk, go, w, combiner,
                                            out_dtype, init)
        assert torch.equal(got, oracle)
        cpu = ops.hash_embedding_bag(
            ci, ct, keys, offsets, None if w is None else weights, combiner,
            out_dtype, init=init)
        assert torch.equal(got.cpu(), cpu)
        assert torch.equal(ops.hash_embedding_bag(
            gi, gt, gk, go, w, combiner, out_dtype, init=init), got)
    cs = torch.full((64,), -1, dtype=torch.int64)
    gs = cs.to(DEV)
    ops.hash_embedding_bag(ci, ct, keys, offsets, init=init, last_used=cs,
                           step=4)
    ops.hash_embedding_bag(gi, gt, gk, go, init=init, last_used=gs, step=4)
    assert torch.equal(gs.cpu(), cs) and (cs == 4).any() and (cs == -1).any()


def test_hash_embedding_bag_unaligned_table_and_no_bags():
    index = ops.HashIndex(16, DEV)
    keys = torch.arange(-5, 15, device=DEV)
    ops.hash_find_or_insert(index, keys[:12])
    flat = admit_test.dyadic(torch.Generator().manual_seed(2),
                             16 * 8 + 1).to(torch.bfloat16).to(DEV)
    table = flat[1:].view(16, 8)
    assert table.data_ptr() % 16 == 2
    offsets = torch.tensor([0, 7, 20], device=DEV)
    init = (SEED, 1, 0)
    got = ops.hash_embedding_bag(index, table, keys, offsets, init=init)
    assert torch.equal(got, admit_test.extended_oracle(
        index, table, keys, offsets, None, "sum", None, init))
    none = ops.hash_embedding_bag(index, table, keys[:0], offsets[:1],
                                  init=init)
    assert none.shape == (0, 8)
    empty = ops.hash_embedding_bag(index, table, keys[:0],
                                   torch.zeros(3, dtype=torch.int64,
                                               device=DEV), init=init)
    assert empty.shape == (2, 8) and not empty.any()


# -------------------------------------------------------------- table level

@pytest.mark.parametrize("optimizer,hparams", table_test.OPTIMIZERS,
                         ids=table_test.OPT_IDS)
def test_admit_after_one_equals_plain_table_on_gpu(optimizer, hparams):
    admit_test.check_admit_one_equals_plain(optimizer, hparams, DEV)


def test_admit_after_three_script_on_gpu():
    admit_test.check_admit_after_three(DEV)


def test_plain_table_is_todays_table():
    table = table_test.make_table("adagrad", {}, DEV)
    assert table.sketch is None
    table.push(index_test.pool97()[:5].to(DEV),
               torch.ones(5, 8, dtype=torch.bfloat16, device=DEV))
    assert table.stats() == {"size": 5, "dropped": 0, "capacity": 128}
    assert sorted(table.state_dict()) == ["keys", "master", "optimizer",
                                          "seed", "state", "step"]


# ---------------------------------------------------------------- end to end

@pytest.mark.timeout(300)
def test_admitting_table_protocol_on_gpu(tmp_path):
    """One PS rank + one worker, both on cuda:0, over gloo, with coalescing
    on. Each process has its own timeout; nothing is started after the
    ranks, and a rank that exits nonzero fails the test before the local
    comparison runs."""
    prefix = str(tmp_path / "run")
    dist_test.run_world(prefix, True, device=DEV, timeout=120)
    dist_test.check_against_local(prefix, device=DEV)
