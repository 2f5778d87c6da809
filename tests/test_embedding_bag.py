"""Pooled (bag) embedding pull / push on the CPU: the references of
ops.embedding_bag and the pooled ops.sparse_* against a naive Python loop
over bags, their argument errors, EmbeddingTable.pull_pooled /
push_pooled, and the worker/server protocol over gloo."""

import os
import subprocess
import sys

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import EmbeddingTable

import _sparse_bag_proc as proc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

V, D = 23, 6
INVALID = [-1, -4, V, V + 2]


def dyadic(gen, *shape):
    return torch.randint(-32, 33, shape, generator=gen).float() / 16


def bags(gen, weighted, lens=(0, 1, 3, 2, 0, 5, 4, 8, 1)):
    n = sum(lens)
    ids = torch.randint(0, V, (n,), generator=gen)
    ids[torch.randperm(n, generator=gen)[:4]] = torch.tensor(INVALID)
    ids[3] = ids[2]                     # the same id twice inside one bag
    offsets = torch.tensor([0] + list(lens)).cumsum(0)
    weights = None
    if weighted:
        weights = torch.tensor([0.5, 1.0, 2.0])[
            torch.randint(0, 3, (n,), generator=gen)]
    return ids, offsets, weights


def naive_coefs(offsets, weights, combiner):
    """[(bag, position, c)] by the definition, one bag at a time."""
    out = []
    for b in range(offsets.numel() - 1):
        pos = range(int(offsets[b]), int(offsets[b + 1]))
        w = [1.0 if weights is None else float(weights[i]) for i in pos]
        W = sum(w)                      # ALL positions, invalid ids too
        for i, wi in zip(pos, w):
            if combiner == "sum":
                c = wi
            else:
                c = wi / W if W != 0 else 0.0
            out.append((b, i, c))
    return out


def naive_bag(table, ids, offsets, weights, combiner):
    out = torch.zeros(offsets.numel() - 1, table.shape[1])
    for b, i, c in naive_coefs(offsets, weights, combiner):
        if 0 <= int(ids[i]) < table.shape[0]:
            out[b] += c * table[int(ids[i])].float()
    return out


def naive_rows(ids, offsets, weights, combiner, g):
    rows = torch.zeros(ids.numel(), g.shape[1])
    for b, i, c in naive_coefs(offsets, weights, combiner):
        rows[i] = c * g[b].float()
    return rows


# ------------------------------------------------------------------ forward

@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
@pytest.mark.parametrize("tdtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
def test_embedding_bag_matches_naive_loop(tdtype, combiner, weighted):
    gen = torch.Generator().manual_seed(1)
    table = dyadic(gen, V, D).to(tdtype)
    ids, offsets, weights = bags(gen, weighted)
    want = naive_bag(table, ids, offsets, weights, combiner)
    out = ops.embedding_bag(table, ids, offsets, weights, combiner)
    assert out.dtype == tdtype and out.shape == (9, D)
    assert torch.allclose(out.float(), want.to(tdtype).float(), atol=1e-6)
    assert (out[0] == 0).all() and (out[4] == 0).all()   # empty bags
    out32 = ops.embedding_bag(table, ids, offsets, weights, combiner,
                              out_dtype=torch.float32)
    assert out32.dtype == torch.float32
    assert torch.allclose(out32, want, atol=1e-6)


def test_embedding_bag_zero_weight_sum_and_invalid_ids_count():
    table = torch.arange(12.0).view(4, 3)
    # bag 0: weights cancel (W == 0 -> all c 0); bag 1: the invalid id
    # still counts in W_b = 2, so the valid row enters with 1/2
    ids = torch.tensor([1, 2, 3, 99])
    offsets = torch.tensor([0, 2, 4])
    w = torch.tensor([1.0, -1.0, 1.0, 1.0])
    out = ops.embedding_bag(table, ids, offsets, w, "mean")
    assert torch.equal(out[0], torch.zeros(3))
    assert torch.equal(out[1], table[3] / 2)


# ------------------------------------------------------------- pooled apply

def run_opt(opt, p, ids, g, st, k, sh, **bag):
    if opt == "sgd":
        ops.sparse_sgd(p, ids, g, 0.1, bf16_out=sh, grad_scale=0.5, **bag)
    elif opt == "sgd_mom":
        ops.sparse_sgd(p, ids, g, 0.1, momentum=0.9, momentum_buf=st[0],
                       weight_decay=0.01, bf16_out=sh, **bag)
    elif opt == "adagrad":
        ops.sparse_adagrad(p, ids, g, st[0], 0.1, bf16_out=sh, **bag)
    else:
        ops.sparse_adam(p, ids, g, st[0], st[1], k, 0.01, bf16_out=sh,
                        **bag)


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("opt", ["sgd", "sgd_mom", "adagrad", "adam"])
def test_pooled_apply_matches_naive_expansion(opt, gdtype):
    """Pooled call == the row call on rows expanded by a Python loop,
    over two steps and all four (combiner, weighted) modes."""
    gen = torch.Generator().manual_seed(2)
    n_state = {"sgd": 0, "sgd_mom": 1, "adagrad": 1, "adam": 2}[opt]
    p0 = torch.rand(V, D, generator=gen)
    st0 = [torch.rand(V, D, generator=gen) * 0.5 for _ in range(n_state)]
    for combiner in ("sum", "mean"):
        for weighted in (False, True):
            got = [p0.clone(), torch.zeros(V, D, dtype=torch.bfloat16)] + \
                [s.clone() for s in st0]
            want = [t.clone() for t in got]
            for k in (1, 2):
                ids, offsets, weights = bags(gen, weighted)
                g = dyadic(gen, 9, D).to(gdtype)
                run_opt(opt, got[0], ids, g, got[2:], k, got[1],
                        offsets=offsets, weights=weights, combiner=combiner)
                rows = naive_rows(ids, offsets, weights, combiner, g)
                run_opt(opt, want[0], ids, rows, want[2:], k, want[1])
            for a, b in zip(got, want):
                assert torch.allclose(a.float(), b.float(), atol=1e-6)
            assert not torch.equal(got[0], p0)
            untouched = torch.ones(V, dtype=torch.bool)
            untouched[ids[(ids >= 0) & (ids < V)]] = False
            assert untouched.any()


def test_pooled_sgd_matches_direct_formula():
    gen = torch.Generator().manual_seed(3)
    p0 = torch.rand(V, D, generator=gen)
    ids, offsets, weights = bags(gen, True)
    g = dyadic(gen, 9, D)
    p = p0.clone()
    ops.sparse_sgd(p, ids, g, 0.1, grad_scale=0.5, offsets=offsets,
                   weights=weights, combiner="mean")
    want = p0.clone()
    for b, i, c in naive_coefs(offsets, weights, "mean"):
        if 0 <= int(ids[i]) < V:
            want[int(ids[i])] -= 0.1 * 0.5 * c * g[b]
    assert torch.allclose(p, want, atol=1e-6)


def test_adagrad_opposite_bag_gradients_cancel():
    """ids [3, 3] in two bags with gradients g and -g: the row's summed
    gradient is 0, so row and accumulator do not move."""
    p = torch.rand(5, 4)
    a = torch.rand(5, 4)
    p0, a0 = p.clone(), a.clone()
    g = torch.tensor([[1.5, -2.0, 0.25, 3.0]])
    ops.sparse_adagrad(p, torch.tensor([3, 3]), torch.cat([g, -g]), a, 0.1,
                       offsets=torch.tensor([0, 1, 2]))
    assert torch.equal(p, p0) and torch.equal(a, a0)


# ------------------------------------------------------------------- errors

@pytest.mark.parametrize("offsets", [[1, 2, 4], [0, 3, 2, 4], [0, 2, 3],
                                     [0, 2, 5]],
                         ids=["first_not_0", "decreasing", "last_short",
                              "last_long"])
def test_bad_offsets_raise(offsets):
    table = torch.rand(V, D)
    ids = torch.tensor([1, 2, 3, 4])
    offsets = torch.tensor(offsets)
    B = offsets.numel() - 1
    with pytest.raises(ValueError):
        ops.embedding_bag(table, ids, offsets)
    for call in (
            lambda: ops.sparse_sgd(table, ids, torch.rand(B, D), 0.1,
                                   offsets=offsets),
            lambda: ops.sparse_adagrad(table, ids, torch.rand(B, D),
                                       torch.zeros(V, D), 0.1,
                                       offsets=offsets),
            lambda: ops.sparse_adam(table, ids, torch.rand(B, D),
                                    torch.zeros(V, D), torch.zeros(V, D), 1,
                                    0.1, offsets=offsets)):
        with pytest.raises(ValueError):
            call()


def test_bad_combiner_weights_and_dtype_raise():
    table = torch.rand(V, D)
    ids = torch.tensor([1, 2, 3, 4])
    offsets = torch.tensor([0, 2, 4])
    g = torch.rand(2, D)
    with pytest.raises(ValueError):
        ops.embedding_bag(table, ids, offsets, combiner="sqrtn")
    with pytest.raises(ValueError):
        ops.embedding_bag(table, ids, offsets, weights=torch.ones(3))
    with pytest.raises(ValueError):
        ops.embedding_bag(table, ids, offsets, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.sparse_sgd(table, ids, g, 0.1, offsets=offsets, combiner="max")
    with pytest.raises(ValueError):
        ops.sparse_adagrad(table, ids, g, torch.zeros(V, D), 0.1,
                           offsets=offsets, weights=torch.ones(5))
    with pytest.raises(ValueError):     # weights without offsets
        ops.sparse_sgd(table, ids, torch.rand(4, D), 0.1,
                       weights=torch.ones(4))
    with pytest.raises(ValueError):     # one gradient row per BAG
        ops.sparse_sgd(table, ids, torch.rand(4, D), 0.1, offsets=offsets)


# --------------------------------------------- row calls stay what they were

def row_calls():
    """Row-mode (no ``offsets``) sparse applies on fixed dyadic inputs:
    {name: tensor} of every tensor they leave behind."""
    gen = torch.Generator().manual_seed(4)
    out = {}
    for opt in ("sgd", "sgd_mom", "adagrad", "adam"):
        n_state = {"sgd": 0, "sgd_mom": 1, "adagrad": 1, "adam": 2}[opt]
        p = dyadic(gen, V, D)
        st = [dyadic(gen, V, D).abs() for _ in range(n_state)]
        sh = torch.zeros(V, D, dtype=torch.bfloat16)
        for k in (1, 2):
            ids = torch.cat([torch.randint(0, V, (30,), generator=gen),
                             torch.tensor(INVALID)])
            g = dyadic(gen, 34, D)
            if opt in ("sgd", "sgd_mom"):
                ops.sparse_sgd(p, ids, g, 0.5, bf16_out=sh, grad_scale=0.5,
                               momentum=0.5 if st else 0.0,
                               momentum_buf=st[0] if st else None)
            elif opt == "adagrad":
                ops.sparse_adagrad(p, ids, g, st[0], 0.5, bf16_out=sh,
                                   grad_scale=0.5)
            else:
                ops.sparse_adam(p, ids, g, st[0], st[1], k, 0.5, beta1=0.5,
                                beta2=0.5, bf16_out=sh, grad_scale=0.5)
        for name, t in zip(["master", "shadow", "s1", "s2"], [p, sh] + st):
            out["%s_%s" % (opt, name)] = t.float()
    return out


def test_row_calls_are_what_they_were(monkeypatch):
    """Calls without ``offsets`` equal a saved copy of the same calls made
    before any pooled call, and never enter the bag code. (A copy saved to
    a file does not serve: the CPU references' sqrt / divide chains differ
    in the last bit from one CPU model to the next.)"""
    saved = row_calls()
    gen = torch.Generator().manual_seed(7)
    ids, offsets, weights = bags(gen, True)
    table = dyadic(gen, V, D)
    ops.embedding_bag(table, ids, offsets, weights, "mean")
    ops.sparse_adagrad(table, ids, dyadic(gen, 9, D), torch.zeros(V, D), 0.1,
                       offsets=offsets, weights=weights, combiner="mean")

    def no_bags(*a, **k):
        raise AssertionError("row call reached the bag code")
    monkeypatch.setattr(ops, "_bag_expand_cpu", no_bags)
    monkeypatch.setattr(ops, "_bag_rows_cpu", no_bags)
    monkeypatch.setattr(ops, "_bag_check", no_bags)
    now = row_calls()
    assert sorted(saved) == sorted(now) and len(now) == 12
    for name, t in now.items():
        assert torch.equal(t, saved[name]), name


# ----------------------------------------------------------- EmbeddingTable

@pytest.mark.parametrize("optimizer,hp", [
    ("sgd", {}), ("sgd", {"momentum": 0.9}), ("adagrad", {}), ("adam", {})],
    ids=["sgd_unfused", "sgd_mom", "adagrad", "adam"])
def test_table_pooled_semantics_and_state_dict(optimizer, hp):
    kw = dict(rows=V, dim=D, lr=0.1, seed=3, optimizer=optimizer, **hp)
    t = EmbeddingTable("t", **kw)
    gen = torch.Generator().manual_seed(5)
    ids, offsets, weights = bags(gen, True)
    pulled = t.pull_pooled(ids, offsets, weights, "mean")
    assert pulled.dtype == torch.bfloat16 and pulled.shape == (9, D)
    assert torch.equal(pulled, ops.embedding_bag(t.shadow, ids, offsets,
                                                 weights, "mean"))
    master0 = t.master.clone()
    g = dyadic(gen, 9, D).to(torch.bfloat16)
    t.push_pooled(ids, offsets, g, weights, "mean")
    t.push_pooled(ids, offsets, g, combiner="sum", lr=0.05)
    assert t.step == 2                  # once per push, fused or not
    # the same two pushes as row pushes of the expanded rows on a table
    # that always takes the fused path
    ref = EmbeddingTable("t", **dict(kw, **(
        {"fused_apply": True} if optimizer == "sgd" else {})))
    ref.push(ids, naive_rows(ids, offsets, weights, "mean", g))
    ref.push(ids, naive_rows(ids, offsets, None, "sum", g), lr=0.05)
    assert torch.allclose(t.master, ref.master, atol=1e-6)
    for k in t.state:
        assert torch.allclose(t.state[k], ref.state[k], atol=1e-6)
    good = ids[(ids >= 0) & (ids < V)]
    idle = torch.ones(V, dtype=torch.bool)
    idle[good] = False
    assert torch.equal(t.master[idle], master0[idle])
    assert not torch.equal(t.master[good], master0[good])
    assert torch.equal(t.shadow, t.master.to(torch.bfloat16))
    # round trip: a restored table continues bit-identically
    t2 = EmbeddingTable("t", **dict(kw, seed=99))
    t2.load_state_dict(t.state_dict())
    assert t2.step == 2 and torch.equal(t2.shadow, t.shadow)
    for tab in (t, t2):
        tab.push_pooled(ids, offsets, g, weights, "sum")
    assert torch.equal(t2.master, t.master)
    for k in t.state:
        assert torch.equal(t2.state[k], t.state[k])
    assert torch.equal(t2.pull_pooled(ids, offsets), t.pull_pooled(ids,
                                                                  offsets))


# ----------------------------------------------------------------- protocol

@pytest.mark.timeout(240)
@pytest.mark.parametrize("world", [2, 3], ids=["one_ps", "two_ps"])
def test_pooled_protocol_over_gloo(world, tmp_path):
    """One worker interleaves row and pooled pulls / pushes (weighted and
    unweighted, both combiners); the PS ranks must end with the state of
    local tables given the same requests, and the worker must have pulled
    the same tensors."""
    from tfmesos_amd.utils import free_port
    port = free_port()
    pulls = str(tmp_path / "pulls.pt")
    procs = []
    for rank in range(world):
        env = dict(os.environ)
        env.update({
            "RANK": str(rank), "WORLD_SIZE": str(world),
            "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
            "PYTHONPATH": REPO,
            # CPU + gloo is what this test covers, also on a GPU box
            "HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1",
        })
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, "_sparse_bag_proc.py"),
             pulls], env=env, stdout=subprocess.PIPE, text=True))
    sums = {}
    try:
        for p in procs:
            out, _ = p.communicate(timeout=180)
            assert p.returncode == 0, out
            for line in out.splitlines():
                if line.startswith("CHECKSUM"):
                    _, name, digest = line.split()
                    sums[name] = digest
    finally:
        # a rank that died must not leave its peers waiting behind
        for p in procs:
            if p.poll() is None:
                p.kill()
    local = {t.name: t for t in proc.make_tables(sorted(proc.TABLES))}
    init = {n: proc.checksum(t) for n, t in local.items()}
    want = proc.apply_local(local, proc.requests())
    assert sums == {n: proc.checksum(t) for n, t in local.items()}
    assert all(sums[n] != init[n] for n in sums)
    got = torch.load(pulls)
    assert len(got) == len(want) == 24
    for a, b in zip(got, want):
        assert a.dtype == torch.bfloat16 and torch.equal(a, b)
