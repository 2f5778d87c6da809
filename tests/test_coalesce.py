"""Worker-side coalescing of row requests on the CPU: the references of
ops.coalesce_ids / ops.segment_sum_rows against plain Python loops, and the
``coalesce=`` mode of SparseWorkerClient over gloo against local tables fed
the UNCOALESCED script."""

import os
import subprocess
import sys

import pytest
import torch

from tfmesos_amd import ops

import _sparse_coalesce_proc as proc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

V = 9       # ids_case draws 12 values, -2 .. 9: negative ids and ids >= V


# -------------------------------------------------------------- coalesce_ids

def ids_case(n, kind):
    gen = torch.Generator().manual_seed(100 + n)
    if kind == "distinct":
        return torch.randperm(n, generator=gen) * 3 - 4
    if kind == "equal":
        return torch.full((n,), 7, dtype=torch.int64)
    return torch.randint(-2, V + 1, (n,), generator=gen)


def naive_coalesce(ids):
    """(uniq, inverse, perm, seg, u) by a dict loop over the positions."""
    where = {}
    for i, v in enumerate(ids.tolist()):
        where.setdefault(v, []).append(i)
    keys = sorted(where)
    n, u = ids.numel(), len(keys)
    inverse = [0] * n
    perm, seg = [], []
    for k, v in enumerate(keys):
        seg.append(len(perm))
        perm += where[v]
        for i in where[v]:
            inverse[i] = k
    return (keys + [-1] * (n - u), inverse, perm, seg + [n] * (n + 1 - u), u)


@pytest.mark.parametrize("kind", ["distinct", "equal", "random"])
@pytest.mark.parametrize("n", [0, 1, 2, 65, 300])
def test_coalesce_ids_matches_naive_loop(n, kind):
    ids = ids_case(n, kind)
    co = ops.coalesce_ids(ids)
    uniq, inverse, perm, seg, u = naive_coalesce(ids)
    for t, shape in zip(co, [(n,), (n,), (n,), (n + 1,), (1,)]):
        assert t.dtype == torch.int64 and tuple(t.shape) == shape
    assert co.uniq.tolist() == uniq
    assert co.inverse.tolist() == inverse
    assert co.perm.tolist() == perm
    assert co.seg.tolist() == seg
    assert co.count.tolist() == [u]
    # the invariants, stated on their own
    assert torch.equal(co.uniq[co.inverse], ids)
    assert bool((co.uniq[1:u] > co.uniq[:u - 1]).all())
    assert bool((co.uniq[u:] == -1).all())
    assert bool((co.seg[1:] >= co.seg[:-1]).all())
    assert bool((co.seg[u:] == n).all())
    for k in range(u):
        group = co.perm[int(co.seg[k]):int(co.seg[k + 1])]
        assert bool((ids[group] == co.uniq[k]).all())
        assert bool((group[1:] > group[:-1]).all())      # stable
    if kind == "random" and n >= 65:
        assert 1 < u < n and int(ids.min()) < 0 and int(ids.max()) >= V


# ---------------------------------------------------------- segment_sum_rows

DTYPES = [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16),
          (torch.float32, torch.float32)]
DTYPE_IDS = ["f32_bf16", "bf16_bf16", "f32_f32"]


def dyadic(gen, *shape):
    """randint(-32, 33)/16: exact in bf16, and every sum of up to 300 of
    them is exact in fp32 in any order."""
    return torch.randint(-32, 33, shape, generator=gen).float() / 16


@pytest.mark.parametrize("dtypes", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", [0, 1, 2, 65, 300])
def test_segment_sum_rows_matches_per_id_loop(n, dtypes):
    src, dst = dtypes
    D = 5
    gen = torch.Generator().manual_seed(200 + n)
    ids = ids_case(n, "random")
    rows = dyadic(gen, n, D).to(src)
    co = ops.coalesce_ids(ids)
    u = int(co.count)
    got = ops.segment_sum_rows(rows, co.perm, co.seg, u, dst)
    assert got.dtype == dst and got.shape == (u, D)
    for k in range(u):
        want = torch.zeros(D)
        for i in range(n):
            if int(ids[i]) == int(co.uniq[k]):
                want += rows[i].float()
        assert torch.equal(got[k], want.to(dst)), k
    # out_dtype defaults to the rows' dtype
    assert ops.segment_sum_rows(rows, co.perm, co.seg, u).dtype == src
    if n == 300:    # 12 values over 300 positions: every row is a real sum
        assert u == 12


def test_argument_errors():
    ids = torch.tensor([3, 1, 3])
    co = ops.coalesce_ids(ids)
    rows = torch.zeros(3, 4)
    with pytest.raises(ValueError):
        ops.coalesce_ids(ids.to(torch.int32))           # non-int64 ids
    with pytest.raises(ValueError):
        ops.coalesce_ids(ids.view(1, 3))                # 2-D ids
    with pytest.raises(ValueError):
        ops.segment_sum_rows(torch.zeros(4, 4), co.perm, co.seg, 2)
    with pytest.raises(ValueError):
        ops.segment_sum_rows(rows.double(), co.perm, co.seg, 2)
    with pytest.raises(ValueError):
        ops.segment_sum_rows(rows, co.perm, co.seg, 2, torch.float16)
    with pytest.raises(ValueError):
        ops.segment_sum_rows(rows, co.perm, co.seg, 4)  # seg holds 4 entries
    assert ops.segment_sum_rows(rows, co.perm, co.seg, 2).shape == (2, 4)


# ----------------------------------------------------------------- over gloo

def run_world(world, pulls, coalesce=True, device="cpu", timeout=180):
    """Start the ranks; return ({"T/shard": digest}, {"T/shard": [(kind,
    ids)]}) printed by the PS ranks. A rank that fails ends the run: its
    peers are killed."""
    from tfmesos_amd.utils import free_port
    port = free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ)
        env.update({
            "RANK": str(rank), "WORLD_SIZE": str(world),
            "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
            "PYTHONPATH": REPO, "COALESCE_PROC_DEVICE": device,
            "COALESCE_PROC_ON": "1" if coalesce else "0",
        })
        if device == "cpu":
            # CPU + gloo is what this covers, also on a GPU box
            env.update({"HIP_VISIBLE_DEVICES": "-1",
                        "CUDA_VISIBLE_DEVICES": "-1"})
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, "_sparse_coalesce_proc.py"),
             pulls], env=env, stdout=subprocess.PIPE, text=True))
    sums, seen = {}, {}
    try:
        for p in procs:
            out, _ = p.communicate(timeout=timeout)     # per process
            assert p.returncode == 0, out
            for line in out.splitlines():
                if line.startswith("CHECKSUM"):
                    _, name, digest = line.split()
                    sums[name] = digest
                elif line.startswith("SEEN"):
                    _, name, kind, count = line.split()
                    seen.setdefault(name, []).append((kind, int(count)))
    finally:
        # a rank that died must not leave its peers waiting behind
        for p in procs:
            if p.poll() is None:
                p.kill()
    return sums, seen


def check_against_local(world, sums, pulls, device="cpu"):
    """(i) checksums (master, state, step) and (ii) pulls equal a local
    table given the uncoalesced script."""
    reqs = proc.requests(world)
    local = proc.make_local(world, device)
    init = proc.local_checksums(local)
    want = proc.apply_local(local, reqs, device)
    assert sums == proc.local_checksums(local)
    assert all(sums[k] != init[k] for k in sums)
    got = torch.load(pulls)
    assert len(got) == len(want) == sum(
        1 for r in reqs if r[0].startswith("pull"))
    for a, b in zip(got, want):
        assert a.dtype == torch.bfloat16 and a.shape == (proc.N, proc.DIM)
        assert torch.equal(a, b.cpu())
    return local, reqs


def check_seen(world, seen, coalesce):
    """(iii) / (iv): the PS tables were handed the distinct ids of every
    request, fewer than its positions — or every position without
    ``coalesce``."""
    assert seen == proc.expected_seen(world, coalesce)
    reqs = proc.requests(world)
    handed = sum(c for calls in seen.values() for _, c in calls)
    if coalesce:
        assert all(proc.distinct(r[1]) < r[1].numel() for r in reqs)
        assert handed == sum(proc.distinct(r[1]) for r in reqs)
    else:
        assert handed == sum(r[1].numel() for r in reqs)


@pytest.mark.timeout(240)
@pytest.mark.parametrize("coalesce", [True, False], ids=["coalesce", "plain"])
@pytest.mark.parametrize("world", [2, 3], ids=["unsharded_adagrad",
                                               "mod_2ps_adam"])
def test_coalesced_protocol_over_gloo(world, coalesce, tmp_path):
    pulls = str(tmp_path / "pulls.pt")
    sums, seen = run_world(world, pulls, coalesce)
    assert sorted(sums) == ["T/%d" % s for s in range(world - 1)]
    local, reqs = check_against_local(world, sums, pulls)
    check_seen(world, seen, coalesce)
    n_push = sum(1 for r in reqs if r[0].startswith("push"))
    if world == 3:      # every shard stepped once per push, also the
        assert [t.step for t in local.shards] == [n_push] * 2   # one-shard one
        assert ("push", 0) in seen["T/1"]
    else:
        assert local.step == n_push
