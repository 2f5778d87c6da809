"""Sparse optimizer applies (ops.sparse_sgd / sparse_adagrad /
sparse_adam), the EmbeddingTable optimizers built on them and the sparse
PS server with an Adagrad table — CPU reference path.

Inputs follow the dyadic recipe: grads are randint(-32, 33)/16 (exact in
bf16, fp32 sums exact in any order) and grad_scale is 0.5 or 1, so the
summation order can never excuse a mismatch."""

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import EmbeddingTable, SparsePSServer

OPTS = ["sgd", "sgd_mom", "adagrad", "adam"]
N_STATE = {"sgd": 0, "sgd_mom": 1, "adagrad": 1, "adam": 2}


def dyadic(gen, *shape):
    return torch.randint(-32, 33, shape, generator=gen).float() / 16


def sparse_step(opt, p, ids, g, st, step, bf16_out=None, grad_scale=1.0):
    if opt == "sgd":
        ops.sparse_sgd(p, ids, g, 0.1, weight_decay=0.01, bf16_out=bf16_out,
                       grad_scale=grad_scale)
    elif opt == "sgd_mom":
        ops.sparse_sgd(p, ids, g, 0.1, momentum=0.9, momentum_buf=st[0],
                       bf16_out=bf16_out, grad_scale=grad_scale)
    elif opt == "adagrad":
        ops.sparse_adagrad(p, ids, g, st[0], 0.1, bf16_out=bf16_out,
                           grad_scale=grad_scale)
    else:
        ops.sparse_adam(p, ids, g, st[0], st[1], step, 0.01,
                        bf16_out=bf16_out, grad_scale=grad_scale)


def dense_step(opt, p, g, st, step, grad_scale=1.0):
    if opt == "sgd":
        ops.fused_sgd(p, g, 0.1, weight_decay=0.01, grad_scale=grad_scale)
    elif opt == "sgd_mom":
        ops.fused_sgd(p, g, 0.1, momentum=0.9, momentum_buf=st[0],
                      grad_scale=grad_scale)
    elif opt == "adagrad":
        ops.fused_adagrad(p, g, st[0], 0.1, grad_scale=grad_scale)
    else:
        ops.fused_adam(p, g, st[0], st[1], step, 0.01,
                       grad_scale=grad_scale)


def make(opt, V, D, seed=0):
    gen = torch.Generator().manual_seed(seed)
    p = torch.rand(V, D, generator=gen)
    st = [torch.rand(V, D, generator=gen) * 0.5 for _ in range(N_STATE[opt])]
    return gen, p, st


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_cancellation(opt):
    """ids [3,3] with grads g,-g: summed gradient 0 -> nothing moves
    (an accumulate-per-contribution design would add 2*g^2)."""
    gen = torch.Generator().manual_seed(1)
    p = torch.rand(6, 8, generator=gen)
    st = [torch.zeros(6, 8) for _ in range(N_STATE[opt])]
    p0, st0 = p.clone(), [s.clone() for s in st]
    g = dyadic(gen, 1, 8)
    sparse_step(opt, p, torch.tensor([3, 3]), torch.cat([g, -g]), st, 1)
    assert torch.equal(p, p0)
    for s, s0 in zip(st, st0):
        assert torch.equal(s, s0)


@pytest.mark.parametrize("opt", OPTS)
def test_dense_parity(opt):
    V, D = 50, 200
    gen, p, st = make(opt, V, D)
    pd, std = p.clone(), [s.clone() for s in st]
    ids = torch.arange(V)
    for step in (1, 2):
        g = dyadic(gen, V, D)
        sparse_step(opt, p, ids, g, st, step, grad_scale=0.5)
        dense_step(opt, pd.view(-1), g.view(-1), [s.view(-1) for s in std],
                   step, grad_scale=0.5)
    assert torch.equal(p, pd)
    for s, sd in zip(st, std):
        assert torch.equal(s, sd)


@pytest.mark.parametrize("opt", OPTS)
def test_out_of_range_ids_ignored(opt):
    V, D = 20, 8
    gen, p, st = make(opt, V, D)
    pc, stc = p.clone(), [s.clone() for s in st]
    sh = p.to(torch.bfloat16)
    shc = sh.clone()
    good = torch.tensor([3, 7, 3, 0, 19, 7])
    g = dyadic(gen, 6, D)
    bad = torch.tensor([-1, -5, V, V + 3])
    order = torch.tensor([6, 0, 1, 7, 2, 3, 8, 4, 5, 9])
    ids = torch.cat([good, bad])[order]
    gg = torch.cat([g, dyadic(gen, 4, D)])[order]
    sparse_step(opt, p, ids, gg, st, 1, bf16_out=sh)
    sparse_step(opt, pc, good, g, stc, 1, bf16_out=shc)
    assert torch.equal(p, pc) and torch.equal(sh, shc)
    for s, sc in zip(st, stc):
        assert torch.equal(s, sc)
    assert torch.equal(sh[good], p[good].to(torch.bfloat16))


@pytest.mark.parametrize("opt", OPTS)
def test_empty_and_all_invalid_are_noops(opt):
    V, D = 10, 8
    gen, p, st = make(opt, V, D)
    p0, st0 = p.clone(), [s.clone() for s in st]
    sh = torch.zeros(V, D, dtype=torch.bfloat16)
    sparse_step(opt, p, torch.zeros(0, dtype=torch.int64), torch.zeros(0, D),
                st, 1, bf16_out=sh)
    sparse_step(opt, p, torch.tensor([-1, V, V + 3, -5]), dyadic(gen, 4, D),
                st, 1, bf16_out=sh)
    assert torch.equal(p, p0) and not sh.any()
    for s, s0 in zip(st, st0):
        assert torch.equal(s, s0)


def test_momentum_needs_buffer():
    with pytest.raises(ValueError):
        ops.sparse_sgd(torch.zeros(4, 4), torch.tensor([1]),
                       torch.ones(1, 4), 0.1, momentum=0.9)


# ------------------------------------------------------------ EmbeddingTable

TABLE_CFG = {
    "sgd_fused": ("sgd", {"fused_apply": True}),
    "sgd_mom": ("sgd", {"momentum": 0.9}),
    "adagrad": ("adagrad", {"weight_decay": 0.01}),
    "adam": ("adam", {"beta1": 0.8}),
}


def _table(cfg, **kw):
    opt, hp = TABLE_CFG[cfg]
    return EmbeddingTable("t", rows=30, dim=8, lr=0.1, seed=5, optimizer=opt,
                          **dict(hp, **kw))


def _pushes(k, seed=11):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(k):
        ids = torch.randint(0, 12, (9,), generator=gen)
        out.append((ids, dyadic(gen, 9, 8).to(torch.bfloat16)))
    return out


@pytest.mark.parametrize("cfg", sorted(TABLE_CFG))
def test_table_matches_hand_replay(cfg):
    t = _table(cfg)
    opt, hp = TABLE_CFG[cfg]
    p = t.master.clone()
    st = [torch.zeros_like(p) for _ in t.state]
    assert all(s.shape == (30, 8) and s.dtype == torch.float32
               for s in t.state.values())
    for step, (ids, g) in enumerate(_pushes(3), 1):
        t.push(ids, g)
        if opt == "sgd":
            ops.sparse_sgd(p, ids, g, 0.1, momentum=hp.get("momentum", 0.0),
                           momentum_buf=st[0] if st else None)
        elif opt == "adagrad":
            ops.sparse_adagrad(p, ids, g, st[0], 0.1, weight_decay=0.01)
        else:
            ops.sparse_adam(p, ids, g, st[0], st[1], step, 0.1, beta1=0.8)
        assert torch.equal(t.master, p)
        assert torch.equal(t.pull(ids), t.master[ids].to(torch.bfloat16))
    for s, (k, v) in zip(st, t.state.items()):
        assert torch.equal(s, v), k
    if opt == "adam":
        assert t.step == 3


def test_default_table_keeps_scatter_add_path():
    t = EmbeddingTable("t", rows=30, dim=8)
    assert t.optimizer == "sgd" and not t.fused and not t.state


def test_unknown_optimizer_raises():
    with pytest.raises(ValueError):
        EmbeddingTable("t", rows=4, dim=4, optimizer="ftrl")
    with pytest.raises(ValueError):
        EmbeddingTable("t", rows=4, dim=4, optimizer="adagrad", momentum=0.5)


@pytest.mark.parametrize("cfg", sorted(TABLE_CFG))
def test_state_dict_roundtrip(cfg):
    pushes = _pushes(4)
    a = _table(cfg)
    for ids, g in pushes[:3]:
        a.push(ids, g)
    sd = a.state_dict()
    b = _table(cfg)
    b.push(*pushes[3])                       # diverge b before loading
    master_buf, shadow_buf = b.master, b.shadow
    b.load_state_dict(sd)
    assert b.master is master_buf and b.shadow is shadow_buf
    assert torch.equal(b.master, a.master) and b.step == a.step
    assert torch.equal(b.shadow, a.master.to(torch.bfloat16))
    for k in a.state:
        assert torch.equal(b.state[k], a.state[k])
    # the snapshot is a copy, not a view of the live table
    a.push(*pushes[3])
    assert not torch.equal(sd["master"], a.master)
    b.push(*pushes[3])
    assert torch.equal(b.master, a.master)
    assert torch.equal(b.shadow, a.shadow)
    for k in a.state:
        assert torch.equal(b.state[k], a.state[k])


def test_load_state_dict_rejects_other_optimizer():
    sd = _table("adagrad").state_dict()
    with pytest.raises(ValueError):
        _table("adam").load_state_dict(sd)


# -------------------------------------------------------------------- server

class FakeWork(object):
    def __init__(self, chan):
        self.chan = chan
        self.done = False

    def is_completed(self):
        if not self.done:
            self.done = self.chan._try_fill()
        return self.done


class FakeChan(object):
    """Scripted peer (the pattern of test_polling_serve.py): ``script``
    is what the peer sends in order; server sends are recorded."""

    def __init__(self, script):
        self.script = list(script)
        self.sent = []
        self._pending = None
        self.device_only = True

    def _try_fill(self):
        if self._pending is None:
            return True
        if not self.script:
            return False
        self._pending.copy_(self.script.pop(0))
        self._pending = None
        return True

    def irecv_into(self, t):
        assert self._pending is None
        self._pending = t
        return FakeWork(self)

    def recv_new(self, shape, dtype, device):
        assert self._pending is None and self.script, "blocking recv starved"
        t = torch.empty(shape, dtype=dtype, device=device)
        t.copy_(self.script.pop(0))
        return t

    def send(self, t):
        self.sent.append(t.detach().clone())


def test_sparse_polling_server_with_adagrad_table():
    tbl = EmbeddingTable("W", rows=10, dim=8, lr=0.5, seed=3,
                         optimizer="adagrad")
    local = EmbeddingTable("W", rows=10, dim=8, lr=0.5, seed=3,
                           optimizer="adagrad")
    gen = torch.Generator().manual_seed(2)
    ids = torch.tensor([1, 3, 1, 9])
    grads = dyadic(gen, 4, 8).to(torch.bfloat16)
    pull_hdr = torch.tensor([4, 0], dtype=torch.int64)
    push_hdr = torch.tensor([-4, 0], dtype=torch.int64)
    stop_hdr = torch.tensor([0, 0], dtype=torch.int64)
    chans = {
        (0, 1): FakeChan([pull_hdr, ids, push_hdr, ids, grads,
                          pull_hdr, ids, stop_hdr]),
        (0, 2): FakeChan([stop_hdr]),
    }
    srv = SparsePSServer(0, [tbl], [1, 2], chans)
    srv.device = torch.device("cpu")
    srv._serve_polling()
    before = local.pull(ids)
    local.push(ids, grads)
    sent = chans[(0, 1)].sent
    assert len(sent) == 2
    assert torch.equal(sent[0], before)
    assert torch.equal(sent[1], local.pull(ids))
    assert not torch.equal(sent[0], sent[1])
    assert torch.equal(tbl.master, local.master)
    assert torch.equal(tbl.state["accum"], local.state["accum"])
