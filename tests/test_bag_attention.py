"""ops.bag_attention on the CPU: the fp32 torch reference, forward and
backward, against an fp64 oracle (masked_fill(-inf), softmax, autograd, one
bag at a time; a query whose bag has no keys gives a zero row and no
gradient).

Inputs: rows are multiples of 1/16 in [-1/4, 1/4], dout multiples of 1/8 in
[-1, 1], scale a power of two (0.25, or the default 2^-3 at D = 64): every
scaled score is a multiple of 2^-12 below 2^1, exact in fp32 in any
summation order.

Bounds (derived, componentwise; bf16 has 8 significant bits, unit roundoff
2^-8; T = 2^-7 + 2^-16; p, dS the fp64 values, dS = scale p (dP - delta)):
  out: T A, A = sum_j p |v_j| — one bf16 rounding of P~ (2^-8 A), one of the
    result (2^-8 A), 2^-16 for the fp32 exp, sum and division.
  dv:  T A, A = sum_i p |dout_i| — the same two roundings.
  dq:  T sum_j |dS| |k_j| + (1 + 2^-7) scale eps_i sum_j p |k_j|. delta is
    formed from the rounded out, so it is off by eps_i <= T sum_d |dout_id|
    A_out,id, which moves dS by scale p eps_i before dS is rounded (2^-8) and
    the result is rounded (2^-8): the second term.
  dk:  the same with i / j and q / k exchanged:
    T sum_i |dS| |q_i| + (1 + 2^-7) scale sum_i eps_i p |q_i|.
Every bound is positive on the rows that have a partner (a query with keys,
a key with queries); check asserts it.
"""

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.ps.sparse import EmbeddingTable

T = 2.0 ** -7 + 2.0 ** -16
QL = (0, 1, 63, 64, 65, 130)    # an empty bag, one row, the tile edges, tiles
KL = (5, 0, 64, 130, 1, 65)     # keys without queries, queries without keys


def make(ql, kl, H, D, seed=0):
    """dict of q, k, v, offsets, kv_offsets (None when kl is None), dout."""
    gen = torch.Generator().manual_seed(seed)
    row = lambda n: (torch.randint(-4, 5, (n, H, D), generator=gen) / 16).to(  # noqa: E731
        torch.bfloat16)
    off = lambda ls: torch.tensor((0,) + tuple(ls)).cumsum(0)  # noqa: E731
    n, m = sum(ql), sum(ql if kl is None else kl)
    dout = (torch.randint(-8, 9, (n, H, D), generator=gen) / 8).to(
        torch.bfloat16)
    return dict(q=row(n), k=row(m), v=row(m), offsets=off(ql),
                kv_offsets=None if kl is None else off(kl), dout=dout)


def oracle(inp, causal=False, scale=0.25):
    """fp64: out, the gradients of q, k, v, the bounds of all four, and the
    rows that have a partner (of q and of k)."""
    x = {n: inp[n].detach().double().cpu().requires_grad_(True) for n in "qkv"}
    q, k, v = x["q"], x["k"], x["v"]
    g = inp["dout"].double().cpu()
    qo = inp["offsets"].tolist()
    ko = qo if inp["kv_offsets"] is None else inp["kv_offsets"].tolist()
    out = torch.zeros(q.shape, dtype=torch.float64)
    bnd = {n: torch.zeros(x[n[-1]].shape, dtype=torch.float64)
           for n in ("out_q", "q", "k", "v")}
    live = {n: torch.zeros(x[n].shape[0], dtype=torch.bool) for n in "qk"}
    for b in range(len(qo) - 1):
        i, j = slice(qo[b], qo[b + 1]), slice(ko[b], ko[b + 1])
        if i.start == i.stop or j.start == j.stop:
            continue
        s = scale * torch.einsum("ihd,jhd->hij", q[i], k[j])
        if causal:
            s = s.masked_fill(torch.ones(s.shape[1:]).triu(1).bool(),
                              float("-inf"))
        p = torch.softmax(s, -1)
        out[i] = torch.einsum("hij,jhd->ihd", p, v[j])
        with torch.no_grad():
            qa, ka, va, ga = q[i].abs(), k[j].abs(), v[j].abs(), g[i].abs()
            a_out = torch.einsum("hij,jhd->ihd", p, va)
            eps = (T * (ga * a_out).sum(-1)).t()[:, :, None]       # [h,i,1]
            delta = (g[i] * out[i]).sum(-1).t()[:, :, None]
            ds = (scale * p * (torch.einsum("ihd,jhd->hij", g[i], v[j])
                               - delta)).abs()
            pe = (1 + 2.0 ** -7) * scale * p * eps
            bnd["out_q"][i] = T * a_out
            bnd["v"][j] = T * torch.einsum("hij,ihd->jhd", p, ga)
            bnd["q"][i] = torch.einsum("hij,jhd->ihd", T * ds + pe, ka)
            bnd["k"][j] = torch.einsum("hij,ihd->jhd", T * ds + pe, qa)
            live["q"][i] = live["k"][j] = True
    if out.requires_grad:
        out.backward(g)
    grads = {n: torch.zeros_like(t) if t.grad is None else t.grad
             for n, t in x.items()}
    return out.detach(), grads, bnd, live


def check(inp, causal=False, scale=0.25):
    """bag_attention on the inputs' device within the bounds; scale is left
    to its default where it equals D ** -0.5."""
    want, want_g, bnd, live = oracle(inp, causal, scale)
    x = {n: inp[n].detach().clone().requires_grad_(True) for n in "qkv"}
    default = scale == inp["q"].shape[2] ** -0.5
    out = ops.bag_attention(x["q"], x["k"], x["v"], inp["offsets"],
                            inp["kv_offsets"], causal,
                            None if default else scale)
    out.backward(inp["dout"])
    assert out.dtype == torch.bfloat16 and out.shape == inp["q"].shape
    assert out.device == inp["q"].device
    got = dict(out_q=out.detach(), **{n: x[n].grad for n in "qkv"})
    want_g["out_q"] = want
    for n, b in bnd.items():
        assert got[n].dtype == torch.bfloat16
        rows = live["q" if n[-1] == "q" else "k"]
        assert rows.any() and (b[rows].flatten(1).sum(1) > 0).all(), n
        err = (got[n].cpu().double() - want_g[n]).abs()
        print("%s ratio %.4f" % (n, (err / b.clamp(min=1e-300)).max()))
        assert (err <= b).all(), n
    return out.detach()


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("D", [7, 8])
def test_cpu_reference_self(D, H, causal):
    check(make(QL, None, H, D), causal)


@pytest.mark.parametrize("H", [1, 3])
def test_cpu_reference_cross(H):
    check(make(QL, KL, H, 7))


def test_default_scale():
    check(make((3, 70), (66, 2), 2, 64), scale=0.125)


def test_causal_matters():
    inp = make(QL, None, 3, 8)
    assert not torch.equal(check(inp), check(inp, causal=True))


def k_is_v(inp):
    """One row tensor as k and v: its gradient is the bf16 sum of the two,
    each rounded once — 2^-8 of the computed sum on top of both bounds."""
    want, want_g, bnd, _ = oracle(dict(inp, v=inp["k"]))
    kv = inp["k"].clone().requires_grad_(True)
    out = ops.bag_attention(inp["q"], kv, kv, inp["offsets"],
                            inp["kv_offsets"], scale=0.25)
    out.backward(inp["dout"])
    assert ((out.detach().cpu().double() - want).abs() <= bnd["out_q"]).all()
    total = want_g["k"] + want_g["v"]
    bound = (1 + 2.0 ** -8) * (bnd["k"] + bnd["v"]) + 2.0 ** -8 * total.abs()
    assert ((kv.grad.cpu().double() - total).abs() <= bound).all()


def test_k_is_v():
    k_is_v(make(QL, KL, 3, 8))


def test_pull_attention_push_round_trip():
    table = EmbeddingTable("history", 50, 8, lr=0.5)
    table.master.copy_(make((50,), None, 1, 8, seed=3)["q"][:, 0])
    table.shadow.copy_(table.master)
    before = table.master.clone()
    ids = torch.tensor([4, 9, 4, 30, 7, 7, 7, 49, 0, 9])    # bags 3, 0, 4, 3
    inp = make((1, 1, 1, 1), (3, 0, 4, 3), 1, 8, seed=4)    # one target a bag
    rows = table.pull(ids).requires_grad_(True)
    kv = rows.view(10, 1, 8)
    assert torch.equal(inp["offsets"], torch.arange(5))
    out = ops.bag_attention(inp["q"], kv, kv, inp["offsets"],
                            inp["kv_offsets"], scale=0.25)
    out.backward(inp["dout"])
    dense = before[ids].view(10, 1, 8)      # the oracle indexes the table
    want, want_g, bnd, _ = oracle(dict(inp, k=dense, v=dense))
    assert ((out.detach().double() - want).abs() <= bnd["out_q"]).all()
    total = (want_g["k"] + want_g["v"]).view(10, 8)
    bound = ((1 + 2.0 ** -8) * (bnd["k"] + bnd["v"])).view(10, 8) \
        + 2.0 ** -8 * total.abs()
    assert total.abs().sum() > 0
    assert ((rows.grad.double() - total).abs() <= bound).all()
    table.push(ids, rows.grad)
    assert not torch.equal(table.master, before)


def test_validation():
    i = make((2, 3), (4, 2), 2, 8)
    q, k, v, off, kvo = i["q"], i["k"], i["v"], i["offsets"], i["kv_offsets"]
    f = ops.bag_attention
    wide = torch.zeros(5, 2, 129, dtype=torch.bfloat16)
    for bad in ((q.float(), k, v, off, kvo), (q[:, 0], k, v, off, kvo),
                (q, k[:, :1], v[:, :1], off, kvo), (q, k, v[:, :, :7], off, kvo),
                (wide, wide, wide, off), (q, k, v, off, kvo[:2]),
                (q, k, v, off.int(), kvo), (q, k, v, off),      # m != n
                (q, k, v, off, kvo, True),                      # causal + cross
                (q, q, q, torch.tensor([0, 3, 2, 5]))):         # not monotone
        with pytest.raises(ValueError):
            f(*bad)
