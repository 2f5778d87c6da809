"""The oracle of the exact GEMM tests, checked without a GPU.

test_gemm_exact_gpu.py compares the HIP GEMM kernels with
_gemm_exact.reference (fp64 matmul of the stored operands) using
torch.equal. Here that reference is itself compared with naive loops
written below, and the +-1 generator, the max|ref| <= 256 exactness
condition, the relu clip fraction and the fp32-exactness of the SGD
results are run on every listed case, so a bad shape or seed shows up
before any GPU run.
"""

import pytest
import torch

import _gemm_exact as ge


def naive(a, b, ta, tb, bias, act, aux):
    """out and colsum straight from the definition, one product at a
    time, indexing the STORED operands."""
    M = a.shape[1] if ta else a.shape[0]
    K = a.shape[0] if ta else a.shape[1]
    N = b.shape[0] if tb else b.shape[1]
    out = torch.zeros(M, N, dtype=torch.float64)
    cs = torch.zeros(N, dtype=torch.float64)
    for n in range(N):
        for k in range(K):
            cs[n] += b[n, k] if tb else b[k, n]
        for m in range(M):
            s = 0.0
            for k in range(K):
                av = a[k, m] if ta else a[m, k]
                bv = b[n, k] if tb else b[k, n]
                s += float(av) * float(bv)
            if bias is not None:
                s += float(bias[n])
            if act == "relu":
                s = max(s, 0.0)
            elif act == "relu_bwd":
                s = s if aux[m, n] > 0 else 0.0
            elif act == "sub":
                s -= float(aux[m, n])
            out[m, n] = s
    return out, cs


TINY = [(3, 5, 4), (1, 7, 9), (6, 2, 11)]


@pytest.mark.parametrize("mnk", TINY, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("combo", sorted(ge.COMBOS))
def test_reference_matches_naive_loops(combo, mnk):
    M, N, K = mnk
    ta, tb = ge.COMBOS[combo]
    for act in ("none", "relu", "relu_bwd", "sub"):
        c = ge._g("tiny", combo, M, N, K, ge.TILE, act=act)
        gen = torch.Generator().manual_seed(ge.SEED - 1 - M)
        a, b, bias, aux = ge.inputs(c, gen)
        assert tuple(a.shape) == ((K, M) if ta else (M, K))
        assert tuple(b.shape) == ((N, K) if tb else (K, N))
        for bv in (None, bias):
            got = ge.reference(a, b, ta, tb, bv, act, aux)
            want = naive(a, b, ta, tb, bv, act, aux)
            assert torch.equal(got[0], want[0])
            assert torch.equal(got[1], want[1])


def test_case_ids_unique_and_tables_complete():
    for table in (ge.ALL, ge.SGD_CASES, ge.PAIR_CASES):
        assert len({c.id for c in table}) == len(table)
    assert len(ge.BY_ID) == len(ge.ALL)
    assert len(ge.UNALIGNED) == 36
    # the last-arriver child: N = 72 and N = 65, and a colsum case
    assert {c.N for c in ge.LA_CASES} >= {72, 65}
    assert len(ge.LA_CASES) == 6 and ge.LA_KEEP[0].colsum
    assert len(ge.proc_lines()) == 2 * (len(ge.LA_CASES) + len(ge.LA_KEEP))
    # every path runs all twelve epilogues on at least one shape
    full = {c.plan[0] + "+" + c.plan[3] for c in ge.CASES if c.epi == "all"}
    assert full >= {"tile+none", "tile_sk+reduce1", "tile_sk+reduce4",
                    "small+none"}
    assert len(ge.EPI_ALL) == 12
    for c in ge.CASES:
        assert set(ge.EPI_TWO) <= set(ge.variants(c)) or c.colsum or \
            c.act != "none"


@pytest.mark.parametrize("c", ge.ALL, ids=lambda c: c.id)
def test_case_is_exactly_representable(c):
    a, b, bias, aux = ge.inputs(c)
    for t in (a, b):
        assert torch.equal(t.abs(), torch.ones_like(t))      # +-1, no zeros
        assert -1 in t and 1 in t
    assert torch.equal(bias, bias.round()) and bias.abs().max() <= 3
    if c.act == "relu_bwd":
        assert torch.equal(aux.abs(), torch.ones_like(aux))
    if c.act == "sub":
        assert torch.equal(aux, aux.round()) and aux.abs().max() <= 3
    ge.assert_conditions(c)
    for v in ge.variants(c):
        out, cs = ge.ref_of(c, v)
        assert tuple(out.shape) == (c.M, c.N) and tuple(cs.shape) == (c.N,)
        assert torch.equal(out, out.round())
        # fp32 holds every value; bf16 wherever the case stores bf16
        assert torch.equal(out.float().double(), out)
        if v[2] == "bf16":
            assert torch.equal(out.to(torch.bfloat16).double(), out)
            if c.colsum:
                assert torch.equal(cs.to(torch.bfloat16).double(), cs)
            # K <= 320 wherever bf16 is stored, but for the one 16-slice
            # case, which stands under the same max|ref| assertion
            assert c.K <= 320 or c.id == "sk1_nn_stripes_64x64x2048"
    assert c.M * c.N <= 1030 * 1030
    # an unaligned case is its base case at another address
    if c.offa or c.offb:
        base = ge.BY_ID[c.id.split("_off")[0]]
        assert (base.combo, base.M, base.N, base.K, base.plan) == \
            (c.combo, c.M, c.N, c.K, c.plan)


def test_expected_vec_levels():
    assert [ge.expect_vec(40, o) for o in (0, 1, 2, 4, 8)] == [8, 1, 2, 2, 8]
    assert [ge.expect_vec(42, o) for o in (0, 1, 2)] == [2, 1, 2]
    assert ge.expect_vec(17, 0) == 1 and ge.expect_vec(65, 2) == 1


@pytest.mark.parametrize("c", ge.SGD_CASES, ids=lambda c: c.id)
def test_sgd_case_is_fp32_exact(c):
    a, b, p = ge.sgd_inputs(c)
    ta, tb = ge.COMBOS[c.combo]
    assert torch.equal(p * 64, (p * 64).round()) and p.abs().max() <= 4
    g, _ = ge.reference(a, b, ta, tb)
    assert g.abs().max() <= 320
    want = ge.sgd_reference(a, b, ta, tb, p, c.nd)
    ge.assert_fp32_exact(want)          # round trip through fp32
    # so are the intermediates, fused or not
    ge.assert_fp32_exact(ge.GSCALE * g)
    ge.assert_fp32_exact(ge.GSCALE * g + c.nd * p.clamp(max=0))
    ge.assert_fp32_exact(ge.LR * (ge.GSCALE * g + c.nd * p.clamp(max=0)))
    # the update moved the parameters, and the decay term is live
    assert not torch.equal(want, p)
    if c.nd:
        assert not torch.equal(
            want, ge.sgd_reference(a, b, ta, tb, p, 0.0))


@pytest.mark.parametrize("c", ge.PAIR_CASES, ids=lambda c: c.id)
def test_pair_case_is_fp32_exact(c):
    ins = ge.pair_inputs(c)
    for (cb, M, N, K, _), (a, b, p) in zip((c.h1, c.h2), ins):
        ta, tb = ge.COMBOS[cb]
        ge.assert_fp32_exact(ge.sgd_reference(a, b, ta, tb, p, c.nd))
    # each shadow fits inside the other half's A operand
    for i in range(2):
        _, M, N, _, _ = (c.h1, c.h2)[i]
        assert ge.SHADOW_AT + M * N <= ins[1 - i][0].numel()
        assert ge.SHADOW_AT % 8 == 0
    if c.id == "pair_wsoff":
        (_, M, N, _, (_, ns)) = c.h1
        assert (M * N * ns) % 2 == 1 and (c.h2[1] * c.h2[2]) % 4 == 0
