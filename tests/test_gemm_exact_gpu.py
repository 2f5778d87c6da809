"""Exact-arithmetic tests of every GEMM kernel path (csrc/gemm.hip).

+-1 inputs make fp32 accumulation exact in any order, so every
comparison with the fp64 reference is torch.equal — see _gemm_exact.py
for the method and the case table, test_gemm_exact.py for the check of
the reference itself. Each case first asserts, through the gemm_plan /
gemm_sgd_plan / gemm_vec_levels bindings, which kernel, K slicing,
reduce and staging level it takes; operands are views into NaN-filled
allocations and every output sits between guard bands of 7.
"""

import os
import subprocess
import sys

import pytest

import _gemm_exact as ge

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("c", ge.CASES, ids=lambda c: c.id)
def test_gemm_exact(c):
    """ops.gemm_bias_act on the tile, split-K (all three reduces),
    one-launch and small kernels, every epilogue variant of the case."""
    from tfmesos_amd import ops
    ge.check_case(ops, c, DEV)


@pytest.mark.parametrize("c", ge.UNALIGNED, ids=lambda c: c.id)
def test_gemm_unaligned_base_exact(c):
    """An operand that starts 2, 4 or 8 bytes into its storage: the
    staging level drops with the base, on the tile and the small
    kernel alike."""
    from tfmesos_amd import ops
    assert max(c.offa, c.offb) in (1, 2, 4)
    ge.check_case(ops, c, DEV)


@pytest.mark.parametrize("c", ge.SGD_CASES, ids=lambda c: c.id)
def test_gemm_sgd_exact(c):
    """ops.gemm_sgd alone: param bit for bit the fp64 result, shadow its
    bf16 rounding."""
    from tfmesos_amd import ops
    ge.check_sgd(ops, c, DEV)


@pytest.mark.parametrize("c", ge.PAIR_CASES, ids=lambda c: c.id)
def test_gemm_sgd_pair_exact(c):
    """ops.gemm_sgd_pair: both halves exact and both read pre-update
    operands."""
    from tfmesos_amd import ops
    ge.check_pair(ops, c, DEV)


def test_gemm_last_arriver_exact_in_child():
    """The last-arriver split-K epilogue behind TFA_GEMM_LA=1 (read once
    per process, hence a fresh child) passes the reduce1 cases, at
    ldc % 4 == 0 and != 0, each run twice: the tile counters reset
    themselves."""
    env = dict(os.environ, TFA_GEMM_LA="1")
    p = subprocess.run(
        [sys.executable, os.path.join(HERE, "_gemm_exact_proc.py")],
        env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
        universal_newlines=True, timeout=180)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:],
                               p.stderr[-2000:])
    lines = [ln for ln in p.stdout.splitlines()
             if ln.startswith(("OK ", "FAIL "))]
    assert lines == ge.proc_lines(), (lines, p.stderr[-2000:])
