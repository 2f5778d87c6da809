"""Exact-arithmetic tests of every conv kernel path (csrc/conv.hip).

+-1 inputs make fp32 accumulation exact in any order, so every
comparison with the fp64 reference is torch.equal — see _conv_exact.py
for the method and the case table, test_conv_exact.py for the check of
the reference itself. Each case also asserts, through the
conv_*_slices bindings, which reduction split the shape takes.
"""

import os
import subprocess
import sys

import pytest
import torch

import _conv_exact as ce

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("c", ce.CASES, ids=lambda c: c.id)
def test_conv_kcrs_exact(c):
    """fwd (+bias), bwd-data and bwd-weight with torch-layout weights;
    dW returns through autograd as bf16."""
    from tfmesos_amd import ops
    ce.check_case(ops, c, DEV, "kcrs")


@pytest.mark.parametrize("c", ce.CASES, ids=lambda c: c.id)
def test_conv_krsc_dw_out_exact(c):
    """Tap-major weights and the grad-arena path: dW accumulated into a
    pre-zeroed fp32 dw_out, w.grad None."""
    from tfmesos_amd import ops
    ce.check_case(ops, c, DEV, "krsc")


def test_launched_slices_of_ragged_split():
    """The 5x5 forward split really launches 7 slices with a 24-tap
    last one (the heuristic value 9 is rounded to whole 32-tap tiles)."""
    from tfmesos_amd import ops
    c = ce.BY_ID["fsplit_kd600_5x5"]
    Ho, Wo = ce.out_hw(c)
    z = ops._ext().conv_fwd_slices(c.N, c.K, Ho, Wo, c.C, c.R, c.S)
    assert ce.launched_slices(c.R * c.S * c.C, z) == (7, 24)


@pytest.mark.parametrize("n", ce.NARROW, ids=lambda n: "off%d_pad%d" % n)
def test_conv_bwd_narrow_dy_exact(n):
    """dy a channel-narrow view of a wider channels-last buffer, at an
    aligned and two misaligned (offset, row stride) pairs."""
    from tfmesos_amd import ops
    ce.check_narrow(ops, n[0], n[1], DEV)


def test_conv_fallback_kernels_exact_in_child():
    """The k-major bwd-weight and non-transpose bwd-data kernels behind
    TFA_BWDW_TR=0 / TFA_BWDD_TR=0 (read once per process, hence a fresh
    child) pass the same cases."""
    env = dict(os.environ, TFA_BWDW_TR="0", TFA_BWDD_TR="0")
    p = subprocess.run(
        [sys.executable, os.path.join(HERE, "_conv_exact_proc.py")],
        env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
        universal_newlines=True, timeout=180)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:],
                               p.stderr[-2000:])
    lines = [ln for ln in p.stdout.splitlines()
             if ln.startswith(("OK ", "FAIL "))]
    assert lines == ce.proc_lines(), (lines, p.stderr[-2000:])
