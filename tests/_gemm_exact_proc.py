"""Helper: the exact split-K GEMM cases (_gemm_exact.py) in one process
with the last-arriver epilogue, selected by TFA_GEMM_LA=1 — read once
per process. Every reduce1 case must then plan "last_arriver" (the
colsum case keeps "reduce4_cs"); each case runs twice, the second run
on the tile counters the first one left. Prints one "OK ..." line per
run; a mismatch prints "FAIL ..." and the exit status is 1. A HIP error
is not caught: it ends the process at once, nothing more is launched.

usage: TFA_GEMM_LA=1 _gemm_exact_proc.py"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import _gemm_exact as ge  # noqa: E402
from tfmesos_amd import ops  # noqa: E402

DEV = "cuda:0"


def main():
    print("TFA_GEMM_LA=%s" % os.environ.get("TFA_GEMM_LA"))
    bad = 0
    for c in ge.LA_CASES + ge.LA_KEEP:
        for run in (1, 2):
            name = "%s run%d" % (c.id, run)
            try:
                ge.check_case(ops, c, DEV, plan=ge.la_plan(c))
                torch.cuda.synchronize()
                print("OK " + name)
            except AssertionError as e:
                bad += 1
                print("FAIL %s: %s" % (name, e))
            sys.stdout.flush()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
