"""Helper: the exact conv cases (_conv_exact.py) in one process, for
kernels selected by environment switches that are read once per process
(TFA_BWDW_TR / TFA_BWDD_TR). Prints one "OK ..." line per case; a
mismatch prints "FAIL ..." and the exit status is 1. A HIP error is not
caught: it ends the process at once, nothing more is launched.

usage: TFA_BWDW_TR=0 TFA_BWDD_TR=0 _conv_exact_proc.py"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import _conv_exact as ce  # noqa: E402
from tfmesos_amd import ops  # noqa: E402

DEV = "cuda:0"


def main():
    print("TFA_BWDW_TR=%s TFA_BWDD_TR=%s" % (
        os.environ.get("TFA_BWDW_TR"), os.environ.get("TFA_BWDD_TR")))
    jobs = [("kcrs %s" % c.id, lambda c=c: ce.check_case(ops, c, DEV, "kcrs"))
            for c in ce.CASES]
    jobs += [("krsc %s" % c.id, lambda c=c: ce.check_case(ops, c, DEV, "krsc"))
             for c in ce.CASES]
    jobs += [("narrow %d %d" % n,
              lambda n=n: ce.check_narrow(ops, n[0], n[1], DEV))
             for n in ce.NARROW]
    bad = 0
    for name, job in jobs:
        try:
            job()
            torch.cuda.synchronize()
            print("OK " + name)
        except AssertionError as e:
            bad += 1
            print("FAIL %s: %s" % (name, e))
        sys.stdout.flush()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
