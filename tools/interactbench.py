#!/usr/bin/env python
"""Time ops.dot_interaction, forward + backward, at sizes a CTR model would
run, against the composition a user had to write before it existed.

Shapes: B = 32768 examples of F bf16 feature vectors of width D — the DLRM
point F = 27, D = 128, one small-F point and one F = 40 point (the
three-tile kernel).

Versions (each is one forward and one backward from a fixed dout):

* fused:    ``ops.dot_interaction`` — one kernel each way, the kept row
  written with the triangle, no [B, F, F] tensor in HBM;
* composed: ``torch.bmm(x, x^T)``, a gather of the ``torch.tril_indices``
  triangle, ``torch.cat`` with x[:, 0], and autograd's backward of the three.

The fused kernels are also timed one at a time, and their effective rate
is reported: the bytes the op has to move (forward: x read, out written;
backward: x and dout read, dx written) over the kernel's time.

Method (that of tools/bagbench.py): device events; every version is warmed
up; each timing window lasts at least --window seconds; the versions
alternate inside one process (--reps rounds) and the median round is
reported with its min-max spread.

    python tools/interactbench.py --out profiles/interaction_bench.txt
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd import ops  # noqa: E402


def window(fn, min_s):
    """Seconds per call over one window of at least min_s (event-timed)."""
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    iters = max(3, int(min_s / max(start.elapsed_time(end) * 1e-3, 1e-6)) + 1)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e-3 / iters, iters


def composed(x, i, j):
    z = torch.bmm(x, x.transpose(1, 2))
    return torch.cat([x[:, 0], z[:, i, j]], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32 * 1024)
    ap.add_argument("--shapes", default="27x128,8x64,40x128",
                    help="comma-separated FxD points")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "interactbench needs a GPU"
    dev = "cuda:0"
    B = args.batch
    ext = ops._ext()

    lines = ["dot_interaction fwd+bwd: B = %d, bf16 x / out / dout, strict "
             "triangle, kept row, %s" % (B, torch.cuda.get_device_name(0)),
             "window >= %.2f s, %d alternating rounds, median reported"
             % (args.window, args.reps),
             "%-8s %-34s %10s %7s   %-15s %s" % (
                 "F x D", "version", "ms/call", "iters", "min-max ms",
                 "effective GB/s")]
    for shape in args.shapes.split(","):
        F, D = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(B, F, D, device=dev, generator=gen).to(torch.bfloat16)
        P = F * (F - 1) // 2
        dout = torch.randn(B, D + P, device=dev, generator=gen).to(
            torch.bfloat16)
        i, j = torch.tril_indices(F, F, -1, device=dev)
        xf = x.clone().requires_grad_(True)
        xc = x.clone().requires_grad_(True)

        def step_fused():
            xf.grad = None
            ops.dot_interaction(xf).backward(dout)

        def step_composed():
            xc.grad = None
            composed(xc, i, j).backward(dout)

        # bytes the op must move, per kernel
        fwd_bytes = 2 * (x.numel() + dout.numel())
        bwd_bytes = 2 * (2 * x.numel() + dout.numel())
        vs = [("fused    (dot_interaction)", step_fused, None),
              ("composed (bmm + gather + cat)", step_composed, None),
              ("fused forward kernel alone",
               lambda: ext.dot_interaction_fwd(x, False, True, False),
               fwd_bytes),
              ("fused backward kernel alone",
               lambda: ext.dot_interaction_bwd(x, dout, False, True),
               bwd_bytes)]
        for _, fn, _ in vs:             # warm every version
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {label: [] for label, _, _ in vs}
        iters = {}
        for _ in range(args.reps):      # versions alternate in one process
            for label, fn, _ in vs:
                s, it = window(fn, args.window)
                times[label].append(s)
                iters[label] = it
        med = {}
        for label, _, nbytes in vs:
            ts = sorted(times[label])
            med[label] = ts[len(ts) // 2]
            lines.append("%-8s %-34s %10.3f %7d   %-15s %s" % (
                shape, label, med[label] * 1e3, iters[label],
                "%.3f-%.3f" % (ts[0] * 1e3, ts[-1] * 1e3),
                "%.0f" % (nbytes / med[label] * 1e-9) if nbytes else "-"))
        lines.append("%-8s composed / fused = %.2fx" % (
            shape, med[vs[1][0]] / med[vs[0][0]]))
        # same result? the composed version rounds Z to bf16 before the
        # gather (as the fused one does once) but accumulates dx through
        # bf16 intermediates
        step_fused()
        step_composed()
        a, b = ops.dot_interaction(x), composed(x, i, j)
        lines.append("%-8s fused vs composed: out max |diff| %.3g (magnitude "
                     "%.3g), dx max |diff| %.3g (magnitude %.3g)" % (
                         shape, float((a.float() - b.float()).abs().max()),
                         float(a.float().abs().max()),
                         float((xf.grad.float() - xc.grad.float()).abs().max()),
                         float(xf.grad.float().abs().max())))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
