#!/usr/bin/env python
"""Time ops.dot_softmax_loss, forward + backward with gradients for q, w and
bias, against the two routes a user had before it existed.

Shapes (B, V, D): (1024, 131072, 128) — V >> B, where role Q's split
matters; (4096, 32768, 64); (8192, 1024, 256) — the shape at which the
sampled backward lost to the composition, where role W's split matters.

Versions (each is one forward and one backward from a fixed dloss):

* fused:    ``ops.dot_softmax_loss`` — nothing [B, V]-sized in memory; also
  with ``splits=1``, the unsplit grid the sampled op's backward has;
* composed: ``cross_entropy(q @ w.T + bias)`` (bf16 matmul, fp32 bias add) and
  autograd's backward of it;
* sampled:  ``ops.sampled_softmax_loss(q, w[labels], w, bias[labels], bias,
  labels, arange(V))`` — the accidental hits drop the label's own column;
  autograd gathers ``w[labels]`` and scatter-adds its gradient into w's.

The fused forward and backward are also timed alone (through the extension's
bindings, which allocate their outputs and workspaces as the op does).

Method (that of tools/sampledbench.py): device events; every version is
warmed up; each timing window lasts at least --window seconds; the versions
alternate inside one process (--reps rounds) and the median round is reported
with its min-max spread. The same inputs are reused by every call, so they
are cache-warm (at most 32 MiB of rows per shape against 256 MiB of last-level
cache): these are not cold-HBM figures.

Peak memory is ``torch.cuda.max_memory_allocated`` over one forward+backward
above what was allocated before it; it includes the gradients returned.

    python tools/softmaxbench.py --out profiles/dot_softmax_bench.txt
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd import ops  # noqa: E402
from sampledbench import peak_bytes, window  # noqa: E402


def composed(q, w, bias, labels):
    logits = (q @ w.t()).float() + bias
    return torch.nn.functional.cross_entropy(logits, labels, reduction="none")


def via_sampled(q, w, bias, labels):
    ids = torch.arange(w.shape[0], device=w.device)
    return ops.sampled_softmax_loss(q, w[labels], w, bias[labels], bias,
                                    labels, ids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x131072x128,4096x32768x64,"
                    "8192x1024x256", help="comma-separated BxVxD points")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "softmaxbench needs a GPU"
    dev = "cuda:0"
    ext = ops._ext()

    lines = ["dot_softmax_loss fwd+bwd: bf16 rows, fp32 bias, gradients for "
             "q, w, bias, %s" % torch.cuda.get_device_name(0),
             "window >= %.2f s, %d alternating rounds, median reported; "
             "inputs reused by every call (cache-warm)"
             % (args.window, args.reps),
             "%-18s %-34s %10s %7s   %s" % (
                 "B x V x D", "version", "ms/call", "iters", "min-max ms")]
    for shape in args.shapes.split(","):
        B, V, D = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev).manual_seed(0)
        rows = lambda n: (torch.randn(n, D, device=dev, generator=gen)  # noqa: E731
                          * D ** -0.25).to(torch.bfloat16)
        q, w = rows(B), rows(V)
        bias = torch.randn(V, device=dev, generator=gen)
        labels = torch.randint(0, V, (B,), device=dev, generator=gen)
        g = torch.rand(B, device=dev, generator=gen) + 0.5
        names = ("fused", "unsplit", "composed", "sampled")
        leaves = {v: [t.clone().requires_grad_(True) for t in (q, w, bias)]
                  for v in names}

        def step(version, fn):
            for t in leaves[version]:
                t.grad = None
            fn(*leaves[version], labels).backward(g)

        fused = lambda q, w, b, l: ops.dot_softmax_loss(q, w, l, b)  # noqa: E731
        unsplit = lambda q, w, b, l: ops.dot_softmax_loss(q, w, l, b, 1)  # noqa: E731
        steps = dict(fused=lambda: step("fused", fused),
                     unsplit=lambda: step("unsplit", unsplit),
                     composed=lambda: step("composed", composed),
                     sampled=lambda: step("sampled", via_sampled))
        loss, lse = ext.dot_softmax_fwd(q, w, labels, bias, 0)
        vs = [("fused    (dot_softmax_loss)", steps["fused"]),
              ("fused, splits=1", steps["unsplit"]),
              ("composed (matmul + cross_entropy)", steps["composed"]),
              ("sampled  (sampled_softmax_loss)", steps["sampled"]),
              ("fused forward kernels alone",
               lambda: ext.dot_softmax_fwd(q, w, labels, bias, 0)),
              ("fused backward kernels alone",
               lambda: ext.dot_softmax_bwd(q, w, labels, bias, lse, loss, g,
                                           0))]
        for _, fn in vs:                # warm every version
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {label: [] for label, _ in vs}
        iters = {}
        for _ in range(args.reps):      # versions alternate in one process
            for label, fn in vs:
                s, it = window(fn, args.window)
                times[label].append(s)
                iters[label] = it
        med = {}
        for label, _ in vs:
            ts = sorted(times[label])
            med[label] = ts[len(ts) // 2]
            lines.append("%-18s %-34s %10.3f %7d   %.3f-%.3f" % (
                shape, label, med[label] * 1e3, iters[label], ts[0] * 1e3,
                ts[-1] * 1e3))
        lines.append("%-18s splits (forward, role Q, role W) = %s; composed / "
                     "fused = %.2fx, sampled / fused = %.2fx, splits=1 / fused "
                     "= %.2fx" % (shape, ops.dot_softmax_nsplit(B, V),
                                  med[vs[2][0]] / med[vs[0][0]],
                                  med[vs[3][0]] / med[vs[0][0]],
                                  med[vs[1][0]] / med[vs[0][0]]))
        for n in names:                 # so that a peak holds its gradients
            for t in leaves[n]:
                t.grad = None
        peaks = {n: peak_bytes(steps[n]) for n in names}
        lines.append("%-18s peak memory above the inputs, MiB: %s; B * V = "
                     "%.0f Mi elements" % (shape, ", ".join(
                         "%s %.1f" % (n, peaks[n] / 2 ** 20) for n in names),
                         B * V / 2 ** 20))
        # nothing [B, V]-sized: beyond the gradients and the fp32 partial
        # tiles of a split role, under B * V bytes
        _, nq, nw = ops.dot_softmax_nsplit(B, V)
        known = (2 * (B + V) * D + 4 * V + 4 * (nq > 1) * nq * B * D
                 + 4 * (nw > 1) * nw * V * (D + 1))
        assert peaks["fused"] - known < B * V, \
            "the fused version allocated something [B, V]-sized"
        # same result? the composed version rounds the logits to bf16
        gf = leaves["fused"]
        for n in ("composed", "sampled"):
            go = leaves[n]
            diffs = ["%s max |diff| %.3g (magnitude %.3g)" % (
                what, float((a.grad.float() - b.grad.float()).abs().max()),
                float(a.grad.float().abs().max()))
                for what, a, b in zip(("dq", "dw", "dbias"), gf, go)]
            lines.append("%-18s fused vs %s: %s" % (shape, n, ", ".join(diffs)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
