#!/usr/bin/env python
"""Time ops.dot_topk and ops.dot_rank against the compositions a user had to
write before they existed.

Shapes (B, V, D, k): (1024, 1M, 64, 10) — an evaluation batch of a two-tower
model against its whole catalogue; (1024, 1M, 128, 64) — wider rows, k at its
limit; (64, 4M, 64, 10) — a serving-sized batch against a larger catalogue.
A shape with the suffix ``a`` has its items sorted by ascending score for
query 0, so that query's row is compacted at every tile: the stated worst
case of the selection.

Versions:

* fused topk:    ``ops.dot_topk`` — MFMA scores and a running top-k per row
  in LDS, then the merge kernel; nothing [B, V]-sized in memory;
* composed topk: ``torch.topk((q @ w.T).float() + bias, k)``;
* fused rank:    ``ops.dot_rank`` — true-score, count and finishing kernels;
* composed rank: the same scores, ``(s > s.gather(1, labels)).sum(1)`` (the
  tie rule by index is left out of it, which favours the composition).

Method (that of tools/sampledbench.py): device events; every version is
warmed up; each timing window lasts at least --window seconds; the versions
alternate inside one process (--reps rounds) and the median round is reported
with its min-max spread. The same inputs are reused by every call: w is 128 -
512 MiB against 256 MiB of last-level cache, so the rows are partly
cache-warm; a cold run is not measured here.

Peak memory is ``torch.cuda.max_memory_allocated`` over one call above what
was allocated before it; the fused versions must stay under B * V bytes.

    python tools/topkbench.py --out profiles/dot_topk_bench.txt
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd import ops  # noqa: E402
from tools.sampledbench import peak_bytes, window  # noqa: E402


def scores(q, w, bias):
    return (q @ w.t()).float() + bias


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x1048576x64x10,"
                    "1024x1048576x128x64,64x4194304x64x10,"
                    "1024x1048576x64x10a",
                    help="comma-separated BxVxDxk points; a trailing 'a' "
                    "sorts the items by ascending score for query 0")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "topkbench needs a GPU"
    dev = "cuda:0"

    lines = ["dot_topk / dot_rank: bf16 rows, fp32 bias, %s"
             % torch.cuda.get_device_name(0),
             "window >= %.2f s, %d alternating rounds, median reported; "
             "inputs reused by every call (partly cache-warm)"
             % (args.window, args.reps),
             "%-22s %-28s %10s %7s   %s" % (
                 "B x V x D x k", "version", "ms/call", "iters", "min-max ms")]
    for shape in args.shapes.split(","):
        B, V, D, k = (int(v) for v in shape.rstrip("a").split("x"))
        gen = torch.Generator(device=dev).manual_seed(0)
        rows = lambda n: (torch.randn(n, D, device=dev, generator=gen)  # noqa: E731
                          * D ** -0.25).to(torch.bfloat16)
        q, w = rows(B), rows(V)
        bias = torch.randn(V, device=dev, generator=gen)
        labels = torch.randint(0, V, (B,), device=dev, generator=gen)
        if shape.endswith("a"):
            perm = torch.argsort(w.float() @ q[0].float() + bias)
            w, bias = w[perm].contiguous(), bias[perm].contiguous()

        def composed_rank():
            s = scores(q, w, bias)
            return (s > s.gather(1, labels[:, None])).sum(1)

        vs = [("fused topk    (dot_topk)", lambda: ops.dot_topk(q, w, k, bias)),
              ("composed topk (matmul+topk)",
               lambda: torch.topk(scores(q, w, bias), k)),
              ("fused rank    (dot_rank)",
               lambda: ops.dot_rank(q, w, labels, bias)),
              ("composed rank (matmul+count)", composed_rank)]
        for _, fn in vs:                # warm every version
            for _ in range(2):
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
            lines.append("%-22s %-28s %10.3f %7d   %.3f-%.3f" % (
                shape, label, med[label] * 1e3, iters[label], ts[0] * 1e3,
                ts[-1] * 1e3))
        lines.append("%-22s composed / fused: topk %.2fx, rank %.2fx; "
                     "nsplit %d" % (
                         shape, med[vs[1][0]] / med[vs[0][0]],
                         med[vs[3][0]] / med[vs[2][0]],
                         ops.dot_topk_nsplit(B, V)))
        peaks = [peak_bytes(fn) / 2 ** 20 for _, fn in vs]
        lines.append("%-22s peak memory above the inputs, MiB: fused topk "
                     "%.2f, composed topk %.2f, fused rank %.2f, composed "
                     "rank %.2f; B * V = %.0f Mi elements" % (
                         (shape,) + tuple(peaks) + (B * V / 2 ** 20,)))
        assert max(peaks[0], peaks[2]) * 2 ** 20 < B * V, \
            "a fused version allocated something [B, V]-sized"
        # same result? against fp32 scores from the same bf16 rows, first
        # queries only (the composition above rounds its logits to bf16)
        n = min(B, 64)
        ref = q[:n].float() @ w.float().t() + bias
        rv, ri = torch.topk(ref, k)
        fv, fi = ops.dot_topk(q, w, k, bias)
        cv, ci = torch.topk(scores(q, w, bias)[:n], k)
        rr = (ref > ref.gather(1, labels[:n, None])).sum(1)
        lines.append("%-22s against fp32 scores, first %d queries: indices "
                     "equal fused %.4f, composed %.4f; values max |diff| "
                     "fused %.3g, composed %.3g (magnitude %.3g); rank max "
                     "|diff| fused %d" % (
                         shape, n, float((fi[:n] == ri).float().mean()),
                         float((ci == ri).float().mean()),
                         float((fv[:n] - rv).abs().max()),
                         float((cv - rv).abs().max()), float(rv.abs().max()),
                         int((ops.dot_rank(q, w, labels, bias)[:n] - rr)
                             .abs().max())))
        del ref, q, w, bias
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
