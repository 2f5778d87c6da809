#!/usr/bin/env python
"""Time ops.sampled_softmax_loss, forward + backward, against the composition
a user had to write before it existed.

Shapes (B, S, D): (4096, 4096, 128) — in-batch-sized retrieval; (1024, 8192,
64) — a word2vec-like step, few examples against many candidates; (8192,
1024, 256) — a wide classifier at the row-width limit.

Versions (each is one forward and one backward from a fixed dloss, with ids
and both adjustments, gradients for h, w_true and w_samp):

* fused:    ``ops.sampled_softmax_loss`` — one MFMA kernel each way (and the
  forward's finishing kernel), nothing [B, S]-sized in memory;
* composed: ``h @ w_samp.T`` in bf16, ``+ samp_adj`` in fp32, ``masked_fill``
  of the accidental hits, ``logsumexp`` over the cat with the true score, and
  autograd's backward of all of it.

The fused forward and backward are also timed alone (through the extension's
bindings, which allocate their outputs as the op does).

Method (that of tools/interactbench.py): device events; every version is
warmed up; each timing window lasts at least --window seconds; the versions
alternate inside one process (--reps rounds) and the median round is reported
with its min-max spread. The same inputs are reused by every call, so they
are cache-warm (at most 9 MiB of rows per shape against 256 MiB of last-level
cache): these are not cold-HBM figures.

Peak memory is ``torch.cuda.max_memory_allocated`` over one forward+backward
above what was allocated before it. Beyond the three row gradients it
returns, the fused version must stay under B * S bytes (a [B, S] tensor of
any dtype used here is at least twice that).

    python tools/sampledbench.py --out profiles/sampled_softmax_bench.txt
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


def composed(h, w_true, w_samp, true_adj, samp_adj, labels, sampled):
    t = (h.float() * w_true.float()).sum(1) + true_adj
    l = (h @ w_samp.t()).float() + samp_adj
    l = l.masked_fill(labels[:, None] == sampled[None, :], float("-inf"))
    return torch.logsumexp(torch.cat([t[:, None], l], 1), 1) - t


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x4096x128,1024x8192x64,"
                    "8192x1024x256", help="comma-separated BxSxD points")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sampledbench needs a GPU"
    dev = "cuda:0"
    ext = ops._ext()

    lines = ["sampled_softmax_loss fwd+bwd: bf16 rows, ids and both "
             "adjustments, %s" % torch.cuda.get_device_name(0),
             "window >= %.2f s, %d alternating rounds, median reported; "
             "inputs reused by every call (cache-warm)"
             % (args.window, args.reps),
             "%-15s %-34s %10s %7s   %s" % (
                 "B x S x D", "version", "ms/call", "iters", "min-max ms")]
    for shape in args.shapes.split(","):
        B, S, D = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev).manual_seed(0)
        rows = lambda n: (torch.randn(n, D, device=dev, generator=gen)  # noqa: E731
                          * D ** -0.25).to(torch.bfloat16)
        h, wt, ws = rows(B), rows(B), rows(S)
        ta = torch.randn(B, device=dev, generator=gen)
        sa = torch.randn(S, device=dev, generator=gen)
        labels = torch.randint(0, 8 * S, (B,), device=dev, generator=gen)
        sampled = torch.randint(0, 8 * S, (S,), device=dev, generator=gen)
        g = torch.rand(B, device=dev, generator=gen) + 0.5
        leaves = {v: [t.clone().requires_grad_(True) for t in (h, wt, ws)]
                  for v in ("fused", "composed")}

        def step(version, fn):
            for t in leaves[version]:
                t.grad = None
            fn(*leaves[version], ta, sa, labels, sampled).backward(g)

        step_fused = lambda: step("fused", ops.sampled_softmax_loss)  # noqa: E731
        step_composed = lambda: step("composed", composed)  # noqa: E731
        loss, lse = ext.sampled_softmax_fwd(h, wt, ws, ta, sa, labels, sampled)
        vs = [("fused    (sampled_softmax_loss)", step_fused),
              ("composed (matmul + logsumexp)", step_composed),
              ("fused forward kernels alone",
               lambda: ext.sampled_softmax_fwd(h, wt, ws, ta, sa, labels,
                                               sampled)),
              ("fused backward kernel alone",
               lambda: ext.sampled_softmax_bwd(h, wt, ws, sa, labels, sampled,
                                               lse, loss, g))]
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
            lines.append("%-15s %-34s %10.3f %7d   %.3f-%.3f" % (
                shape, label, med[label] * 1e3, iters[label], ts[0] * 1e3,
                ts[-1] * 1e3))
        lines.append("%-15s composed / fused = %.2fx" % (
            shape, med[vs[1][0]] / med[vs[0][0]]))
        pf, pc = peak_bytes(step_fused), peak_bytes(step_composed)
        lines.append("%-15s peak memory above the inputs: fused %.2f MiB, "
                     "composed %.2f MiB; B * S = %.2f Mi elements" % (
                         shape, pf / 2 ** 20, pc / 2 ** 20, B * S / 2 ** 20))
        assert pf - 2 * (2 * B + S) * D < B * S, \
            "the fused version allocated something [B, S]-sized"
        # same result? the composed version rounds the logits to bf16
        a = ops.sampled_softmax_loss(h, wt, ws, ta, sa, labels, sampled)
        b = composed(h, wt, ws, ta, sa, labels, sampled)
        gf, gc = leaves["fused"], leaves["composed"]
        lines.append("%-15s fused vs composed: loss max |diff| %.3g "
                     "(magnitude %.3g), dh max |diff| %.3g (magnitude %.3g), "
                     "dw_samp max |diff| %.3g (magnitude %.3g)" % (
                         shape, float((a - b).abs().max()),
                         float(a.abs().max()),
                         float((gf[0].grad.float() - gc[0].grad.float())
                               .abs().max()),
                         float(gf[0].grad.float().abs().max()),
                         float((gf[2].grad.float() - gc[2].grad.float())
                               .abs().max()),
                         float(gf[2].grad.float().abs().max())))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
