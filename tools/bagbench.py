#!/usr/bin/env python
"""Time EmbeddingTable.pull_pooled / push_pooled at a size a user would
run, against the composition a user had to write before they existed.

Table 4M x 256 (Adagrad: fp32 master + bf16 shadow + accumulator), n = 1M
ids in B = 32768 bags (random cut points: mean length 32, some empty),
two modes: unweighted sum and weighted mean.

Versions:

* pull, fused:    ``pull_pooled`` — one gather-and-reduce kernel, B x D out;
* pull, composed: ``embedding_gather`` of the n x D bf16 rows, then a
  torch ``index_add_`` segment sum in fp32 (times the coefficients for
  weighted mean) and the cast to bf16;
* push, fused:    ``push_pooled`` — bag gradients read through the
  indirection inside the sparse-apply kernel;
* push, composed: the n x D rows ``c * bag_grads[bag_of]`` built in bf16
  and handed to ``push``.

The composed versions get ``bag_of`` and the coefficients precomputed
outside the timed region (the fused ones derive them from the offsets
inside it).

Method (that of tools/sparsebench.py): device events; every (version,
mode) is warmed up; each timing window lasts at least --window seconds;
the versions alternate inside one process (--reps rounds) and the median
round is reported with its min-max spread.

    python tools/bagbench.py --out profiles/embedding_bag_bench.txt
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd import ops  # noqa: E402
from tfmesos_amd.ps.sparse import EmbeddingTable  # noqa: E402


def big_table(rows, dim, dev):
    """An Adagrad EmbeddingTable whose buffers are generated on the device
    (the constructor's seeded host init of 1G elements is setup time this
    tool does not need)."""
    t = EmbeddingTable("bench", 1, dim, device=dev, lr=0.01,
                       optimizer="adagrad")
    t.rows = rows
    t.master = torch.rand(rows, dim, device=dev) / dim ** 0.5
    t.shadow = t.master.to(torch.bfloat16)
    t.state = {k: torch.zeros(rows, dim, device=dev) for k in t.state}
    return t


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--n", type=int, default=1024 * 1024)
    ap.add_argument("--bags", type=int, default=32 * 1024)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bagbench needs a GPU"
    dev = "cuda:0"
    V, D, n, B = args.rows, args.dim, args.n, args.bags

    gen = torch.Generator(device=dev).manual_seed(0)
    ids = torch.randint(0, V, (n,), device=dev, generator=gen)
    cuts = torch.randint(0, n + 1, (B - 1,), device=dev, generator=gen)
    offsets = torch.cat([cuts.new_zeros(1), cuts.sort().values,
                         cuts.new_full((1,), n)])
    lens = offsets[1:] - offsets[:-1]
    bag_of = torch.repeat_interleave(torch.arange(B, device=dev), lens)
    w = torch.rand(n, device=dev, generator=gen) + 0.5
    W = torch.zeros(B, device=dev).index_add_(0, bag_of, w)
    modes = [("sum", None, None),
             ("weighted mean", w, (w / W[bag_of])[:, None])]
    bag_grads = (torch.randn(B, D, device=dev, generator=gen) * 0.01).to(
        torch.bfloat16)

    tf, tc = big_table(V, D, dev), big_table(V, D, dev)
    tc.master.copy_(tf.master)
    tc.shadow.copy_(tf.shadow)

    def versions(weights, coef):
        combiner = "sum" if weights is None else "mean"

        def pull_fused():
            return tf.pull_pooled(ids, offsets, weights, combiner)

        def pull_composed():
            rows = ops.embedding_gather(tc.shadow, ids).float()
            if coef is not None:
                rows = rows * coef
            out = torch.zeros(B, D, device=dev).index_add_(0, bag_of, rows)
            return out.to(torch.bfloat16)

        def push_fused():
            tf.push_pooled(ids, offsets, bag_grads, weights, combiner)

        def push_composed():
            rows = bag_grads[bag_of]
            if coef is not None:
                rows = (rows.float() * coef).to(torch.bfloat16)
            tc.push(ids, rows)

        return [("pull fused    (pull_pooled)", pull_fused),
                ("pull composed (gather + index_add_)", pull_composed),
                ("push fused    (push_pooled)", push_fused),
                ("push composed (expanded rows + push)", push_composed)]

    lines = ["pooled pull/push: table %d x %d adagrad, n = %d ids in B = %d "
             "bags (length mean %.1f, max %d, %d empty), bf16 bag grads, %s"
             % (V, D, n, B, float(lens.float().mean()), int(lens.max()),
                int((lens == 0).sum()), torch.cuda.get_device_name(0)),
             "window >= %.2f s, %d alternating rounds, median reported"
             % (args.window, args.reps),
             "%-40s %-14s %10s %7s   %s" % ("version", "mode", "ms/call",
                                            "iters", "min-max ms")]
    for mode, weights, coef in modes:
        vs = versions(weights, coef)
        for _, fn in vs:                # warm every (version, mode)
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
            lines.append("%-40s %-14s %10.3f %7d   %.3f-%.3f"
                         % (label, mode, med[label] * 1e3, iters[label],
                            ts[0] * 1e3, ts[-1] * 1e3))
        lines.append("%s: composed / fused = %.2fx pull, %.2fx push"
                     % (mode, med[vs[1][0]] / med[vs[0][0]],
                        med[vs[3][0]] / med[vs[2][0]]))
    # same result? from identical state, one pull and one push of each
    # version per mode (the composed push rounds its n x D rows to bf16)
    tc.master.copy_(tf.master)
    tc.shadow.copy_(tf.shadow)
    for k in tf.state:
        tc.state[k].copy_(tf.state[k])
    for mode, weights, coef in modes:
        vs = versions(weights, coef)
        a, b = vs[0][1](), vs[1][1]()
        vs[2][1]()
        vs[3][1]()
        lines.append("%s, fused vs composed from identical state: pull max "
                     "|diff| %.3g (bf16 rows of magnitude %.3g), master after "
                     "one push max |diff| %.3g"
                     % (mode, float((a.float() - b.float()).abs().max()),
                        float(a.float().abs().max()),
                        float((tf.master - tc.master).abs().max())))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
