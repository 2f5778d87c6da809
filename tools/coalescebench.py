#!/usr/bin/env python
"""Time the worker-side coalescing of one row request.

Versions, on the same ids [n] and fp32 gradient rows [n, D]:

* kernels:     ops.coalesce_ids + ops.segment_sum_rows (fp32 rows -> bf16,
               csrc/coalesce.hip) + the ops.embedding_gather expand of the
               [u, D] bf16 rows back to [n, D] (the pull side);
* composition: what a user writes without them — torch.unique(
               return_inverse=True), index_add_ into fp32 zeros, cast to
               bf16, index_select.

Both end with the distinct ids, the per-id bf16 sums and the expanded rows
on the device, and both read the number of distinct ids back once (it sizes
the outputs). The rows are dyadic (randint(-32, 33)/16), so the fp32 sums
are exact in any order and the two versions must agree bit for bit.

Shapes: n = 1M, D = 256, ids Zipf-like (log-uniform) over 4M rows (a large
request with hot ids) and n = 256, D = 200, uniform over 1000 rows (a small
one, where time is launches). For each the tool prints u/n and the bytes a
push puts on the wire with and without coalescing, u(8+2D) against n(8+2D).

Method (that of tools/partbench.py): device events; every (version, shape)
is warmed up; each timing window lasts at least --window seconds; the
versions alternate inside one process (--reps rounds) and the median round
is reported. "no slower" = the kernels' median is at or below the
composition's median plus the composition's min-max spread.

    python tools/coalescebench.py --out profiles/coalesce_bench.txt
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd import ops  # noqa: E402

SHAPES = [(1024 * 1024, 256, 4 * 1024 * 1024, "zipf"),      # n, D, V, ids
          (256, 200, 1000, "uniform")]


def kernels(ids, rows):
    co = ops.coalesce_ids(ids)
    u = int(co.count)
    summed = ops.segment_sum_rows(rows, co.perm, co.seg, u, torch.bfloat16)
    return co.uniq[:u], summed, ops.embedding_gather(summed, co.inverse)


def composition(ids, rows):
    uniq, inv = torch.unique(ids, return_inverse=True)
    summed = torch.zeros(uniq.numel(), rows.shape[1], device=rows.device)
    summed = summed.index_add_(0, inv, rows).to(torch.bfloat16)
    return uniq, summed, summed.index_select(0, inv)


VERSIONS = [("kernels (coalesce_ids + segment_sum_rows)", kernels),
            ("composition (unique/index_add_/index_select)", composition)]


def make_ids(kind, n, V, gen, dev):
    if kind == "uniform":
        return torch.randint(0, V, (n,), device=dev, generator=gen)
    # log-uniform over [1, V]: P(id = k) ~ 1/k, Zipf with exponent 1
    x = torch.rand(n, device=dev, generator=gen, dtype=torch.float64)
    return (float(V) ** x).long().clamp_(1, V) - 1


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
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "coalescebench needs a GPU"
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = ["coalescing of one row request: fp32 rows -> per-id bf16 sums "
             "+ expand, %s" % torch.cuda.get_device_name(0),
             "window >= %.2f s, %d alternating rounds, median reported"
             % (args.window, args.reps),
             "%-46s %-26s %10s %8s   %s" % ("version", "n x D, ids", "us/call",
                                            "iters", "min-max us")]
    for n, D, V, kind in SHAPES:
        ids = make_ids(kind, n, V, gen, dev)
        rows = torch.randint(-32, 33, (n, D), device=dev,
                             generator=gen).float() / 16
        outs = [fn(ids, rows) for _, fn in VERSIONS]
        same = all(torch.equal(a, b) for a, b in zip(*outs))
        u = outs[0][0].numel()
        del outs
        for _, fn in VERSIONS:             # warm every (version, shape)
            for _ in range(3):
                fn(ids, rows)
        torch.cuda.synchronize()
        times = {label: [] for label, _ in VERSIONS}
        iters = {}
        for _ in range(args.reps):         # versions alternate in one process
            for label, fn in VERSIONS:
                s, it = window(lambda: fn(ids, rows), args.window)
                times[label].append(s)
                iters[label] = it
        med, spread = {}, {}
        for label, _ in VERSIONS:
            ts = sorted(times[label])
            med[label] = ts[len(ts) // 2]
            spread[label] = ts[-1] - ts[0]
            lines.append("%-46s %-26s %10.1f %8d   %.1f-%.1f"
                         % (label, "%d x %d, %s/%d" % (n, D, kind, V),
                            med[label] * 1e6, iters[label], ts[0] * 1e6,
                            ts[-1] * 1e6))
        k, c = VERSIONS[0][0], VERSIONS[1][0]
        lines.append("  same outputs: %s; composition / kernels = %.2f; "
                     "kernels no slower (median <= composition median + its "
                     "spread): %s"
                     % (same, med[c] / med[k], med[k] <= med[c] + spread[c]))
        lines.append("  u/n = %d/%d = %.3f; wire bytes of a push: %d coalesced "
                     "against %d (x %.2f)"
                     % (u, n, u / n, u * (8 + 2 * D), n * (8 + 2 * D), n / u))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
