#!/usr/bin/env python
"""Time the worker-side routing of one push to a row-sharded table.

Versions, on the same ids [n] and fp32 gradient rows [n, D]:

* kernels:     ops.shard_partition + ops.permute_rows (csrc/partition.hip:
               count, cumsum, scatter, one permute+cast pass);
* composition: what a user writes without them — stable torch.sort of
               ids % S, bincount, cumsum, ids // S, index_select of ids and
               rows, cast to bf16.

Both end with the shard-local ids and the bf16 rows in wire order plus the
shard boundaries on the device; neither copies anything to the host.

Shapes: n = 1M, D = 256, S = 8 (a large push) and n = 256, D = 200, S = 2
(a small one, where time is launches).

Method (that of tools/sparsebench.py): device events; every (version,
shape) is warmed up; each timing window lasts at least --window seconds;
the versions alternate inside one process (--reps rounds) and the median
round is reported.

    python tools/partbench.py --out profiles/partition_bench.txt
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd import ops  # noqa: E402

SHAPES = [(1024 * 1024, 256, 8), (256, 200, 2)]    # n, D, S


def kernels(ids, rows, V, S):
    part = ops.shard_partition(ids, V, S, "mod")
    return part.local, ops.permute_rows(rows, part.perm, torch.bfloat16), \
        part.starts


def composition(ids, rows, V, S):
    shard = ids % S
    perm = torch.sort(shard, stable=True)[1]
    starts = torch.zeros(S + 1, dtype=torch.int64, device=ids.device)
    starts[1:] = torch.bincount(shard, minlength=S).cumsum(0)
    local = torch.div(ids, S, rounding_mode="floor").index_select(0, perm)
    return local, rows.index_select(0, perm).to(torch.bfloat16), starts


VERSIONS = [("kernels (shard_partition + permute_rows)", kernels),
            ("composition (sort/bincount/index_select)", composition)]


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
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "partbench needs a GPU"
    dev = "cuda:0"
    V = args.rows
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = ["shard routing of one push: table of %d rows, strategy mod, "
             "fp32 rows -> bf16 wire rows, %s"
             % (V, torch.cuda.get_device_name(0)),
             "window >= %.2f s, %d alternating rounds, median reported"
             % (args.window, args.reps),
             "%-42s %-22s %10s %8s   %s" % ("version", "n x D, S", "us/call",
                                            "iters", "min-max us")]
    for n, D, S in SHAPES:
        ids = torch.randint(0, V, (n,), device=dev, generator=gen)
        rows = torch.randn(n, D, device=dev, generator=gen)
        outs = [fn(ids, rows, V, S) for _, fn in VERSIONS]
        same = all(torch.equal(a, b) for a, b in zip(*outs))
        for _, fn in VERSIONS:             # warm every (version, shape)
            for _ in range(3):
                fn(ids, rows, V, S)
        torch.cuda.synchronize()
        times = {label: [] for label, _ in VERSIONS}
        iters = {}
        for _ in range(args.reps):         # versions alternate in one process
            for label, fn in VERSIONS:
                s, it = window(lambda: fn(ids, rows, V, S), args.window)
                times[label].append(s)
                iters[label] = it
        med = {}
        for label, _ in VERSIONS:
            ts = sorted(times[label])
            med[label] = ts[len(ts) // 2]
            lines.append("%-42s %-22s %10.1f %8d   %.1f-%.1f"
                         % (label, "%d x %d, S=%d" % (n, D, S),
                            med[label] * 1e6, iters[label], ts[0] * 1e6,
                            ts[-1] * 1e6))
        lines.append("  same outputs: %s; composition / kernels = %.2f"
                     % (same, med[VERSIONS[1][0]] / med[VERSIONS[0][0]]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
