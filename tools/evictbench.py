#!/usr/bin/env python
"""Time eviction from a hashed embedding table (csrc/hash.hip: use stamps,
compaction by hole filling, rebuild).

Shape: capacity 2**20 rows (H = 2**21 slots), D = 64, Adagrad (master fp32,
shadow bf16, accumulator fp32: 640 bytes per row), a FULL table of which a
random 1 %, 10 % or 50 % of the rows is idle and goes in one
``HashedEmbeddingTable.evict(max_idle=)``.

* evict, total: device events around one call; before every call row_keys,
  size and the stamps are put back (untimed; the compaction reads nothing
  else, the slot arrays are rebuilt by the call itself).
* per kernel: the same call under torch.profiler, device time per kernel
  name, averaged over --prof-iters calls. The torch kernels of one call
  (the keep mask, the scan of the flags, the slot clear) are summed as
  "torch plumbing".
* move kernel rate: (bytes read + bytes written) / move kernel time, the
  bytes being pairs * 2 * (640 + 16): every row tensor's row, the key and
  the stamp. Yardstick in the same run: ops.embedding_gather (a kernel that
  predates eviction) of the same number of random rows of a bf16 [2**20, 64]
  table, event-timed over a window, as pairs * 2 * 128 bytes / time.
* stamp overhead: HashedEmbeddingTable.push of n = 65536 held keys (uniform,
  all hits) with and without use tracking, steady state, and one
  ops.hash_find launch on the same keys — the floor for "one more launch of
  n lanes". Method of tools/hashbench.py: every version warmed up, windows
  of at least --window seconds, versions alternating for --reps rounds,
  median reported with min-max.

Nothing here has a threshold.

    python tools/evictbench.py --out profiles/hash_evict_bench.txt
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd import ops  # noqa: E402
from tfmesos_amd.ps.sparse import HashedEmbeddingTable  # noqa: E402

CAPACITY = 2 ** 20
DIM = 64
N = 65536
FRACTIONS = [0.01, 0.10, 0.50]
ROW_BYTES = DIM * (4 + 2 + 4)       # master, shadow, accumulator
MULT = -7046029254386353131         # see tools/hashbench.py
OURS = ["keep_flag_kernel", "plan_kernel", "move_kernel", "finalize_kernel",
        "rebuild_kernel"]


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


def single_calls(reset, fn, iters):
    """Seconds of each of ``iters`` calls of fn, each after an untimed
    reset."""
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    out = []
    for _ in range(iters):
        reset()
        start.record()
        fn()
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end) * 1e-3)
    return sorted(out)


def kernel_times(reset, fn, iters):
    """{kernel name: (seconds per call, launches per call)} from
    torch.profiler, device activity only."""
    from torch.profiler import ProfilerActivity, profile
    total, count = {}, {}
    for _ in range(iters):
        reset()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            if t is None:
                t = getattr(ev, "cuda_time_total", 0)
            if t <= 0:
                continue
            total[ev.key] = total.get(ev.key, 0.0) + t * 1e-6
            count[ev.key] = count.get(ev.key, 0) + ev.count
    return {k: (total[k] / iters, count[k] / iters) for k in total}


def median(ts):
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--prof-iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "evictbench needs a GPU"
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = ["eviction from a full hashed table, capacity %d rows, D = %d, "
             "Adagrad (%d bytes per row), %s"
             % (CAPACITY, DIM, ROW_BYTES, torch.cuda.get_device_name(0)),
             "evict: %d single calls, median (min-max); kernels: "
             "torch.profiler device time, mean of %d calls"
             % (args.iters, args.prof_iters)]
    kw = dict(device=dev, lr=0.01, optimizer="adagrad")
    table = HashedEmbeddingTable("h", DIM, CAPACITY, track_use=True, **kw)
    keys = torch.arange(1, CAPACITY + 1, device=dev) * MULT     # wraps
    table.index.assign(keys)
    table.master.normal_(generator=gen)
    table.step = 100
    gather_table = torch.randn(CAPACITY, DIM, device=dev,
                               generator=gen).to(torch.bfloat16)
    for frac in FRACTIONS:
        idle = torch.rand(CAPACITY, device=dev, generator=gen) < frac
        stamps = torch.where(idle, 0, 100)
        evicted = int(idle.sum())
        K = CAPACITY - evicted
        pairs = int((~idle[K:]).sum())

        def reset():
            table.index.row_keys.copy_(keys)
            table.index.size.fill_(CAPACITY)
            table.last_used.copy_(stamps)

        def evict():
            table.evict(max_idle=50)

        for _ in range(3):
            reset()
            evict()
        assert table.stats()["size"] == K
        found = ops.hash_find(table.index, keys)
        assert bool(((found >= 0) == ~idle).all())
        ts = single_calls(reset, evict, args.iters)
        lines.append("")
        lines.append("evict %4.0f %%: %d rows go, %d stay, %d (hole, mover) "
                     "pairs" % (frac * 100, evicted, K, pairs))
        lines.append("  %-44s %10.1f us   %.1f-%.1f"
                     % ("evict(max_idle=), total", median(ts) * 1e6,
                        ts[0] * 1e6, ts[-1] * 1e6))
        kt = kernel_times(reset, evict, args.prof_iters)
        if not kt:
            raise SystemExit("evictbench: torch.profiler reported no device "
                             "activity; per-kernel times are unavailable")
        plumbing, launches, move = 0.0, 0.0, None
        for name, (sec, cnt) in sorted(kt.items()):
            mine = [k for k in OURS if k in name]
            if not mine:
                plumbing += sec
                launches += cnt
                continue
            lines.append("  %-44s %10.1f us   x%g" % (mine[0], sec * 1e6, cnt))
            if mine[0] == "move_kernel":
                move = sec
        lines.append("  %-44s %10.1f us   x%g"
                     % ("torch plumbing (mask, scan, slot clear)",
                        plumbing * 1e6, launches))
        lines.append("  %-44s %10.1f us"
                     % ("sum of the kernels",
                        sum(s for s, _ in kt.values()) * 1e6))
        rows = torch.randint(0, CAPACITY, (max(pairs, 1),), device=dev,
                             generator=gen)
        for _ in range(3):
            ops.embedding_gather(gather_table, rows)
        gs = sorted(window(lambda: ops.embedding_gather(gather_table, rows),
                           args.window)[0] for _ in range(args.reps))
        move_bytes = pairs * 2 * (ROW_BYTES + 16)
        gather_bytes = pairs * 2 * DIM * 2
        move_rate = move_bytes / move
        gather_rate = gather_bytes / median(gs)
        lines.append("  move kernel: %.1f MB in %.1f us = %.0f GB/s; "
                     "embedding_gather of %d random bf16 rows: %.1f MB in "
                     "%.1f us = %.0f GB/s; ratio %.2f"
                     % (move_bytes / 1e6, move * 1e6, move_rate / 1e9, pairs,
                        gather_bytes / 1e6, median(gs) * 1e6,
                        gather_rate / 1e9, move_rate / gather_rate))
    # ---- stamp overhead of a push
    del table, gather_table
    tracked = HashedEmbeddingTable("a", DIM, CAPACITY, track_use=True, **kw)
    plain = HashedEmbeddingTable("b", DIM, CAPACITY, **kw)
    for t in (tracked, plain):
        t.index.assign(keys)
    req = keys[torch.randint(0, CAPACITY, (N,), device=dev, generator=gen)]
    grads = (torch.randint(-8, 9, (N, DIM), device=dev, generator=gen).float()
             / 1024).to(torch.bfloat16)
    versions = [
        ("tracked push (find_or_insert+init+touch+apply)",
         lambda: tracked.push(req, grads)),
        ("untracked push", lambda: plain.push(req, grads)),
        ("one hash_find launch", lambda: ops.hash_find(plain.index, req)),
    ]
    for _, fn in versions:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {label: [] for label, _ in versions}
    iters = {}
    for _ in range(args.reps):
        for label, fn in versions:
            s, it = window(fn, args.window)
            times[label].append(s)
            iters[label] = it
    lines.append("")
    lines.append("push of n = %d held keys (uniform, all hits), steady, "
                 "window >= %.2f s, %d alternating rounds, median"
                 % (N, args.window, args.reps))
    med = {}
    for label, _ in versions:
        ts = sorted(times[label])
        med[label] = median(ts)
        lines.append("  %-48s %10.1f us %8d   %.1f-%.1f"
                     % (label, median(ts) * 1e6, iters[label], ts[0] * 1e6,
                        ts[-1] * 1e6))
    lines.append("  stamp overhead (tracked - untracked): %.1f us; one "
                 "n-lane launch (hash_find): %.1f us"
                 % ((med[versions[0][0]] - med[versions[1][0]]) * 1e6,
                    med[versions[2][0]] * 1e6))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
