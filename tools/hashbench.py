#!/usr/bin/env python
"""Time what the key index of a hashed embedding table costs per request.

A ``HashedEmbeddingTable`` request is a key -> row translation
(csrc/hash.hip) followed by the row op an ``EmbeddingTable`` runs. The tool
times, on the same keys,

* hashed pull:     HashedEmbeddingTable.pull, insert_on_pull=True (training:
                   find_or_insert + init of new rows + gather);
* serving pull:    HashedEmbeddingTable.pull, insert_on_pull=False (the one
                   launch ops.hash_gather);
* hashed push:     HashedEmbeddingTable.push (find_or_insert + init + fused
                   Adagrad apply);
* dense pull/push: EmbeddingTable(fused_apply=True).pull / .push given the
                   ALREADY TRANSLATED rows of the same request.

hashed - dense is the cost of the index. Nothing here has a threshold.

Shape: H = 2**21 slots (capacity 2**20 rows), D = 64, n = 65536 keys per
request, Adagrad. The table holds load * H keys: load 0.25 (half full) and
0.5 (full, the maximum load). Keys are distinct int64 spread over the whole
range; a request draws them uniformly or Zipf-like (log-uniform rank, P(rank
k) ~ 1/k) from the keys the table holds.

* steady state: every key of the request has a row (all hits).
* cold: the table holds load * H - n keys and the request is n keys it has
  never seen (all inserts; distinct, so uniform only). Between two timed
  calls the index is put back (HashIndex.assign, untimed); a call is timed
  on its own with device events and the calls of a window are summed.

Method (that of tools/coalescebench.py): device events; every version is
warmed up; a steady-state window lasts at least --window seconds; the
versions alternate inside one process (--reps rounds) and the median round
is reported with its min-max.

    python tools/hashbench.py --out profiles/hash_bench.txt
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd import ops  # noqa: E402
from tfmesos_amd.ps.sparse import (  # noqa: E402
    EmbeddingTable, HashedEmbeddingTable)

SLOTS = 2 ** 21
DIM = 64
N = 65536
LOADS = [0.25, 0.5]
MULT = -7046029254386353131     # 0x9E3779B97F4A7C15 as int64: odd, so
                                # i -> i * MULT is a bijection of int64


def make_keys(count, dev):
    keys = torch.arange(1, count + 1, device=dev) * MULT    # wraps
    assert not bool((keys == ops.HASH_EMPTY).any())
    return keys


def draw(kind, held, gen):
    """N keys of ``held`` [m]: uniform or log-uniform rank."""
    m = held.numel()
    if kind == "uniform":
        return held[torch.randint(0, m, (N,), device=held.device,
                                  generator=gen)]
    x = torch.rand(N, device=held.device, generator=gen, dtype=torch.float64)
    return held[(float(m) ** x).long().clamp_(1, m) - 1]


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


def cold_window(reset, fn, iters):
    """Seconds per call of ``fn`` over ``iters`` calls, each after an
    untimed ``reset`` and timed on its own."""
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    total = 0.0
    for _ in range(iters):
        reset()
        start.record()
        fn()
        end.record()
        end.synchronize()
        total += start.elapsed_time(end) * 1e-3
    return total / iters, iters


def report(lines, label, what, ts, iters):
    ts = sorted(ts)
    lines.append("%-34s %-30s %10.1f %8d   %.1f-%.1f"
                 % (label, what, ts[len(ts) // 2] * 1e6, iters, ts[0] * 1e6,
                    ts[-1] * 1e6))
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cold-iters", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hashbench needs a GPU"
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    capacity = SLOTS // 2
    lines = ["hashed against dense embedding table, per request of n = %d "
             "keys, D = %d, H = %d slots, Adagrad, %s"
             % (N, DIM, SLOTS, torch.cuda.get_device_name(0)),
             "steady: window >= %.2f s; cold: %d single calls; %d "
             "alternating rounds, median reported"
             % (args.window, args.cold_iters, args.reps),
             "%-34s %-30s %10s %8s   %s" % ("version", "load, keys", "us/call",
                                            "iters", "min-max us")]
    kw = dict(device=dev, lr=0.01, optimizer="adagrad")
    train = HashedEmbeddingTable("h", DIM, capacity, **kw)
    serve = HashedEmbeddingTable("s", DIM, capacity, insert_on_pull=False,
                                 **kw)
    dense = EmbeddingTable("d", capacity, DIM, fused_apply=True, **kw)
    assert train.index.slot_keys.numel() == SLOTS
    grads = (torch.randint(-8, 9, (N, DIM), device=dev, generator=gen).float()
             / 1024).to(torch.bfloat16)
    all_keys = make_keys(capacity + N, dev)
    for load in LOADS:
        fill = int(load * SLOTS)
        held, fresh = all_keys[:fill], all_keys[capacity:]
        for t in (train, serve):
            t.index.assign(held)
        for kind in ("uniform", "zipf"):
            keys = draw(kind, held, gen)
            rows = ops.hash_find(train.index, keys)
            assert bool((rows >= 0).all())
            assert torch.equal(rows, ops.hash_find_or_insert(train.index,
                                                             keys)[0])
            versions = [
                ("hashed pull (find_or_insert)", lambda: train.pull(keys)),
                ("serving pull (hash_gather)", lambda: serve.pull(keys)),
                ("dense pull (rows given)", lambda: dense.pull(rows)),
                ("hashed push", lambda: train.push(keys, grads)),
                ("dense push (rows given)", lambda: dense.push(rows, grads)),
            ]
            what = "%.2f, steady %s" % (load, kind)
            for _, fn in versions:             # warm every version
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {label: [] for label, _ in versions}
            iters = {}
            for _ in range(args.reps):         # versions alternate
                for label, fn in versions:
                    s, it = window(fn, args.window)
                    times[label].append(s)
                    iters[label] = it
            med = {label: report(lines, label, what, times[label],
                                 iters[label]) for label, _ in versions}
            distinct = torch.unique(keys).numel()
            lines.append(
                "  %d distinct keys; index cost (hashed - dense): pull %.1f "
                "us, serving pull %.1f us, push %.1f us"
                % (distinct,
                   (med[versions[0][0]] - med[versions[2][0]]) * 1e6,
                   (med[versions[1][0]] - med[versions[2][0]]) * 1e6,
                   (med[versions[3][0]] - med[versions[4][0]]) * 1e6))
        # cold: n never-seen keys bring the table from fill - n to fill
        base = held[:fill - N]
        rows = torch.arange(fill - N, fill, device=dev)

        def reset():
            train.index.assign(base)

        versions = [
            ("hashed pull (all inserts)", reset, lambda: train.pull(fresh)),
            ("dense pull (rows given)", lambda: None,
             lambda: dense.pull(rows)),
            ("hashed push (all inserts)", reset,
             lambda: train.push(fresh, grads)),
            ("dense push (rows given)", lambda: None,
             lambda: dense.push(rows, grads)),
        ]
        what = "%.2f, cold uniform" % load
        for _, rs, fn in versions:
            for _ in range(3):
                rs()
                fn()
        torch.cuda.synchronize()
        reset()
        got = ops.hash_find_or_insert(train.index, fresh)
        assert torch.equal(got[0], rows) and bool(got[1].all())
        times = {label: [] for label, _, _ in versions}
        for _ in range(args.reps):
            for label, rs, fn in versions:
                times[label].append(cold_window(rs, fn, args.cold_iters)[0])
        med = {label: report(lines, label, what, times[label],
                             args.cold_iters) for label, _, _ in versions}
        lines.append("  index cost (hashed - dense): pull %.1f us, push %.1f us"
                     % ((med[versions[0][0]] - med[versions[1][0]]) * 1e6,
                        (med[versions[2][0]] - med[versions[3][0]]) * 1e6))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
