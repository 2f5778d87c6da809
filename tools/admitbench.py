#!/usr/bin/env python
"""Time feature admission of a hashed embedding table (csrc/hash.hip: the
count / decide kernels of hash_find_or_admit, hash_gather_init and
hash_embedding_bag) and show what it buys.

Shape: capacity 2**20 rows (H = 2**21 slots), D = 64, Adagrad, requests of
n = 65536 keys — the shape of tools/hashbench.py and tools/evictbench.py.
Method of tools/hashbench.py: every version warmed up, windows of at least
--window seconds, versions alternating for --reps rounds, median reported
with min-max.

1. plain: push and training row pull (find_or_insert + init + gather) of a
   table WITHOUT admission on n held keys (uniform, all hits). With
   ``--only plain --rounds-json FILE`` these rounds alone are measured and
   written to FILE, and ``--package-root DIR`` imports tfmesos_amd from
   another checkout: that is how another commit is timed with this script.
   ``--base FILES`` / ``--this FILES`` put such files (processes started
   alternately by the caller) into the report: the difference of the
   medians against the min-max spread of the base's rounds.
2. steady push with admission: every key already has a row, so no position
   is flagged and the two extra n-lane launches (count, decide) find nothing
   to do; against the plain push on the same keys.
3. the fused serving kernels on all-hit keys: hash_gather_init against
   hash_gather; hash_embedding_bag (init given) against hash_find +
   embedding_bag, bags of 32. Bytes = the rows read + the rows written +
   8 bytes per key (the slot array traffic is not counted), over the time.
4. what admission buys (runs on the CPU too): a Zipf(1.1) stream of 64
   requests of n keys over 2**26 distinct keys into a table of 2**17 rows,
   for admit_after 1, 2, 3: rows held, dropped, filtered.

Nothing here has a threshold.

    python tools/admitbench.py --out profiles/hash_admit_bench.txt
"""

import argparse
import json
import os
import sys

import torch

CAPACITY = 2 ** 20
DIM = 64
N = 65536
BAG = 32
MULT = -7046029254386353131         # see tools/hashbench.py
STREAM_KEYS = 2 ** 26
STREAM_CAPACITY = 2 ** 17
STREAM_REQUESTS = 64


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
    return start.elapsed_time(end) * 1e-3 / iters


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def alternate(versions, args):
    """{label: [seconds per round]} with the versions alternating."""
    for _, fn in versions:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {label: [] for label, _ in versions}
    for _ in range(args.reps):
        for label, fn in versions:
            times[label].append(window(fn, args.window))
    return times


def fmt(label, ts, extra=""):
    return "  %-52s %9.1f us   %.1f-%.1f%s" % (
        label, median(ts) * 1e6, min(ts) * 1e6, max(ts) * 1e6, extra)


def held_table(cls, dev, gen, **kw):
    """A full table of CAPACITY rows and a request of N of its keys."""
    table = cls("h", DIM, CAPACITY, device=dev, lr=0.01, optimizer="adagrad",
                **kw)
    keys = torch.arange(1, CAPACITY + 1, device=dev) * MULT     # wraps
    table.index.assign(keys)
    table.master.normal_(generator=gen)
    table.shadow.copy_(table.master)
    return table, keys


def request(keys, dev, gen):
    req = keys[torch.randint(0, CAPACITY, (N,), device=dev, generator=gen)]
    grads = (torch.randint(-8, 9, (N, DIM), device=dev, generator=gen).float()
             / 1024).to(torch.bfloat16)
    return req, grads


def plain_rounds(cls, args, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    table, keys = held_table(cls, dev, gen)
    req, grads = request(keys, dev, gen)
    return alternate([("push", lambda: table.push(req, grads)),
                      ("pull", lambda: table.pull(req))], args)


def against_base(lines, base, this):
    lines.append("")
    lines.append("1. table WITHOUT admission, n = %d held keys: another "
                 "commit (base) against this one, %d + %d processes started "
                 "alternately" % (N, len(base), len(this)))
    for what in ("push", "pull"):
        b = [t for r in base for t in r[what]]
        t = [t for r in this for t in r[what]]
        lines.append(fmt("base  %s" % what, b))
        lines.append(fmt("this  %s" % what, t))
        diff = (median(t) - median(b)) * 1e6
        spread = (max(b) - min(b)) * 1e6
        lines.append("  %s: this - base = %+.1f us, spread of the base's "
                     "rounds %.1f us: %s"
                     % (what, diff, spread,
                        "inside" if diff <= spread else "OUTSIDE"))


def steady_push(lines, cls, args, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    plain, keys = held_table(cls, dev, gen)
    admit, _ = held_table(cls, dev, gen, admit_after=2)
    req, grads = request(keys, dev, gen)
    from tfmesos_amd import ops
    times = alternate([
        ("plain push", lambda: plain.push(req, grads)),
        ("push with admit_after=2", lambda: admit.push(req, grads)),
        ("one hash_find launch", lambda: ops.hash_find(plain.index, req)),
    ], args)
    lines.append("")
    lines.append("2. steady push of n = %d held keys (nothing flagged)" % N)
    for label, ts in times.items():
        lines.append(fmt(label, ts))
    lines.append("  admission overhead: %.1f us (two n-lane launches: count, "
                 "decide); one n-lane launch (hash_find): %.1f us"
                 % ((median(times["push with admit_after=2"]) -
                     median(times["plain push"])) * 1e6,
                    median(times["one hash_find launch"]) * 1e6))
    assert admit.stats()["filtered"] == 0


def serving(lines, cls, args, dev):
    from tfmesos_amd import ops
    gen = torch.Generator(device=dev).manual_seed(1)
    table, keys = held_table(cls, dev, gen)
    req, _ = request(keys, dev, gen)
    index, shadow = table.index, table.shadow
    offsets = torch.arange(0, N + 1, BAG, device=dev)
    init = (0, 1, 0)

    def two_launch_bag():
        return ops.embedding_bag(shadow, ops.hash_find(index, req), offsets)

    assert torch.equal(ops.hash_gather_init(index, shadow, req, 0),
                       ops.hash_gather(index, shadow, req))
    assert torch.equal(ops.hash_embedding_bag(index, shadow, req, offsets,
                                              init=init), two_launch_bag())
    times = alternate([
        ("hash_gather", lambda: ops.hash_gather(index, shadow, req)),
        ("hash_gather_init",
         lambda: ops.hash_gather_init(index, shadow, req, 0)),
        ("hash_find + embedding_bag", two_launch_bag),
        ("hash_embedding_bag(init=)",
         lambda: ops.hash_embedding_bag(index, shadow, req, offsets,
                                        init=init)),
    ], args)
    row_bytes = N * (2 * DIM * 2 + 8)
    bag_bytes = N * (DIM * 2 + 8) + (N // BAG) * DIM * 2
    lines.append("")
    lines.append("3. serving kernels, n = %d held keys (all hits), bf16 "
                 "[%d, %d] table; bags of %d" % (N, CAPACITY, DIM, BAG))
    for label, ts in times.items():
        nbytes = bag_bytes if "bag" in label else row_bytes
        lines.append(fmt(label, ts, "   %6.0f GB/s"
                         % (nbytes / median(ts) / 1e9)))
    lines.append("  hash_gather_init / hash_gather: %.2f; "
                 "hash_embedding_bag / (hash_find + embedding_bag): %.2f "
                 "(time ratios)"
                 % (median(times["hash_gather_init"]) /
                    median(times["hash_gather"]),
                    median(times["hash_embedding_bag(init=)"]) /
                    median(times["hash_find + embedding_bag"])))


def stream(lines, cls, dev):
    lines.append("")
    lines.append("4. Zipf(1.1) stream: %d pushes of n = %d keys over %d "
                 "distinct keys into %d rows (%s)"
                 % (STREAM_REQUESTS, N, STREAM_KEYS, STREAM_CAPACITY, dev))
    gen = torch.Generator().manual_seed(2)
    # inverse-CDF draw of a bounded power law with exponent 1.1
    a, hi = 0.1, float(STREAM_KEYS)
    reqs = []
    for _ in range(STREAM_REQUESTS):
        u = torch.rand(N, generator=gen, dtype=torch.float64)
        rank = (1.0 - u * (1.0 - hi ** -a)) ** (-1.0 / a)
        reqs.append((rank.long().clamp_(1, STREAM_KEYS) * MULT).to(dev))
    distinct = torch.cat(reqs).unique().numel()
    grads = torch.zeros(N, DIM, dtype=torch.bfloat16, device=dev)
    lines.append("  %d distinct keys in the stream" % distinct)
    for k in (1, 2, 3):
        table = cls("s", DIM, STREAM_CAPACITY, device=dev, lr=0.01,
                    optimizer="adagrad", admit_after=k)
        for req in reqs:
            table.push(req, grads)
        st = table.stats()
        lines.append("  admit_after=%d: rows held %7d  dropped %8d  "
                     "filtered %8d" % (k, st["size"], st["dropped"],
                                       st["filtered"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["plain", "stream"], default=None)
    ap.add_argument("--rounds-json", default=None)
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--base", nargs="*", default=[])
    ap.add_argument("--this", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root or os.path.dirname(
        os.path.dirname(os.path.abspath(__file__))))
    from tfmesos_amd.ps.sparse import HashedEmbeddingTable as cls
    if args.only == "stream":
        lines = []
        stream(lines, cls, "cuda:0" if torch.cuda.is_available() else "cpu")
        sys.stdout.write("\n".join(lines) + "\n")
        return
    assert torch.cuda.is_available(), "admitbench needs a GPU"
    dev = "cuda:0"
    if args.only == "plain":
        rounds = plain_rounds(cls, args, dev)
        with open(args.rounds_json, "w") as fh:
            json.dump(rounds, fh)
        for label, ts in rounds.items():
            print(fmt(label, ts))
        return
    lines = ["feature admission of a hashed table, capacity %d rows, D = %d, "
             "Adagrad, %s" % (CAPACITY, DIM, torch.cuda.get_device_name(0)),
             "windows >= %.2f s, %d alternating rounds, median (min-max)"
             % (args.window, args.reps)]
    if args.base and args.this:
        against_base(lines, [json.load(open(f)) for f in args.base],
                     [json.load(open(f)) for f in args.this])
    steady_push(lines, cls, args, dev)
    serving(lines, cls, args, dev)
    stream(lines, cls, dev)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
