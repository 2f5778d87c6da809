#!/usr/bin/env python
"""Time one EmbeddingTable.push at a size a user would run.

Table 4M x 256 (fp32 master + bf16 shadow + optimizer state), n = 1M
pushed rows of bf16 grads, two id sets:

* uniform: ids uniform over the table;
* skewed:  the same, with one id on about 1 % of the contributions.

Versions: plain SGD through the scatter-add path (fused_apply=False —
fp32 atomics + unique + shadow refresh) against the fused sparse-apply
kernel (fused_apply=True), plus Adagrad, Adam and FTRL-Proximal (fused
kernel only; FTRL-Proximal moves Adam's bytes, so the Adam row is its
yardstick and the ratio is printed).

Method: device events; every (version, id set) is warmed up; each timing
window lasts at least --window seconds; the versions alternate inside
one process (--reps rounds) and the median round is reported. Bytes are
computed from the shapes (ids + grads read once, and per touched row:
master read+write, shadow write, each state tensor read+write), so the
bytes/s column is useful traffic, not a counter reading.

    python tools/sparsebench.py --out profiles/sparse_apply_bench.txt
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd.ps.sparse import EmbeddingTable  # noqa: E402

VERSIONS = [
    ("sgd scatter-add (fused_apply=False)", "sgd", {}),
    ("sgd fused       (fused_apply=True)", "sgd", {"fused_apply": True}),
    ("adagrad fused", "adagrad", {}),
    ("adam fused", "adam", {}),
    ("ftrl_proximal fused", "ftrl_proximal", {"l1": 0.001, "l2": 0.001}),
]


def big_table(rows, dim, dev, optimizer, hp):
    """An EmbeddingTable whose buffers are generated on the device (the
    constructor's seeded host init of 1G elements is setup time this
    tool does not need)."""
    t = EmbeddingTable("bench", 1, dim, device=dev, lr=0.01,
                       optimizer=optimizer, **hp)
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
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sparsebench needs a GPU"
    dev = "cuda:0"
    V, D, n = args.rows, args.dim, args.n

    gen = torch.Generator(device=dev).manual_seed(0)
    uniform = torch.randint(0, V, (n,), device=dev, generator=gen)
    skewed = uniform.clone()
    hot = torch.rand(n, device=dev, generator=gen) < 0.01
    skewed[hot] = 12345 % V
    grads = (torch.randn(n, D, device=dev, generator=gen) * 0.01).to(
        torch.bfloat16)
    idsets = [("uniform", uniform), ("skewed", skewed)]
    touched = {k: int(torch.unique(v).numel()) for k, v in idsets}

    lines = ["sparse push: table %d x %d, n = %d bf16 grad rows, %s"
             % (V, D, n, torch.cuda.get_device_name(0)),
             "hot id share (skewed): %.2f %% of contributions; touched rows:"
             " uniform %d, skewed %d"
             % (100.0 * float(hot.float().mean()), touched["uniform"],
                touched["skewed"]),
             "window >= %.2f s, %d alternating rounds, median reported"
             % (args.window, args.reps),
             "%-38s %-8s %10s %10s %7s   %s" % ("version", "ids", "ms/push",
                                                "GB/s", "iters",
                                                "min-max ms")]
    tables = [(label, big_table(V, D, dev, opt, hp))
              for label, opt, hp in VERSIONS]
    median = {}
    for idname, ids in idsets:
        for _, t in tables:            # warm every (version, id set)
            for _ in range(3):
                t.push(ids, grads)
        torch.cuda.synchronize()
        times = {label: [] for label, _ in tables}
        iters = {}
        for _ in range(args.reps):     # versions alternate in one process
            for label, t in tables:
                s, it = window(lambda: t.push(ids, grads), args.window)
                times[label].append(s)
                iters[label] = it
        for label, t in tables:
            ts = sorted(times[label])
            s = median[(label, idname)] = ts[len(ts) // 2]
            nbytes = n * (8 + 2 * D) + touched[idname] * D * (
                4 + 4 + 2 + 8 * len(t.state))
            lines.append("%-38s %-8s %10.3f %10.1f %7d   %.3f-%.3f"
                         % (label, idname, s * 1e3, nbytes / s / 1e9,
                            iters[label], ts[0] * 1e3, ts[-1] * 1e3))
    for idname, _ in idsets:
        f = median[("ftrl_proximal fused", idname)]
        a = median[("adam fused", idname)]
        lines.append("ftrl_proximal / adam (%s): %.3f ms / %.3f ms = %.3f"
                     % (idname, f * 1e3, a * 1e3, f / a))
    # same result? one push of each SGD version from identical state, at
    # the timed size (the atomics' arrival order may move last bits)
    del tables
    a = big_table(V, D, dev, "sgd", {})
    b = big_table(V, D, dev, "sgd", {"fused_apply": True})
    b.master.copy_(a.master)
    b.shadow.copy_(a.shadow)
    for idname, ids in idsets:
        a.push(ids, grads)
        b.push(ids, grads)
        lines.append("sgd scatter-add vs fused after one more push (%s): "
                     "max |master diff| %.3g, shadow rows differing %d"
                     % (idname, float((a.master - b.master).abs().max()),
                        int((a.shadow != b.shadow).any(1).sum())))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
