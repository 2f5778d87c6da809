#!/usr/bin/env python
"""A/B of the sparse kernels between this tree and a second built tree:
same bits, same speed.

    python tools/sparse_ab.py /path/to/other/tree --out profiles/NAME.txt

The other tree is a checkout of the commit to compare against, built with
the same command. Every measurement runs in a fresh child process that
imports ONE tree (two builds of ``tfmesos_amd._C`` cannot share a process);
the children run one after the other, each under --child-timeout seconds,
and the tool stops at the first non-zero exit.

Same bits. Both trees run the same seeded, NON-dyadic cases (normal fp32 and
bf16 rows, whose sums depend on the order of summation):

* sparse_sgd / sparse_adagrad / sparse_adam in row mode and in bag mode
  (sum, and weighted mean), fp32 and bf16 gradients;
* segment_sum_rows, all four (rows, out) dtype pairs, and permute_rows;
* D in {7, 130, 256} with n = 2000 and one id repeated 1300 times, and the
  shapes tools/sparsebench.py times: 1000 x 200 with n = 256 and 4M x 256
  with n = 1M (one id on about 1 % of the positions).

A child saves every input and output tensor; the tool loads both files and
compares every pair with torch.equal. A tensor above 64 MiB is saved as two
wrapping int64 checksums of its bytes (plain sum and position-weighted sum)
instead of its 4 GiB, and those are compared. Any difference fails.

Same speed. The large shapes of tools/sparsebench.py, coalescebench.py and
partbench.py, by their method: device events, 3 warm-up calls, one window of
at least --window seconds per row and child; --reps rounds alternate the two
trees; median and min-max per row and tree. A row FAILS when this tree's
median is above the other tree's maximum (the other tree's own min-max
spread is the noise of the run; a spread of zero at the printed precision
counts as one unit of the last digit). A median below the other tree's
minimum is marked "faster". ``bench.py --workload nmf`` on both trees gives
the end-to-end lines.
"""

import argparse
import json
import os
import subprocess
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 64 << 20
SHAPES = [(500, 7, 2000, 1300), (500, 130, 2000, 1300),     # V, D, n, hot
          (500, 256, 2000, 1300), (1000, 200, 256, 0),
          (4 << 20, 256, 1 << 20, 10000)]
DEV = "cuda:0"


# ------------------------------------------------------------------ children

def keep(t):
    """What a child saves of a tensor: itself, or two checksums."""
    t = t.contiguous()
    if t.numel() * t.element_size() <= BIG:
        return t.cpu()
    b = t.view(-1).view(torch.uint8)
    if b.numel() % 8:       # zero-pad to whole int64 words
        b = torch.cat([b, b.new_zeros(8 - b.numel() % 8)])
    b = b.view(torch.int64)
    s1 = torch.zeros((), dtype=torch.int64, device=t.device)
    s2 = torch.zeros_like(s1)
    step = 1 << 24
    for i in range(0, b.numel(), step):
        c = b[i:i + step]
        w = torch.arange(i + 1, i + 1 + c.numel(), device=t.device)
        s1 += c.sum()
        s2 += (c * (2 * w + 1)).sum()
    return ("checksums", torch.stack([s1, s2]).cpu())


def make_ids(gen, V, n, hot):
    ids = torch.randint(0, V, (n,), device=DEV, generator=gen)
    if hot:
        ids[torch.randperm(n, device=DEV, generator=gen)[:hot]] = 12345 % V
    ids[:2] = torch.tensor([-1, V], device=DEV)     # ignored by the applies
    return ids


def make_bags(gen, n):
    """Offsets of B = n // 8 bags with random boundaries, and weights."""
    B = max(1, n // 8)
    cuts = torch.sort(torch.randint(0, n + 1, (B - 1,), device=DEV,
                                    generator=gen))[0]
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), cuts,
                         torch.full((1,), n, dtype=torch.int64, device=DEV)])
    return offsets, torch.rand(n, device=DEV, generator=gen) + 0.5


def apply_case(ops, opt, V, D, ids, grads, bag, gen):
    p = torch.rand(V, D, device=DEV, generator=gen)
    sh = p.to(torch.bfloat16)
    if opt == "sgd":
        st = []
        ops.sparse_sgd(p, ids, grads, 0.1, weight_decay=0.01, bf16_out=sh,
                       **bag)
    elif opt == "adagrad":
        st = [torch.rand(V, D, device=DEV, generator=gen)]
        ops.sparse_adagrad(p, ids, grads, st[0], 0.1, bf16_out=sh, **bag)
    else:
        st = [torch.rand(V, D, device=DEV, generator=gen) for _ in range(2)]
        ops.sparse_adam(p, ids, grads, st[0], st[1], 3, 0.01, bf16_out=sh,
                        **bag)
    return [p, sh] + st


def child_check(ops, out):
    saved = {}
    for V, D, n, hot in SHAPES:
        gen = torch.Generator(device=DEV).manual_seed(1000 + D + n)
        tag = "%dx%d n=%d" % (V, D, n)
        ids = make_ids(gen, V, n, hot)
        offsets, weights = make_bags(gen, n)
        B = offsets.numel() - 1
        rows = torch.randn(n, D, device=DEV, generator=gen)
        brows = torch.randn(B, D, device=DEV, generator=gen)
        saved[tag + " in"] = [keep(t) for t in (ids, offsets, weights, rows,
                                                brows)]
        modes = [("row", rows, {}),
                 ("bag sum", brows, dict(offsets=offsets)),
                 ("bag wmean", brows, dict(offsets=offsets, weights=weights,
                                           combiner="mean"))]
        for opt in ("sgd", "adagrad", "adam"):
            for mode, g, bag in modes:
                for dt in (torch.float32, torch.bfloat16):
                    outs = apply_case(ops, opt, V, D, ids, g.to(dt), bag, gen)
                    saved["%s %s %s %s" % (tag, opt, mode, dt)] = \
                        [keep(t) for t in outs]
                    del outs
        co = ops.coalesce_ids(ids)
        u = int(co.count)
        perm = torch.randint(-1, n + 1, (n,), device=DEV, generator=gen)
        for rdt in (torch.float32, torch.bfloat16):
            for odt in (torch.float32, torch.bfloat16):
                r = rows.to(rdt)
                saved["%s segment_sum %s %s" % (tag, rdt, odt)] = [keep(
                    ops.segment_sum_rows(r, co.perm, co.seg, u, odt))]
                saved["%s permute %s %s" % (tag, rdt, odt)] = [keep(
                    ops.permute_rows(r, perm, odt))]
    torch.cuda.synchronize()
    torch.save(saved, out)


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


def child_time(ops, out, min_s):
    V, D, n = 4 << 20, 256, 1 << 20
    gen = torch.Generator(device=DEV).manual_seed(0)
    uniform = torch.randint(0, V, (n,), device=DEV, generator=gen)
    skewed = uniform.clone()
    skewed[torch.rand(n, device=DEV, generator=gen) < 0.01] = 12345 % V
    grads = (torch.randn(n, D, device=DEV, generator=gen) * 0.01).to(
        torch.bfloat16)
    offsets, _ = make_bags(gen, n)
    bgrads = grads[:offsets.numel() - 1]
    p = torch.rand(V, D, device=DEV, generator=gen) / D ** 0.5
    sh = p.to(torch.bfloat16)
    s1, s2 = torch.zeros_like(p), torch.zeros_like(p)
    rows = []
    for name, ids in (("uniform", uniform), ("skewed", skewed)):
        rows += [
            ("sgd push, %s" % name,
             lambda ids=ids: ops.sparse_sgd(p, ids, grads, 0.01,
                                            bf16_out=sh)),
            ("adagrad push, %s" % name,
             lambda ids=ids: ops.sparse_adagrad(p, ids, grads, s1, 0.01,
                                                bf16_out=sh)),
            ("adam push, %s" % name,
             lambda ids=ids: ops.sparse_adam(p, ids, grads, s1, s2, 1, 0.01,
                                             bf16_out=sh))]
    rows.append(("adagrad pooled push, skewed",
                 lambda: ops.sparse_adagrad(p, skewed, bgrads, s1, 0.01,
                                            bf16_out=sh, offsets=offsets)))
    x = torch.rand(n, device=DEV, generator=gen, dtype=torch.float64)
    zipf = (float(V) ** x).long().clamp_(1, V) - 1
    frows = torch.randn(n, D, device=DEV, generator=gen)
    co = ops.coalesce_ids(zipf)
    u = int(co.count)
    rows.append(("segment_sum_rows fp32->bf16, zipf",
                 lambda: ops.segment_sum_rows(frows, co.perm, co.seg, u,
                                              torch.bfloat16)))
    part = ops.shard_partition(uniform, V, 8, "mod")
    rows.append(("permute_rows fp32->bf16, S=8",
                 lambda: ops.permute_rows(frows, part.perm, torch.bfloat16)))
    times = {}
    for label, fn in rows:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times[label] = window(fn, min_s)
    with open(out, "w") as fh:
        json.dump(times, fh)


def child(args):
    sys.path.insert(0, args.tree)
    from tfmesos_amd import ops
    assert os.path.abspath(ops.__file__).startswith(
        os.path.abspath(args.tree) + os.sep), ops.__file__
    ops._ext()      # raise now if the tree is not built
    assert torch.cuda.is_available(), "sparse_ab needs a GPU"
    if args.child == "check":
        child_check(ops, args.child_out)
    else:
        child_time(ops, args.child_out, args.window)


# -------------------------------------------------------------------- parent

def run(cmd, cwd, limit):
    """One child, under a time limit; a failure ends the tool."""
    try:
        r = subprocess.run(cmd, cwd=cwd, timeout=limit, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired:
        raise SystemExit("sparse_ab: %s ran past %d s" % (cmd, limit))
    if r.returncode != 0:
        sys.stdout.write(r.stdout[-4000:])
        raise SystemExit("sparse_ab: %s exited with %d" % (cmd, r.returncode))
    return r.stdout


def run_child(kind, tree, out, args):
    print("sparse_ab: %s child on %s" % (kind, tree), flush=True)
    run([sys.executable, os.path.abspath(__file__), tree, "--child", kind,
         "--child-out", out, "--window", str(args.window)], tree,
        args.child_timeout)


def fmt_ms(s):
    return "%.3f" % (s * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tree", help="the other built tree")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--nmf-steps", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default=None,
                    help="what the other tree is, for the report's first "
                         "line (default: its path)")
    ap.add_argument("--child",choices=["check", "time"], default=None)
    ap.add_argument("--child-out", default=None)
    args = ap.parse_args()
    args.tree = os.path.abspath(args.tree)
    if args.child:
        return child(args)
    trees = [("other", args.tree), ("this", HERE)]
    lines = ["sparse kernels, this tree against %s (\"other\")"
             % (args.label or args.tree)]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        saved = {}
        for label, tree in trees:
            path = os.path.join(tmp, "check_%s.pt" % label)
            run_child("check", tree, path, args)
            saved[label] = torch.load(path)
            os.remove(path)
        a, b = saved["other"], saved["this"]
        assert a.keys() == b.keys()
        whole = sums = 0
        for k in a:
            assert len(a[k]) == len(b[k])
            for i, (x, y) in enumerate(zip(a[k], b[k])):
                if isinstance(x, tuple):    # too large to save: checksums
                    sums += 1
                    x, y = x[1], y[1]
                else:
                    whole += 1
                if not torch.equal(x, y):
                    bad += 1
                    lines.append("DIFFERENT: %s, tensor %d" % (k, i))
        lines.append("same bits: %d cases; %d tensors compared whole with "
                     "torch.equal, %d tensors above %d MiB by their two int64 "
                     "checksums; %d differ"
                     % (len(a), whole, sums, BIG >> 20, bad))
        del saved, a, b
        times = {label: {} for label, _ in trees}
        for r in range(args.reps):          # the trees alternate
            for label, tree in trees:
                path = os.path.join(tmp, "time.json")
                run_child("time", tree, path, args)
                with open(path) as fh:
                    for k, v in json.load(fh).items():
                        times[label].setdefault(k, []).append(v)
    lines += ["", "same speed: 4M x 256 table, n = 1M, D = 256, %s; window >= "
              "%.2f s, %d alternating rounds of one process per tree"
              % (torch.cuda.get_device_name(0), args.window, args.reps),
              "%-36s %10s %17s %10s %17s  %s"
              % ("ms/call", "other med", "min-max", "this med", "min-max",
                 "verdict")]
    for k in times["other"]:
        o, t = sorted(times["other"][k]), sorted(times["this"][k])
        omed, tmed = o[len(o) // 2], t[len(t) // 2]
        # at the printed precision (us)
        lo, hi, mine = (round(x * 1e6) for x in (o[0], o[-1], tmed))
        verdict = "SLOWER" if mine > max(hi, lo + 1) else \
            "faster" if mine < lo else "within"
        bad += verdict == "SLOWER"
        lines.append("%-36s %10s %17s %10s %17s  %s"
                     % (k, fmt_ms(omed), "%s-%s" % (fmt_ms(o[0]), fmt_ms(o[-1])),
                        fmt_ms(tmed), "%s-%s" % (fmt_ms(t[0]), fmt_ms(t[-1])),
                        verdict))
    lines += ["", "bench.py --gpus 1 --workload nmf --steps %d --warmup 50"
              % args.nmf_steps]
    for label, tree in trees:
        outp = run([sys.executable, "bench.py", "--gpus", "1", "--workload",
                    "nmf", "--steps", str(args.nmf_steps), "--warmup", "50"],
                   tree, args.child_timeout)
        lines.append("%-5s %s" % (label, outp.strip().splitlines()[-1]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
