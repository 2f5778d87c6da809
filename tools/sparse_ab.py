#!/usr/bin/env python
"""A/B of one kernel family between this tree and a second built tree:
same bits, same speed. --suite sparse (the default) is described first;
--suite bn, the batch-norm kernels, at the end.

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

--suite bn. Same bits: bn_fwd then bn_bwd on seeded normal inputs, for the
shapes of tests/test_kernels_gpu.py (one per kernel path) and one per
Inception stage, relu on and off, with dense and with channel-narrow out /
dy; and ops.bn_group_apply (joined) and ops.bn_group_multi over the block-A
widths at 35 x 35. Saved per case: y, mean, invstd, dx, dgamma, dbeta;
tensors above 8 MiB as checksums. Same speed: forward and backward of the
Inception-stage and grouped cases, by the rule above. End to end:
``bench.py --workload inception`` on both trees, with every array of
--dump-outputs compared for equality. The other tree runs the same-bits
cases and the benchmark twice: a case or array that it does not reproduce
itself (a kernel with a data race) is reported as such and not compared.
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

def keep(t, big=BIG):
    """What a child saves of a tensor: itself, or two checksums."""
    t = t.contiguous()
    if t.numel() * t.element_size() <= big:
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


# -------------------------------------------------------------- bn children

BN_BIG = 8 << 20
BN_UNIT = [(4, 16, 14, 14), (2, 64, 35, 35), (8, 32, 7, 9), (1, 7, 5, 5),
           (2, 20, 5, 7), (4, 48, 104, 104), (2, 256, 64, 64),
           (2, 2048, 72, 72)]
BN_STAGES = [(32, 32, 147, 147), (32, 192, 35, 35), (32, 768, 17, 17),
             (32, 2048, 8, 8)]
BN_GROUP = (32, [64, 64, 96, 32], 35, 35)       # Inception block A


def cl_randn(gen, shape, narrow=False):
    """Seeded normal bf16 NCHW tensor in channels-last memory; narrow: as a
    channel slice of a wider buffer (kept 16-byte aligned when C % 8 == 0)."""
    N, C, H, W = shape
    pad, off = (16, 8) if C % 8 == 0 else (5, 3)
    wide = C + pad if narrow else C
    t = torch.randn(N, H, W, wide, device=DEV, generator=gen).to(
        torch.bfloat16).permute(0, 3, 1, 2)
    return t.narrow(1, off, C) if narrow else t


def bn_params(gen, C):
    g = (torch.rand(C, device=DEV, generator=gen) + 0.5).to(torch.bfloat16)
    b = (torch.randn(C, device=DEV, generator=gen) * 0.2).to(torch.bfloat16)
    return g, b


def bn_single(ext, gen, shape, relu, narrow):
    """bn_fwd + bn_bwd -> [y, mean, invstd, dx, dgamma, dbeta]."""
    x = cl_randn(gen, shape)
    g, b = bn_params(gen, shape[1])
    out = cl_randn(gen, shape, True) if narrow else \
        torch.empty(0, device=DEV, dtype=torch.bfloat16)
    dy = cl_randn(gen, shape, narrow)
    y, mean, invstd = ext.bn_fwd(x, g, b, 1e-3, relu, out)
    return [y, mean, invstd] + list(ext.bn_bwd(x, dy, g, b, mean, invstd,
                                               relu))


def bn_group_case(gen, joined):
    """Inputs of one grouped case: (xs, ws, bs), the view a joined forward
    writes into (a channel-narrow slice of a wider concat buffer; None for
    multi) and seeded gradients for the output(s)."""
    N, Cs, H, W = BN_GROUP
    xs = [cl_randn(gen, (N, c, H, W)).requires_grad_(True) for c in Cs]
    ps = [bn_params(gen, c) for c in Cs]
    ws = [g.requires_grad_(True) for g, _ in ps]
    bs = [b.requires_grad_(True) for _, b in ps]
    if joined:
        view = cl_randn(gen, (N, sum(Cs) + 64, H, W)).narrow(1, 32, sum(Cs))
        dys = [cl_randn(gen, (N, sum(Cs), H, W), True)]
    else:
        view = None
        dys = [cl_randn(gen, (N, c, H, W), i % 2 == 1)
               for i, c in enumerate(Cs)]
    return (xs, ws, bs), view, dys


def bn_group_fwd(ops, inputs, view, relu):
    if view is not None:
        return [ops.bn_group_apply(view, *inputs, eps=1e-3, relu=relu)]
    return list(ops.bn_group_multi(*inputs, eps=1e-3, relu=relu))


def bn_child_check(ops, out):
    ext = ops._ext()
    saved = {}
    for shape in BN_UNIT + BN_STAGES:
        for relu in (False, True):
            for narrow in (False, True):
                gen = torch.Generator(device=DEV).manual_seed(
                    2000 + shape[1] + shape[2])
                saved["%s relu=%d %s" % (shape, relu, "narrow" if narrow
                                         else "dense")] = \
                    [keep(t, BN_BIG) for t in bn_single(ext, gen, shape, relu,
                                                        narrow)]
    for relu in (False, True):
        for joined in (True, False):
            gen = torch.Generator(device=DEV).manual_seed(3000)
            inputs, view, dys = bn_group_case(gen, joined)
            ys = bn_group_fwd(ops, inputs, view, relu)
            mean, invstd = ys[0].grad_fn.saved_tensors[:2]
            grads = torch.autograd.grad(ys, sum(inputs, []), dys)
            saved["group %s relu=%d" % ("joined" if joined else "multi",
                                        relu)] = \
                [keep(t, BN_BIG) for t in ys + [mean, invstd] + list(grads)]
    torch.cuda.synchronize()
    torch.save(saved, out)


def bn_child_time(ops, out, min_s):
    ext = ops._ext()
    gen = torch.Generator(device=DEV).manual_seed(0)
    none = torch.empty(0, device=DEV, dtype=torch.bfloat16)
    rows = []
    for shape in BN_STAGES:
        x, dy = cl_randn(gen, shape), cl_randn(gen, shape)
        g, b = bn_params(gen, shape[1])
        _, mean, invstd = ext.bn_fwd(x, g, b, 1e-3, True, none)
        rows += [
            ("fwd %dx%dx%dx%d" % shape,
             lambda x=x, g=g, b=b: ext.bn_fwd(x, g, b, 1e-3, True, none)),
            ("bwd %dx%dx%dx%d" % shape,
             lambda x=x, dy=dy, g=g, b=b, mean=mean, invstd=invstd:
             ext.bn_bwd(x, dy, g, b, mean, invstd, True))]
    for joined in (True, False):
        name = "group %s %s" % ("joined" if joined else "multi",
                                "+".join(map(str, BN_GROUP[1])))
        inputs, view, dys = bn_group_case(gen, joined)
        ys = bn_group_fwd(ops, inputs, view, True)
        rows += [
            ("fwd " + name,
             lambda inputs=inputs, view=view: bn_group_fwd(ops, inputs, view,
                                                           True)),
            ("bwd " + name,
             lambda ys=ys, dys=dys, inputs=inputs: torch.autograd.grad(
                 ys, sum(inputs, []), dys, retain_graph=True))]
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
    suite = SUITES[args.suite]
    if args.child == "check":
        suite["check"](ops, args.child_out)
    else:
        suite["time"](ops, args.child_out, args.window)


def nmf_bench(args, dump):
    return ["--workload", "nmf", "--steps", str(args.nmf_steps), "--warmup",
            "50"]


def inception_bench(args, dump):
    return ["--workload", "inception", "--steps", "20", "--warmup", "5",
            "--dump-outputs", dump]


def same_dumps(tmp):
    """Compare the trees' --dump-outputs arrays: (report line, differ). An
    array that two runs of the other tree do not reproduce is left out."""
    import numpy as np
    dirs = [os.path.join(tmp, "dump_" + t) for t in ("other", "this",
                                                     "other again")]
    names = sorted(os.listdir(dirs[0]))
    assert names and all(names == sorted(os.listdir(d)) for d in dirs[1:])

    def differ(a, b):
        return [n for n in names if not np.array_equal(
            np.load(os.path.join(a, n)), np.load(os.path.join(b, n)))]
    unstable = differ(dirs[0], dirs[2])
    diff = [n for n in differ(dirs[0], dirs[1]) if n not in unstable]
    return ("--dump-outputs: %d arrays compared for equality; %d differ%s; "
            "%d left out, which two runs of the other tree do not "
            "reproduce%s"
            % (len(names), len(diff), "".join(" " + n for n in diff),
               len(unstable), "".join(" " + n for n in unstable)), len(diff))


SUITES = {
    "sparse": dict(
        title="sparse kernels", check=child_check, time=child_time, big=BIG,
        speed="4M x 256 table, n = 1M, D = 256", bench=nmf_bench),
    "bn": dict(
        title="batch-norm kernels", check=bn_child_check, time=bn_child_time,
        big=BN_BIG, speed="Inception-stage layers and block-A groups, relu",
        bench=inception_bench, dumps=same_dumps, repeat=True),
}


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
         "--child-out", out, "--window", str(args.window), "--suite",
         args.suite], tree, args.child_timeout)


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
    ap.add_argument("--suite", choices=["sparse", "bn"], default="sparse")
    ap.add_argument("--child", choices=["check", "time"], default=None)
    ap.add_argument("--child-out", default=None)
    args = ap.parse_args()
    args.tree = os.path.abspath(args.tree)
    if args.child:
        return child(args)
    suite = SUITES[args.suite]
    trees = [("other", args.tree), ("this", HERE)]
    lines = ["%s, this tree against %s (\"other\")"
             % (suite["title"], args.label or args.tree)]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        saved = {}
        runs = trees + [("other again", args.tree)] * bool(suite.get("repeat"))
        for label, tree in runs:
            path = os.path.join(tmp, "check.pt")
            run_child("check", tree, path, args)
            saved[label] = torch.load(path)
            os.remove(path)
        a, b = saved["other"], saved["this"]
        again = saved.get("other again", a)
        assert a.keys() == b.keys() == again.keys()

        def differing(p, q):
            """Indices of the tensors (or checksum pairs) that differ."""
            assert len(p) == len(q)
            return [i for i, (x, y) in enumerate(zip(p, q)) if not torch.equal(
                *((x[1], y[1]) if isinstance(x, tuple) else (x, y)))]
        whole = sums = unstable = 0
        for k in a:
            if differing(a[k], again[k]):
                unstable += 1
                lines.append("NOT REPRODUCED by two runs of the other tree, "
                             "left out: %s (tensors %s; this tree against the "
                             "first run: %s)" % (k, differing(a[k], again[k]),
                                                 differing(a[k], b[k])))
                continue
            n = sum(isinstance(x, tuple) for x in a[k])
            sums += n
            whole += len(a[k]) - n
            for i in differing(a[k], b[k]):
                bad += 1
                lines.append("DIFFERENT: %s, tensor %d" % (k, i))
        lines.append("same bits: %d cases, %d more left out; %d tensors "
                     "compared whole with torch.equal, %d tensors above %d "
                     "MiB by their two int64 checksums; %d differ"
                     % (len(a) - unstable, unstable, whole, sums,
                        suite["big"] >> 20, bad))
        del saved, a, b
        times = {label: {} for label, _ in trees}
        for r in range(args.reps):          # the trees alternate
            for label, tree in trees:
                path = os.path.join(tmp, "time.json")
                run_child("time", tree, path, args)
                with open(path) as fh:
                    for k, v in json.load(fh).items():
                        times[label].setdefault(k, []).append(v)
        bench = {label: suite["bench"](
            args, os.path.join(tmp, "dump_" + label)) for label, _ in runs}
        outs = {label: run([sys.executable, "bench.py", "--gpus", "1"]
                           + bench[label], tree, args.child_timeout)
                for label, tree in runs}
        dumps = suite["dumps"](tmp) if "dumps" in suite else None
    lines += ["", "same speed: %s, %s; window >= "
              "%.2f s, %d alternating rounds of one process per tree"
              % (suite["speed"], torch.cuda.get_device_name(0), args.window,
                 args.reps),
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
    lines += ["", "bench.py --gpus 1 " + " ".join(
        "DIR" if a.startswith(tmp) else a for a in bench["this"])]
    for label, _ in runs:
        lines.append("%-11s %s" % (label,
                                   outs[label].strip().splitlines()[-1]))
    if dumps:
        lines.append(dumps[0])
        bad += dumps[1]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
