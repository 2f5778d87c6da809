#!/usr/bin/env python
"""Time ops.layer_norm, forward + backward, against what a user had to write
before it existed: ``torch.nn.functional.layer_norm`` next to a separate
residual add, autograd's backward of both.

Shapes [n, D]: 32768 x 64, 32768 x 128, 8192 x 512, 4096 x 1024, and 65536 x
1024 as a shape whose kernels outlast the host's work, each with and without
a residual. Rows are bf16 and weight and bias bf16 on both sides.

Versions (each is one forward and one backward from fixed gradients; with a
residual the gradients arrive through both y and the new stream s):

* fused: ``ops.layer_norm(x, w, b, residual=r)``;
* torch: ``s = x + r; y = F.layer_norm(s, (D,), w, b)``.

The fused forward and backward are also timed alone, without autograd
(``ops.layer_norm_fwd`` / ``ops.layer_norm_bwd``, rows "fwd" and "bwd"), each
against its own half of the useful bytes.

Useful bytes are computed from the shapes alone, the traffic the op cannot
avoid: the forward reads x (and r) and writes y (and s), mean and rstd; the
backward reads dy, s (and ds), mean and rstd and writes dx; both directions
touch the [D] parameters once. GB/s is those bytes over the measured time,
for both versions, so it is a rate of useful work, not of memory traffic.

Method: device events; every version is warmed up; the versions alternate
inside one process (--reps rounds) and the median round is reported with its
min-max spread. A window's call count is sized from 20 calls timed after 5
more warm-up calls (the first call after a switch of versions is several
times slower than the steady state), and the window is run again with more
calls until its event-timed length reaches --window seconds; the shortest
window of a row is printed and asserted. "host ms" is the host clock over the
same loop before the device is waited for: the time the host needs to enqueue
a call. Where it equals ms/call the host, not the device, sets the pace. The
same inputs are reused by every call, so they are cache-warm: these are not
cold-HBM figures.

    python tools/normbench.py --out profiles/layer_norm_bench.txt
"""

import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd import ops  # noqa: E402

SHAPES = ((32768, 64), (32768, 128), (8192, 512), (4096, 1024), (65536, 1024))


def useful_bytes(n, D, residual):
    """(forward, backward) bytes."""
    rows = 2 * n * D                    # one bf16 [n, D] tensor
    stats = 2 * 4 * n                   # mean and rstd, fp32
    fwd = (4 if residual else 2) * rows + stats + 2 * 2 * D
    bwd = (4 if residual else 3) * rows + stats + 3 * 2 * D
    return fwd, bwd


def timed(fn, iters):
    """(device seconds, host seconds to enqueue) of iters calls."""
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    host = time.perf_counter() - t0
    end.synchronize()
    return start.elapsed_time(end) * 1e-3, host


def window(fn, min_s):
    """(seconds a call, host seconds a call, calls, window seconds) over one
    window of at least min_s."""
    timed(fn, 5)
    iters = max(20, int(1.1 * min_s / (timed(fn, 20)[0] / 20)) + 1)
    while True:
        dev, host = timed(fn, iters)
        if dev >= min_s:
            return dev / iters, host / iters, iters, dev
        iters = int(iters * 1.5 * min_s / dev) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "normbench needs a GPU"
    dev = "cuda:0"
    ops._ext()

    lines = ["layer_norm fwd+bwd: bf16 rows, bf16 weight and bias, %s"
             % torch.cuda.get_device_name(0),
             "window >= %.2f s (shortest of a row printed), %d alternating "
             "rounds, median reported; inputs reused by every call "
             "(cache-warm)"
             % (args.window, args.reps),
             "%-13s %-9s %-6s %9s %9s %7s %9s  %-15s %8s" % (
                 "n x D", "residual", "ver", "ms/call", "host ms", "iters",
                 "window s", "min-max ms", "GB/s")]
    for n, D in SHAPES:
        for residual in (True, False):
            g = torch.Generator(device=dev).manual_seed(0)
            rows = lambda: torch.randn(n, D, device=dev, generator=g).to(  # noqa: E731
                torch.bfloat16)
            x, r, dy, ds = rows(), rows(), rows(), rows()
            w = (1 + 0.5 * torch.randn(D, device=dev, generator=g)).to(
                torch.bfloat16)
            b = torch.randn(D, device=dev, generator=g).to(torch.bfloat16)
            leaves = {ver: [t.clone().requires_grad_(True)
                            for t in (x, r, w, b)]
                      for ver in ("fused", "torch")}

            def fused(x, r, w, b):
                if residual:
                    return ops.layer_norm(x, w, b, residual=r)
                return (ops.layer_norm(x, w, b),)

            def composed(x, r, w, b):
                if residual:
                    s = x + r
                    return F.layer_norm(s, (D,), w, b), s
                return (F.layer_norm(x, (D,), w, b),)

            def step(ver, fn):
                for t in leaves[ver]:
                    t.grad = None
                outs = fn(*leaves[ver])
                torch.autograd.backward(outs, (dy, ds)[:len(outs)])
                return outs

            rr = r if residual else None
            saved = ops.layer_norm_fwd(x, w, b, 1e-5, rr, False)[1:]
            vs = [("fused", lambda: step("fused", fused)),
                  ("torch", lambda: step("torch", composed)),
                  ("fwd", lambda: ops.layer_norm_fwd(x, w, b, 1e-5, rr,
                                                     False)),
                  ("bwd", lambda: ops.layer_norm_bwd(
                      dy, *saved, w, False, ds if residual else None))]
            for _, fn in vs:            # warm every version
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            runs = {label: [] for label, _ in vs}
            for _ in range(args.reps):  # versions alternate in one process
                for label, fn in vs:
                    runs[label].append(window(fn, args.window))
            fb, bb = useful_bytes(n, D, residual)
            nbytes = {"fused": fb + bb, "torch": fb + bb, "fwd": fb, "bwd": bb}
            med = {}
            for label, _ in vs:
                rs = sorted(runs[label])
                sec, host, iters, _ = rs[len(rs) // 2]
                shortest = min(r[3] for r in rs)
                assert shortest >= args.window, (label, shortest)
                med[label] = sec
                lines.append(
                    "%-13s %-9s %-6s %9.4f %9.4f %7d %9.3f  %-15s %8.1f" % (
                        "%d x %d" % (n, D), "yes" if residual else "no", label,
                        sec * 1e3, host * 1e3, iters, shortest,
                        "%.4f-%.4f" % (rs[0][0] * 1e3, rs[-1][0] * 1e3),
                        nbytes[label] / sec / 1e9))
            a, c = vs[0][1](), vs[1][1]()
            gf, gt = leaves["fused"], leaves["torch"]
            diff = lambda s, t: float((s.float() - t.float()).abs().max())  # noqa: E731
            lines.append("%-13s %-9s torch / fused = %.2fx; %.1f MB useful; "
                         "max |diff| y %.3g, dx %.3g, dweight %.3g, dbias %.3g"
                         % ("%d x %d" % (n, D), "yes" if residual else "no",
                            med["torch"] / med["fused"], (fb + bb) / 1e6,
                            diff(a[0], c[0]), diff(gf[0].grad, gt[0].grad),
                            diff(gf[2].grad, gt[2].grad),
                            diff(gf[3].grad, gt[3].grad)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
