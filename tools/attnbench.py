#!/usr/bin/env python
"""Time ops.bag_attention, forward + backward, against what a user had to
write before it existed: pad the ragged bags and attend under a mask.

Workloads (H = 4 heads of D = 64; bag lengths drawn once, uniformly from
[8, 192], mean ~100; the drawn lengths are printed):

* self:   256 bags, every row is query and key of its bag;
* causal: the same with ``causal=True``;
* target: 2048 bags of keys, one query per bag (``offsets = arange(B+1)``).

Versions (each is one forward and one backward from a fixed dout, gradients
for q, k and v; the rows arrive packed [rows, H, D], as pulled):

* fused:    ``ops.bag_attention``;
* padded:   ``index_copy`` the packed rows into zeros [B, H, Lmax, D] (index
  built once, outside the timing), ``matmul`` in bf16, ``masked_fill``, fp32
  ``softmax``, ``matmul``, ``index_select`` the valid rows back, autograd's
  backward of all of it;
* sdpa:     the same padding around
  ``torch.nn.functional.scaled_dot_product_attention`` with a boolean mask
  (skipped with its error if this torch build cannot run it).

The fused forward is also timed alone (through the extension's binding).

Method (that of tools/sampledbench.py): device events; every version is
warmed up; each timing window lasts at least --window seconds; the versions
alternate inside one process (--reps rounds) and the median round is reported
with its min-max spread. The same inputs are reused by every call, so they
are cache-warm: these are not cold-HBM figures.

Peak memory is ``torch.cuda.max_memory_allocated`` over one forward+backward
above what was allocated before it.

    python tools/attnbench.py --out profiles/bag_attention_bench.txt
"""

import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tfmesos_amd import ops  # noqa: E402
from tools.sampledbench import peak_bytes, window  # noqa: E402


class Padding(object):
    """Pads packed rows to [B, Lmax] and back: an index_copy into zeros and
    an index_select, so that neither backward meets a duplicate index."""

    def __init__(self, lens, dev):
        self.B, self.L = lens.numel(), int(lens.max())
        pos = torch.arange(self.L)
        self.valid = (pos[None, :] < lens[:, None]).to(dev)          # [B,L]
        self.flat = self.valid.flatten().nonzero()[:, 0]    # packed -> padded

    def pad(self, x):                   # [rows,H,D] -> [B,H,L,D]
        xp = x.new_zeros((self.B * self.L,) + x.shape[1:])
        return xp.index_copy(0, self.flat, x).view(
            (self.B, self.L) + x.shape[1:]).transpose(1, 2)

    def unpad(self, xp):                # [B,H,L,D] -> [rows,H,D]
        return xp.transpose(1, 2).reshape(
            (self.B * self.L,) + xp.shape[1::2]).index_select(0, self.flat)


def padded(q, k, v, pq, pk, mask, scale, sdpa):
    qp, kp, vp = pq.pad(q), pk.pad(k), pk.pad(v)
    if sdpa:
        out = F.scaled_dot_product_attention(qp, kp, vp, attn_mask=mask,
                                             scale=scale)
    else:
        s = (qp @ kp.transpose(-1, -2)).float() * scale
        p = torch.softmax(s.masked_fill(~mask, float("-inf")), -1)
        out = p.to(q.dtype) @ vp
    return pq.unpad(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attnbench needs a GPU"
    dev = "cuda:0"
    ext = ops._ext()
    H, D = 4, 64
    scale = D ** -0.5

    lines = ["bag_attention fwd+bwd: bf16 rows, H = %d, D = %d, %s"
             % (H, D, torch.cuda.get_device_name(0)),
             "window >= %.2f s, %d alternating rounds, median reported; "
             "inputs reused by every call (cache-warm)"
             % (args.window, args.reps)]
    for name, B, causal, target in (("self", 256, False, False),
                                    ("causal", 256, True, False),
                                    ("target", 2048, False, True)):
        gen = torch.Generator().manual_seed(0)
        klens = torch.randint(8, 193, (B,), generator=gen)
        qlens = torch.ones_like(klens) if target else klens
        n, m = int(qlens.sum()), int(klens.sum())
        lines.append("%s: B = %d bags, key lengths uniform in [8, 192]: min %d"
                     ", mean %.1f, max %d; n = %d query rows, m = %d key rows"
                     % (name, B, klens.min(), klens.float().mean(),
                        klens.max(), n, m))
        off = lambda ls: torch.cat([ls.new_zeros(1), ls.cumsum(0)]).to(dev)  # noqa: E731
        qoff, koff = off(qlens), (None if not target else off(klens))
        pq, pk = Padding(qlens, dev), Padding(klens, dev)
        mask = (pq.valid[:, :, None] & pk.valid[:, None, :])[:, None]
        # a padded query row attends to key 0, so that no softmax row is empty
        mask = mask | (~pq.valid[:, None, :, None]
                       & (torch.arange(pk.L, device=dev) == 0))
        if causal:
            mask = mask & torch.ones(pq.L, pk.L, dtype=torch.bool,
                                     device=dev).tril()
        g = torch.Generator(device=dev).manual_seed(1)
        rows = lambda r: torch.randn(r, H, D, device=dev, generator=g).to(  # noqa: E731
            torch.bfloat16)
        q, k, v, dout = rows(n), rows(m), rows(m), rows(n)
        leaves = {ver: [t.clone().requires_grad_(True) for t in (q, k, v)]
                  for ver in ("fused", "padded", "sdpa")}

        def step(ver, fn):
            for t in leaves[ver]:
                t.grad = None
            out = fn(*leaves[ver])
            out.backward(dout)
            return out

        fused = lambda a, b, c: ops.bag_attention(a, b, c, qoff, koff, causal)  # noqa: E731
        vs = [("fused  (bag_attention)", lambda: step("fused", fused)),
              ("padded (matmul + softmax)", lambda: step(
                  "padded", lambda a, b, c: padded(a, b, c, pq, pk, mask,
                                                   scale, False))),
              ("sdpa   (padded + F.sdpa)", lambda: step(
                  "sdpa", lambda a, b, c: padded(a, b, c, pq, pk, mask,
                                                 scale, True))),
              ("fused forward alone", lambda: ext.bag_attention_fwd(
                  q, k, v, qoff, qoff if koff is None else koff, causal,
                  scale))]
        try:
            vs[2][1]()
            torch.cuda.synchronize()
        except Exception as e:      # this build has no kernel for it
            lines.append("%s: sdpa skipped: %s" % (name, str(e)[:200]))
            del vs[2]
        for _, fn in vs:                # warm every version
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
        for label, fn in vs:
            ts = sorted(times[label])
            med[label] = ts[len(ts) // 2]
            lines.append("%-8s %-28s %9.3f ms/call %6d iters  min-max "
                         "%.3f-%.3f ms  peak %.1f MiB" % (
                             name, label, med[label] * 1e3, iters[label],
                             ts[0] * 1e3, ts[-1] * 1e3,
                             peak_bytes(fn) / 2 ** 20))
        for label, _ in vs[1:-1]:
            lines.append("%-8s %s / fused = %.2fx" % (
                name, label.split()[0], med[label] / med[vs[0][0]]))
        lines.append("%-8s padded scores the fused path never allocates: "
                     "B H Lq Lk = %d x %d x %d x %d = %.1f Mi elements; fused "
                     "grid: %d forward blocks, %d + %d backward blocks a head"
                     % (name, B, H, pq.L, pk.L, B * H * pq.L * pk.L / 2 ** 20,
                        int(((qlens + 63) // 64).sum()),
                        int(((qlens + 63) // 64).sum()),
                        int(((klens + 63) // 64).sum())))
        a, b = vs[0][1]().detach().float(), vs[1][1]().detach().float()
        gf, gp = leaves["fused"], leaves["padded"]
        lines.append("%-8s fused vs padded: out max |diff| %.3g (magnitude "
                     "%.3g); dq %.3g (%.3g); dk %.3g (%.3g); dv %.3g (%.3g)"
                     % ((name, float((a - b).abs().max()),
                         float(a.abs().max())) + tuple(
                        f(x.grad.float(), y.grad.float())
                        for x, y in zip(gf, gp)
                        for f in (lambda s, t: float((s - t).abs().max()),
                                  lambda s, t: float(s.abs().max())))))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
