"""Compute ops: hand-written HIP/CDNA4 kernels with CPU torch reference.

Policy (per the MI355X-native design): on a GPU device these ops REQUIRE
the in-tree HIP extension ``tfmesos_amd._C`` (built from
``tfmesos_amd/ops/csrc/*.hip`` for gfx950) and raise if it is missing —
no silent PyTorch fallback on GPU. On CPU (tests, CI without GPUs) they
run a plain PyTorch fp32 reference implementation of the same op; the
numerics tests compare HIP kernel output against these references.

Op inventory mirrors what the reference delegated to TensorFlow's PS
runtime: fused optimizer apply (SGD/momentum, Adagrad,
Adam, FTRL-Proximal), bf16 GEMM with fused bias+ReLU epilogue, fused softmax
cross-entropy, embedding gather / scatter-add, fused sparse optimizer
apply for embedding rows (sparse_sgd / sparse_adagrad / sparse_adam /
sparse_ftrl — TF's SparseApply*: duplicates summed, one update per touched row), and
pooled (bag) lookups: embedding_bag forward (TF's embedding_lookup_sparse,
combiner sum / mean, optional weights) and the same sparse applies fed
bag gradients (``offsets=``); and the routing of requests to a row-sharded
table (TF's partitioned variable): shard_partition, permute_rows,
shard_bag_offsets, bag_coefficients; and the worker-side coalescing of a row
request (TF's unique / unsorted_segment_sum): coalesce_ids, segment_sum_rows;
and the key index of hashed embedding tables (TF's MutableHashTable):
HashIndex, hash_find, hash_find_or_insert, hash_rebuild, hash_gather,
hash_init_rows, hash_init_new_rows, and eviction from it: hash_touch (use
stamps), hash_compact (keep the flagged rows, dense again), hash_remove.
Feature admission: HashAdmission (a count-min sketch), hash_admit_cells,
hash_find_or_admit, and the serving ops that read an absent key's initial
row instead of storing it: hash_gather_init, hash_embedding_bag.
"""

import collections

import numpy as np
import torch

_EXT = None
_EXT_ERR = None


def _ext():
    global _EXT, _EXT_ERR
    if _EXT is None and _EXT_ERR is None:
        try:
            from tfmesos_amd import _C  # built in-tree by setup.py/__graft_entry__
            _EXT = _C
        except ImportError as e:
            _EXT_ERR = e
    if _EXT is None:
        raise RuntimeError(
            "tfmesos_amd HIP extension not built (%s). On a GPU box the "
            "native kernels are mandatory — run `python __graft_entry__.py "
            "build` or `python setup.py build_ext --inplace`." % _EXT_ERR)
    return _EXT


def ext_available():
    try:
        _ext()
        return True
    except RuntimeError:
        return False


# --------------------------------------------------------------- optimizers

@torch.no_grad()
def fused_sgd(param, grad, lr, momentum=0.0, weight_decay=0.0, momentum_buf=None,
              bf16_out=None, grad_scale=1.0, neg_decay=0.0):
    """In-place SGD(+momentum, +wd) on an fp32 master param.

    grad may be bf16 or fp32 and is multiplied by grad_scale (worker-mean
    for sync replicas). If bf16_out is given, also writes the updated
    param as bf16 (the broadcast copy) in the same pass. neg_decay folds
    a soft nonnegativity penalty (g += neg_decay * min(p, 0) — the NMF
    objective) into the same pass.
    """
    if param.is_cuda:
        _ext().fused_sgd(param, grad, momentum_buf if momentum_buf is not None
                         else torch.empty(0, device=param.device),
                         bf16_out if bf16_out is not None
                         else torch.empty(0, dtype=torch.bfloat16, device=param.device),
                         float(lr), float(momentum), float(weight_decay),
                         float(grad_scale), float(neg_decay))
        return
    g = grad.float() * grad_scale
    if neg_decay:
        g = g + neg_decay * torch.clamp(param, max=0.0)
    if weight_decay:
        g = g + weight_decay * param
    if momentum and momentum_buf is not None:
        momentum_buf.mul_(momentum).add_(g)
        g = momentum_buf
    param.add_(g, alpha=-lr)
    if bf16_out is not None:
        bf16_out.copy_(param.to(torch.bfloat16))


@torch.no_grad()
def fused_adam(param, grad, exp_avg, exp_avg_sq, step, lr, beta1=0.9,
               beta2=0.999, eps=1e-8, weight_decay=0.0, bf16_out=None,
               grad_scale=1.0):
    """In-place Adam on fp32 master param (bias-corrected, as
    tf.train.AdamOptimizer used by mnist_replica.py:147)."""
    if param.is_cuda:
        _ext().fused_adam(param, grad, exp_avg, exp_avg_sq,
                          bf16_out if bf16_out is not None
                          else torch.empty(0, dtype=torch.bfloat16, device=param.device),
                          int(step), float(lr), float(beta1), float(beta2),
                          float(eps), float(weight_decay), float(grad_scale))
        return
    g = grad.float() * grad_scale
    if weight_decay:
        g = g + weight_decay * param
    exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (exp_avg_sq / bc2).sqrt_().add_(eps)
    param.addcdiv_(exp_avg / bc1, denom, value=-lr)
    if bf16_out is not None:
        bf16_out.copy_(param.to(torch.bfloat16))


@torch.no_grad()
def fused_adagrad(param, grad, accum, lr, eps=1e-10, weight_decay=0.0,
                  bf16_out=None, grad_scale=1.0):
    if param.is_cuda:
        _ext().fused_adagrad(param, grad, accum,
                             bf16_out if bf16_out is not None
                             else torch.empty(0, dtype=torch.bfloat16, device=param.device),
                             float(lr), float(eps), float(weight_decay),
                             float(grad_scale))
        return
    g = grad.float() * grad_scale
    if weight_decay:
        g = g + weight_decay * param
    accum.addcmul_(g, g, value=1.0)
    param.addcdiv_(g, accum.sqrt().add_(eps), value=-lr)
    if bf16_out is not None:
        bf16_out.copy_(param.to(torch.bfloat16))


def _ftrl_check(lr, l1, l2, acc0):
    if not lr > 0 or not l1 >= 0 or not l2 >= 0 or not acc0 > 0:
        raise ValueError("ftrl_proximal needs lr > 0, l1 >= 0, l2 >= 0 and "
                         "initial_accumulator_value > 0, got lr=%r, l1=%r, "
                         "l2=%r, initial_accumulator_value=%r"
                         % (lr, l1, l2, acc0))


@torch.no_grad()
def fused_ftrl(param, grad, accum, linear, lr, l1=0.0, l2=0.0,
               initial_accumulator_value=0.1, bf16_out=None, grad_scale=1.0):
    """In-place FTRL-Proximal (TF's FtrlOptimizer, lr_power -0.5) on an fp32
    master param: per-coordinate adaptive steps, l1 gives weights that are
    exactly 0.0, l2 is the only regulariser (no weight decay, no l2
    shrinkage). Per element, all in fp32 in this order, constants rounded
    to fp32 first, sign(0) = 0::

        gv = grad * grad_scale
        if accum == 0 and linear == 0:      # never updated: seed linear
            linear = -(p * (sqrt(acc0)/lr + 2*l2) + sign(p)*l1)
        n_new = accum + gv*gv
        s_old = sqrt(accum + acc0);  s_new = sqrt(n_new + acc0)
        sigma = (s_new - s_old) / lr
        z     = linear + (gv - sigma*p)
        quad  = s_new/lr + 2*l2
        p     = (sign(z)*l1 - z)/quad  if |z| > l1  else +0.0
        accum = n_new;  linear = z

    accum holds the sum of squared gradients only: acc0 =
    initial_accumulator_value is added on read and never stored, so both
    state tensors START AS ZEROS. FTRL's weight is a pure function of its
    state; the seeding step makes the current weight of a never-updated
    element (a table's random initial row) the FTRL solution instead of
    throwing it away on the first touch, so this is not bit for bit TF's
    Ftrl and its name here is "ftrl_proximal". GPU: csrc/ftrl.h in
    csrc/apply.hip, shadow written in the same pass."""
    acc0 = initial_accumulator_value
    _ftrl_check(lr, l1, l2, acc0)
    if param.is_cuda:
        _ext().fused_ftrl(param, grad, accum, linear,
                          bf16_out if bf16_out is not None
                          else torch.empty(0, dtype=torch.bfloat16,
                                           device=param.device),
                          float(lr), float(l1), float(l2), float(acc0),
                          float(grad_scale))
        return
    # constants as full fp32 tensors: torch divides by a one-element operand
    # through its reciprocal, which is not the correctly rounded quotient
    def f32(x):
        return torch.full(param.shape, float(x), dtype=torch.float32)
    lr, l1, l2, acc0 = f32(lr), f32(l1), f32(l2), f32(acc0)
    two_l2 = 2 * l2
    gv = grad.float() * f32(grad_scale)
    seed = -(param * (acc0.sqrt() / lr + two_l2) + torch.sign(param) * l1)
    lin = torch.where((accum == 0) & (linear == 0), seed, linear)
    n_new = accum + gv * gv
    s_new = (n_new + acc0).sqrt()
    sigma = (s_new - (accum + acc0).sqrt()) / lr
    z = lin + (gv - sigma * param)
    quad = s_new / lr + two_l2
    param.copy_(torch.where(z.abs() > l1, (torch.sign(z) * l1 - z) / quad,
                            torch.zeros_like(z)))
    accum.copy_(n_new)
    linear.copy_(z)
    if bf16_out is not None:
        bf16_out.copy_(param.to(torch.bfloat16))


# --------------------------------------------------------------------- gemm

GEMM_ROUTES = {"auto": 0, "stripes": 1, "fwd1": 2}
# gemm_fwd1_kernel geometries kept for measurement (tile, "s": strided B)
GEMM_FWD1_VARIANTS = {None: -1, "16x16": 0, "16x32": 1, "32x16": 2,
                      "32x32": 3, "16x16s": 4, "16x32s": 5, "32x16s": 6,
                      "32x32s": 7}


def gemm_bias_act(a, b, bias=None, act="none", trans_a=False, trans_b=False,
                  out=None, aux=None, colsum_out=None, route="auto",
                  fwd1_variant=None):
    """C = act(op(A) @ op(B) + bias), bf16 in, fp32 accumulate.

    Output dtype: bf16 by default; pass ``out`` (bf16 or fp32) to write
    in place — backward GEMMs write fp32 straight into the flat gradient
    buffer, skipping a cast+copy. Fused epilogues (one kernel each):

    * ``act="relu_bwd"`` with ``aux``: mask the product by ``aux > 0``
      (the saved forward activation) — the dX GEMM absorbs relu_bwd.
    * ``colsum_out``: also write ``sum_k op(B)[k, n]`` (fp32 [N]) — the
      dW GEMM absorbs the bias gradient's column sum.

    GPU: hand-written MFMA kernel (csrc/gemm.hip) with split-K for deep
    skinny shapes. CPU: torch reference in fp32.

    ``route`` picks the kernels of a K-sliced plain forward (GPU only;
    the results are bit-identical): ``"auto"`` (one launch for outputs
    up to 128x128, unless TFA_GEMM_FWD1=0), ``"stripes"`` (always
    split-K stripes + reduce) or ``"fwd1"`` (always the one-launch
    kernel; raises unless the call is nn, act none/relu, without
    aux/colsum, and slices K 2..16 ways). ``fwd1_variant`` selects one
    of GEMM_FWD1_VARIANTS instead of the shipped geometry.
    """
    act_code = {"none": 0, "relu": 1, "relu_bwd": 2, "sub": 3}[act]
    route_code = GEMM_ROUTES[route]
    variant_code = GEMM_FWD1_VARIANTS[fwd1_variant]
    if a.is_cuda:
        empty = torch.empty(0, device=a.device)
        ebias = bias if bias is not None else empty
        eaux = aux if aux is not None else empty
        ecs = colsum_out if colsum_out is not None else empty
        if out is None:
            out = torch.empty(
                (a.shape[1] if trans_a else a.shape[0],
                 b.shape[0] if trans_b else b.shape[1]),
                device=a.device, dtype=a.dtype)
        if route_code or variant_code >= 0:
            return _ext().gemm_bias_act_route(
                a, b, ebias, act_code, bool(trans_a), bool(trans_b), out,
                eaux, ecs, route_code, variant_code)
        return _ext().gemm_bias_act_out(a, b, ebias, act_code,
                                        bool(trans_a), bool(trans_b), out,
                                        eaux, ecs)
    x = a.float().t() if trans_a else a.float()
    y = b.float().t() if trans_b else b.float()
    c = x @ y
    if bias is not None:
        c = c + bias.float()
    if act == "relu":
        c = torch.relu(c)
    elif act == "relu_bwd":
        c = c * (aux.float() > 0)
    elif act == "sub":
        c = c - aux.float()
    if colsum_out is not None:
        colsum_out.copy_(y.sum(0).to(colsum_out.dtype))
    if out is not None:
        out.copy_(c.to(out.dtype))
        return out
    return c.to(a.dtype)


@torch.no_grad()
def gemm_sgd(a, b, param, lr, shadow=None, grad_scale=1.0, neg_decay=0.0,
             trans_a=False, trans_b=False):
    """Fused GEMM -> SGD: p -= lr*(grad_scale*(op(A)@op(B)) +
    neg_decay*min(p,0)); optional bf16 shadow refresh. The gradient
    never materializes on GPU (the split-K reduce IS the apply)."""
    if a.is_cuda:
        e = torch.empty(0, dtype=torch.bfloat16, device=a.device)
        _ext().gemm_sgd(a, b, bool(trans_a), bool(trans_b),
                        param.view(-1), shadow.view(-1) if shadow is not None
                        else e, float(lr), float(grad_scale),
                        float(neg_decay))
        return
    x = a.float().t() if trans_a else a.float()
    y = b.float().t() if trans_b else b.float()
    g = (x @ y).reshape(param.shape)
    fused_sgd(param, g, lr, grad_scale=grad_scale, neg_decay=neg_decay,
              bf16_out=shadow)


@torch.no_grad()
def gemm_sgd_pair(spec1, spec2, lr, grad_scale=1.0, neg_decay=0.0):
    """Two fused GEMM->SGD updates with SIMULTANEOUS semantics: both
    gradient GEMMs read pre-update operands (their stripe phases run
    before either apply). spec: (a, b, param, shadow, trans_a,
    trans_b)."""
    (a1, b1, p1, s1, ta1, tb1) = spec1
    (a2, b2, p2, s2, ta2, tb2) = spec2
    if a1.is_cuda:
        e = torch.empty(0, dtype=torch.bfloat16, device=a1.device)
        _ext().gemm_sgd_pair(
            a1, b1, bool(ta1), bool(tb1), p1.view(-1),
            s1.view(-1) if s1 is not None else e,
            a2, b2, bool(ta2), bool(tb2), p2.view(-1),
            s2.view(-1) if s2 is not None else e,
            float(lr), float(grad_scale), float(neg_decay))
        return
    def grad(a, b, ta, tb, p):
        x = a.float().t() if ta else a.float()
        y = b.float().t() if tb else b.float()
        return (x @ y).reshape(p.shape)
    g1 = grad(a1, b1, ta1, tb1, p1)
    g2 = grad(a2, b2, ta2, tb2, p2)
    fused_sgd(p1, g1, lr, grad_scale=grad_scale, neg_decay=neg_decay,
              bf16_out=s1)
    fused_sgd(p2, g2, lr, grad_scale=grad_scale, neg_decay=neg_decay,
              bf16_out=s2)


class _FanOutFn(torch.autograd.Function):
    """Explicit fan-out of a tensor to n consumers: backward sums the
    n incoming gradients with ONE n-way add kernel instead of
    autograd's (n-1) pairwise adds (35 of them per Inception step)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n = n
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *dys):
        ds = [d for d in dys if d is not None]
        if not ds:
            return None, None
        if len(ds) == 1:
            return ds[0], None
        if ds[0].is_cuda and ds[0].dtype == torch.bfloat16:
            cl = [d.contiguous(memory_format=torch.channels_last)
                  if d.dim() == 4 else d.contiguous() for d in ds]
            return _ext().add_n(cl), None
        out = ds[0].clone()
        for d in ds[1:]:
            out += d
        return out, None


def fan_out(x, n):
    """Returns n differentiable aliases of x (see _FanOutFn)."""
    return _FanOutFn.apply(x, n)


def colsum(x, out=None):
    """out[n] = sum_m x[m,n] in fp32 (bias gradients)."""
    if x.is_cuda:
        return _ext().colsum(x, out if out is not None else
                             torch.empty(0, dtype=torch.float32,
                                         device=x.device))
    s = x.float().sum(0)
    if out is not None:
        out.copy_(s)
        return out
    return s


# ------------------------------------------------------------- softmax-xent

def softmax_xent_fwd(logits, labels):
    """Returns (mean_loss fp32 scalar, probs bf16 [B,C]).

    Fused rowwise softmax + cross-entropy (the reference workload's loss,
    mnist_replica.py:143-145).
    """
    if logits.is_cuda:
        return _ext().softmax_xent_fwd(logits, labels)
    lg = logits.float()
    probs = torch.softmax(lg, dim=1)
    loss = torch.nn.functional.nll_loss(torch.log_softmax(lg, 1), labels)
    return loss, probs.to(logits.dtype)


def softmax_xent_fused(logits, labels, scale=None):
    """Returns (mean_loss fp32 scalar, dlogits bf16 [B,C]) in one fused
    kernel (fwd softmax + loss + bwd (p - onehot)*scale); scale defaults
    to 1/B. The mnist step's loss path is this single launch."""
    B = logits.shape[0]
    s = float(scale if scale is not None else 1.0 / B)
    if logits.is_cuda:
        return _ext().softmax_xent_fused(logits, labels, s)
    lg = logits.float()
    probs = torch.softmax(lg, dim=1)
    loss = torch.nn.functional.nll_loss(torch.log_softmax(lg, 1), labels)
    d = probs.clone()
    d[torch.arange(B), labels] -= 1.0
    return loss, (d * s).to(logits.dtype)


def softmax_xent_bwd(probs, labels, scale=None):
    """dlogits = (probs - onehot) * scale (scale defaults to 1/B)."""
    if probs.is_cuda:
        return _ext().softmax_xent_bwd(
            probs, labels, float(scale if scale is not None else 1.0 / probs.shape[0]))
    B = probs.shape[0]
    s = scale if scale is not None else 1.0 / B
    d = probs.float()
    d[torch.arange(B), labels] -= 1.0
    return (d * s).to(probs.dtype)


# ---------------------------------------------------------------- embedding

def embedding_gather(table, ids):
    """rows = table[ids]; table [V,D] (bf16 or fp32), ids int64 [N]."""
    if table.is_cuda:
        return _ext().embedding_gather(table, ids)
    return table.index_select(0, ids)


def embedding_scatter_add(table, ids, rows):
    """table[ids] += rows (duplicate ids accumulate)."""
    if table.is_cuda:
        _ext().embedding_scatter_add(table, ids, rows)
        return
    table.index_add_(0, ids, rows.to(table.dtype))


# ------------------------------------------------------ pooled (bag) lookup
#
# A bagged request is CSR-shaped: ids int64 [n], offsets int64 [B+1]
# (nondecreasing, offsets[0] == 0, offsets[B] == n; bag b is positions
# [offsets[b], offsets[b+1])), optional weights fp32 [n] (default 1).
# W_b = sum of w_i over ALL positions of bag b; the coefficient of position
# i is c_i = w_i (sum) or w_i / W_b (mean), 0 when W_b == 0. Ids outside
# [0, V) contribute nothing but still count in W_b. offsets is a caller
# contract: the CPU path validates it (ValueError); the GPU path does not
# (no device->host sync) — its kernels clamp every position they derive
# from it, so a violating input stays in bounds with an unspecified result.

def _bag_check(ids, offsets, weights, combiner):
    if combiner not in ("sum", "mean"):
        raise ValueError("unknown combiner %r (have 'sum', 'mean')"
                         % (combiner,))
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("offsets must be int64 [B+1]")
    if weights is not None and tuple(weights.shape) != (ids.numel(),):
        raise ValueError("weights must be [n] = [%d], got %s"
                         % (ids.numel(), tuple(weights.shape)))


def _bag_expand_cpu(ids, offsets, weights, combiner):
    """CPU reference of the expansion: validates offsets, returns the
    per-position bag row ``bag_of`` and coefficient ``c`` (fp32)."""
    n, B = ids.numel(), offsets.numel() - 1
    lens = offsets[1:] - offsets[:-1]
    if int(offsets[0]) != 0 or int(offsets[-1]) != n or bool((lens < 0).any()):
        raise ValueError("offsets must be nondecreasing with offsets[0] == 0 "
                         "and offsets[-1] == n = %d" % n)
    bag_of = torch.repeat_interleave(torch.arange(B), lens)
    c = weights.float() if weights is not None else torch.ones(n)
    if combiner == "mean":
        W = torch.zeros(B).index_add_(0, bag_of, c)[bag_of]
        c = torch.where(W == 0, torch.zeros(n), c / W)
    return bag_of, c


def _bag_weights(weights, dev):
    if weights is None:
        return torch.empty(0, device=dev)
    return weights.to(torch.float32).contiguous()


@torch.no_grad()
def embedding_bag(table, ids, offsets, weights=None, combiner="sum",
                  out_dtype=None):
    """out[b] = sum_i c_i * table[ids[i]] over bag b: fp32 accumulation in
    position order, rounded once to out_dtype; an empty bag gives a zero
    row. table [V,D] bf16 or fp32; out_dtype defaults to the table's,
    torch.float32 is allowed for a bf16 table (long bags lose bits in
    bf16). GPU: csrc/embedding_bag.hip, no atomics, no host sync."""
    _bag_check(ids, offsets, weights, combiner)
    if table.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("embedding_bag: table must be bf16 or fp32")
    out_dtype = table.dtype if out_dtype is None else out_dtype
    if out_dtype not in (table.dtype, torch.float32):
        raise ValueError("embedding_bag: out_dtype must be the table's dtype "
                         "or torch.float32")
    if table.is_cuda:
        return _ext().embedding_bag(
            table, ids.contiguous(), offsets.contiguous(),
            _bag_weights(weights, table.device), combiner == "mean",
            out_dtype == torch.float32)
    bag_of, c = _bag_expand_cpu(ids, offsets, weights, combiner)
    keep = (ids >= 0) & (ids < table.shape[0])
    rows = table.index_select(0, ids[keep]).float()
    out = torch.zeros(offsets.numel() - 1, table.shape[1])
    out.index_add_(0, bag_of[keep], c[keep, None] * rows)
    return out.to(out_dtype)


# ----------------------------------------------- row-sharded table routing
#
# A table of V rows split by row over S shards (TF's partitioned variable,
# partition_strategy "mod" or "div"):
#   mod: shard = id % S, local = id // S;
#   div: q, x = divmod(V, S); the first x shards hold q+1 rows, the rest q;
#        shard = max(id // (q+1), (id - x) // q), local = id - start(shard).
# An id outside [0, V) goes to shard 0 with local = -1: out of range on
# every shard, so it behaves as on an unsharded table. GPU: csrc/
# partition.hip — no atomics, bit-reproducible, nothing read back.

ShardPartition = collections.namedtuple(
    "ShardPartition", ["local", "perm", "inv", "starts"])
ShardPartition.__doc__ = """Stable partition of a request's ids by shard.

local [n]: shard-local ids grouped by shard, original order inside a shard;
perm [n]: the original position held by each slot; inv [n]: the slot of
each original position; starts [S+1]: shard s owns slots
[starts[s], starts[s+1])."""

_STRATEGIES = ("mod", "div")


def _shard_check(rows, num_shards, strategy):
    if strategy not in _STRATEGIES:
        raise ValueError("unknown partition strategy %r (have %s)"
                         % (strategy, list(_STRATEGIES)))
    if not 1 <= num_shards <= 64:
        raise ValueError("num_shards must be in [1, 64], got %r"
                         % (num_shards,))
    if rows < num_shards:
        raise ValueError("a table of %d rows cannot be split over %d shards"
                         % (rows, num_shards))


def shard_rows(rows, num_shards, shard, strategy="mod"):
    """Row count of shard ``shard`` of a ``rows``-row table."""
    return len(shard_global_ids(rows, num_shards, shard, strategy))


def shard_global_ids(rows, num_shards, shard, strategy="mod"):
    """The global ids shard ``shard`` holds, in local order (a range)."""
    _shard_check(rows, num_shards, strategy)
    if not 0 <= shard < num_shards:
        raise ValueError("shard must be in [0, %d), got %r"
                         % (num_shards, shard))
    if strategy == "mod":
        return range(shard, rows, num_shards)
    q, x = divmod(rows, num_shards)
    start = shard * q + min(shard, x)
    return range(start, start + q + (1 if shard < x else 0))


def _route_cpu(ids, rows, num_shards, strategy):
    """(shard, local) per id, by the rule above."""
    valid = (ids >= 0) & (ids < rows)
    safe = torch.where(valid, ids, torch.zeros_like(ids))
    if strategy == "mod":
        shard = safe % num_shards
        local = torch.div(safe, num_shards, rounding_mode="floor")
    else:
        q, x = divmod(rows, num_shards)
        shard = torch.maximum(
            torch.div(safe, q + 1, rounding_mode="floor"),
            torch.div(safe - x, q, rounding_mode="floor"))
        local = safe - (shard * q + torch.clamp(shard, max=x))
    return (torch.where(valid, shard, torch.zeros_like(ids)),
            torch.where(valid, local, torch.full_like(ids, -1)))


@torch.no_grad()
def shard_partition(ids, rows, num_shards, strategy="mod"):
    """Stable partition of ids int64 [n] (n < 2**31) by owning shard ->
    ShardPartition. GPU: count / scan / scatter (csrc/partition.hip; the
    scan is torch.cumsum), no host sync. CPU: a stable sort of the shard
    numbers."""
    _shard_check(rows, num_shards, strategy)
    if ids.dim() != 1 or ids.dtype != torch.int64:
        raise ValueError("ids must be int64 [n]")
    if ids.numel() >= 2 ** 31:
        raise ValueError("shard_partition: n must be below 2**31")
    if ids.is_cuda:
        return ShardPartition(*_ext().shard_partition(
            ids.contiguous(), int(rows), int(num_shards), strategy == "div"))
    shard, local = _route_cpu(ids, rows, num_shards, strategy)
    perm = torch.sort(shard, stable=True)[1]
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(ids.numel())
    starts = torch.zeros(num_shards + 1, dtype=torch.int64)
    starts[1:] = torch.bincount(shard, minlength=num_shards).cumsum(0)
    return ShardPartition(local[perm], perm, inv, starts)


@torch.no_grad()
def permute_rows(rows, perm, out_dtype=None):
    """out[j] = rows[perm[j]] cast to out_dtype (default: rows' dtype);
    rows [n,D] fp32 or bf16, out fp32 or bf16: a push's gradient rows laid
    out in wire order and wire dtype in one pass."""
    out_dtype = rows.dtype if out_dtype is None else out_dtype
    ok = (torch.float32, torch.bfloat16)
    if rows.dim() != 2 or rows.dtype not in ok or out_dtype not in ok:
        raise ValueError("permute_rows: rows must be [n,D] fp32 or bf16 and "
                         "out_dtype fp32 or bf16")
    if rows.is_cuda:
        return _ext().permute_rows(rows.contiguous(), perm.contiguous(),
                                   out_dtype == torch.bfloat16)
    return rows.index_select(0, perm).to(out_dtype)


@torch.no_grad()
def shard_bag_offsets(perm, starts, offsets):
    """shard_offsets int64 [S, B+1] of a bagged request (offsets [B+1])
    after shard_partition: the stable partition keeps each bag contiguous
    inside each shard, and shard_offsets[s][b] is the number of shard s's
    slots whose original position lies before offsets[b]."""
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("offsets must be int64 [B+1]")
    if perm.is_cuda:
        return _ext().shard_bag_offsets(perm.contiguous(),
                                        starts.contiguous(),
                                        offsets.contiguous())
    S = starts.numel() - 1
    out = torch.empty(S, offsets.numel(), dtype=torch.int64)
    off = offsets.clamp(0, perm.numel())
    for s in range(S):
        seg = perm[int(starts[s]):int(starts[s + 1])]
        out[s] = torch.searchsorted(seg, off)
    return out


@torch.no_grad()
def bag_coefficients(n, offsets, weights=None, combiner="sum"):
    """c fp32 [n]: the coefficient of every position of a bagged request
    (rule above: w_i, or w_i / W_b for mean, 0 when W_b == 0), 0 for a
    position no bag covers. On the GPU the bits equal what embedding_bag
    and the pooled sparse applies compute internally (csrc/bag.h), so
    passing c as ``weights`` with combiner "sum" reproduces a "mean"
    call bit for bit."""
    if combiner not in ("sum", "mean"):
        raise ValueError("unknown combiner %r (have 'sum', 'mean')"
                         % (combiner,))
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("offsets must be int64 [B+1]")
    if weights is not None and tuple(weights.shape) != (n,):
        raise ValueError("weights must be [n] = [%d], got %s"
                         % (n, tuple(weights.shape)))
    if offsets.is_cuda:
        return _ext().bag_coefficients(
            int(n), offsets.contiguous(),
            _bag_weights(weights, offsets.device), combiner == "mean")
    return _bag_expand_cpu(torch.empty(n), offsets, weights, combiner)[1]


# ------------------------------------------------ coalescing a row request
#
# What TF's PS does before a row request reaches the wire: embedding_lookup
# gathers each DISTINCT id once (unique), and a sparse gradient has its
# duplicate indices summed (unsorted_segment_sum). coalesce_ids finds the
# distinct ids of a request, segment_sum_rows sums the gradient rows per
# distinct id in fp32 and rounds once. GPU: csrc/coalesce.hip — no atomics,
# bit-reproducible, nothing read back.

Coalesced = collections.namedtuple(
    "Coalesced", ["uniq", "inverse", "perm", "seg", "count"])
Coalesced.__doc__ = """The distinct ids of a request's ids [n], all int64 on
the ids' device. With u distinct ids:

uniq [n]: the distinct ids ascending in uniq[:u], -1 behind them;
inverse [n]: uniq[inverse[i]] == ids[i]; perm [n]: the permutation of the
stable sort of ids (positions grouped by id, request order inside a group);
seg [n+1]: seg[k] is the first sorted position of distinct id k for k < u
and n for k >= u; count [1]: u."""


@torch.no_grad()
def coalesce_ids(ids):
    """The distinct ids of ids int64 [n] (n < 2**31) -> Coalesced. The ids'
    range does not matter: negative and too-large ids are distinct values
    like any other. GPU: stable torch.sort, then head flags / count / scan
    / scatter (csrc/coalesce.hip; the scan is torch.cumsum), no host sync.
    CPU: torch.unique and a stable sort."""
    if ids.dim() != 1 or ids.dtype != torch.int64:
        raise ValueError("ids must be int64 [n]")
    n = ids.numel()
    if n >= 2 ** 31:
        raise ValueError("coalesce_ids: n must be below 2**31")
    if ids.is_cuda:
        return Coalesced(*_ext().coalesce_ids(ids.contiguous()))
    u, inverse = torch.unique(ids, sorted=True, return_inverse=True)
    perm = torch.sort(ids, stable=True)[1]
    uniq = torch.full((n,), -1, dtype=torch.int64)
    uniq[:u.numel()] = u
    seg = torch.full((n + 1,), n, dtype=torch.int64)
    lens = torch.bincount(inverse, minlength=u.numel())
    seg[:u.numel()] = lens.cumsum(0) - lens
    return Coalesced(uniq, inverse, perm, seg, torch.tensor([u.numel()]))


@torch.no_grad()
def segment_sum_rows(rows, perm, seg, num, out_dtype=None):
    """out [num,D]: out[k] = sum of rows[perm[j]] over j in
    [seg[k], seg[k+1]) — fp32 accumulation in that order, rounded ONCE to
    out_dtype (default: rows' dtype). rows [n,D] fp32 or bf16, out fp32 or
    bf16; perm / seg as coalesce_ids returns them, num (a host int) <= the
    number of distinct ids. GPU: one wave per output row, runs longer than
    512 cut into pieces summed by separate waves (csrc/coalesce.hip)."""
    out_dtype = rows.dtype if out_dtype is None else out_dtype
    ok = (torch.float32, torch.bfloat16)
    if rows.dim() != 2 or rows.dtype not in ok or out_dtype not in ok:
        raise ValueError("segment_sum_rows: rows must be [n,D] fp32 or bf16 "
                         "and out_dtype fp32 or bf16")
    n = rows.shape[0]
    if perm.dim() != 1 or perm.numel() != n:
        raise ValueError("segment_sum_rows: need one perm entry per row: "
                         "%d rows, perm %s" % (n, tuple(perm.shape)))
    num = int(num)
    if num < 0 or seg.dim() != 1 or seg.numel() < num + 1:
        raise ValueError("segment_sum_rows: seg must hold num + 1 = %d "
                         "entries, got %s" % (num + 1, tuple(seg.shape)))
    if rows.is_cuda:
        return _ext().segment_sum_rows(rows.contiguous(), perm.contiguous(),
                                       seg.contiguous(), num,
                                       out_dtype == torch.bfloat16)
    # the segment of every sorted position: the ends seg[1:num+1] at or
    # before it; positions behind seg[num] belong to no output row
    of = torch.bucketize(torch.arange(n), seg[1:num + 1], right=True)
    keep = of < num
    out = torch.zeros(num, rows.shape[1])
    out.index_add_(0, of[keep], rows.float().index_select(0, perm[keep]))
    return out.to(out_dtype)


# ------------------------------------------------- hashed embedding tables
#
# An index from arbitrary int64 keys to the dense rows 0 .. size-1 of a
# table of fixed capacity (TF's MutableHashTable / dynamic embedding
# variable): the features of CTR and recommender models are 64-bit hashes or
# raw categorical ids of an open vocabulary, not row numbers. Every int64
# value is a key except HASH_EMPTY (INT64_MIN), which is treated as absent
# and never inserted. Rows are handed out in allocation order; row_keys[r]
# is the key that owns row r. GPU: csrc/hash.hip — an open-addressing slot
# array (load <= 0.5), integer atomics only, identical results from run to
# run, nothing read back. CPU (the reference): a Python dict.

HASH_EMPTY = -2 ** 63
HASH_KEY_SPACE = 2 ** 62    # ``rows=`` of a row-sharded hashed table
_HASH_GOLD = 0x9E3779B97F4A7C15
_U64 = 2 ** 64


def _mix64(z):
    """The splitmix64 finaliser on a numpy uint64 ARRAY (array arithmetic
    wraps silently; numpy scalars would warn)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _u64_array(keys):
    return keys.detach().cpu().contiguous().numpy().view(np.uint64)


def _hash_keys_check(keys):
    if keys.dim() != 1 or keys.dtype != torch.int64:
        raise ValueError("keys must be int64 [n]")
    if keys.numel() >= 2 ** 31:
        raise ValueError("hash index: n must be below 2**31")


def hash_slots(capacity):
    """Slots H of an index of ``capacity`` rows: the smallest power of two
    that is at least 2 * capacity and at least 64 (one wave's probe)."""
    H = 64
    while H < 2 * capacity:
        H *= 2
    return H


def hash_home(keys, slots):
    """The home slot of every key in an array of ``slots`` slots (a power of
    two): splitmix64-finaliser(key as uint64) & (slots - 1). int64 [n] on
    the CPU. An internal detail of the index — exposed so that a test can
    build long probe chains; no result of any op depends on it."""
    _hash_keys_check(keys)
    if slots < 1 or slots & (slots - 1):
        raise ValueError("slots must be a power of two, got %r" % (slots,))
    h = _mix64(_u64_array(keys)) & np.uint64(slots - 1)
    return torch.from_numpy(h.astype(np.int64))


class HashIndex(object):
    """Key index of a hashed table with ``capacity`` rows on ``device``.

    row_keys int64 [capacity] (HASH_EMPTY behind ``size``), size, dropped and
    evicted (rows removed by ``hash_compact``) int64 [1] on the device
    (reading them is the caller's sync), and on a GPU the slot arrays slot_keys / slot_rows int64 [hash_slots(capacity)].
    On the CPU the reference keeps a dict instead of slot arrays."""

    def __init__(self, capacity, device="cpu"):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("capacity must be >= 1, got %d" % capacity)
        self.device = torch.device(device)
        self.capacity = capacity
        self.row_keys = torch.full((capacity,), HASH_EMPTY,
                                   dtype=torch.int64, device=self.device)
        self.size = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.dropped = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.evicted = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._alloc_slots()

    def _alloc_slots(self):
        self._map = {}
        self.slot_keys = self.slot_rows = None
        if self.device.type != "cpu":
            H = hash_slots(self.capacity)
            self.slot_keys = torch.full((H,), HASH_EMPTY, dtype=torch.int64,
                                        device=self.device)
            self.slot_rows = torch.full((H,), -1, dtype=torch.int64,
                                        device=self.device)

    def reserve(self, capacity):
        """Grow to ``capacity`` rows: larger row_keys and slot arrays, then
        a rebuild. The key -> row mapping is unchanged; no host sync."""
        capacity = int(capacity)
        if capacity < self.capacity:
            raise ValueError("reserve(%d): the index already has capacity %d "
                             "(shrinking is not supported)"
                             % (capacity, self.capacity))
        if capacity == self.capacity:
            return
        row_keys = torch.full((capacity,), HASH_EMPTY, dtype=torch.int64,
                              device=self.device)
        row_keys[:self.capacity] = self.row_keys
        self.row_keys = row_keys
        self.capacity = capacity
        self._alloc_slots()
        hash_rebuild(self)

    def assign(self, keys):
        """Make ``keys`` (distinct, none HASH_EMPTY, at most capacity) the
        owners of rows 0 .. len(keys)-1 (checkpoint load)."""
        _hash_keys_check(keys)
        n = keys.numel()
        if n > self.capacity:
            raise ValueError("%d keys do not fit capacity %d"
                             % (n, self.capacity))
        self.row_keys.fill_(HASH_EMPTY)
        self.row_keys[:n] = keys.to(self.device)
        self.size.fill_(n)
        self.dropped.zero_()
        self.evicted.zero_()
        hash_rebuild(self)


def _hash_index_check(index, keys):
    _hash_keys_check(keys)
    if keys.device.type != index.device.type:
        raise ValueError("keys are on %s, the index on %s"
                         % (keys.device, index.device))


@torch.no_grad()
def hash_find(index, keys):
    """rows int64 [n]: the row of keys[i], -1 when the key is absent (or
    HASH_EMPTY). Read-only."""
    _hash_index_check(index, keys)
    if keys.is_cuda:
        return _ext().hash_find(index.slot_keys, index.slot_rows,
                                keys.contiguous())
    get = index._map.get
    return torch.tensor([get(k, -1) for k in keys.tolist()],
                        dtype=torch.int64)


@torch.no_grad()
def hash_find_or_insert(index, keys):
    """(rows int64 [n], is_new bool [n]). Like hash_find, but an absent key
    gets the next free row: the new keys of one request receive rows size,
    size + 1, ... in the order of their FIRST occurrence in the request and
    every duplicate gets that row; is_new marks the one position (the first
    occurrence) that allocated it. A key that would need a row >= capacity
    gets -1 and ``dropped`` grows by the number of DISTINCT such keys of the
    request; it gets a row on a later request once there is room
    (``reserve``). HASH_EMPTY gives -1 and is not counted. Deterministic:
    the GPU (csrc/hash.hip) equals this dict loop integer for integer."""
    _hash_index_check(index, keys)
    if keys.is_cuda:
        rows, is_new = _ext().hash_find_or_insert(
            index.slot_keys, index.slot_rows, index.row_keys, index.size,
            index.dropped, keys.contiguous())
        return rows, is_new
    m, cap = index._map, index.capacity
    size = int(index.size)
    rows, fresh, lost = [], [], set()
    for k in keys.tolist():
        r = -1 if k == HASH_EMPTY else m.get(k)
        if r is None:
            if size < cap:
                r = m[k] = size
                index.row_keys[r] = k
                size += 1
                fresh.append(len(rows))
            else:
                r = -1
                lost.add(k)
        rows.append(r)
    index.size.fill_(size)
    index.dropped += len(lost)
    is_new = torch.zeros(len(rows), dtype=torch.bool)
    is_new[fresh] = True
    return torch.tensor(rows, dtype=torch.int64), is_new


# Feature admission. Most keys of a hashed categorical feature are seen once
# or twice and never again; a key earns a row only after it has been named
# by ``admit_after`` push requests. The counts live in a count-min sketch:
# 4 rows of ``width`` int32 counters, key k counts in cell
# mix64(uint64(k) + (j + 1) * G) & (width - 1) of sketch row j (wrapping
# uint64; mix64 and G as in hash_init_rows), its estimate is the minimum of
# its four cells. Count-min never underestimates: a key is admitted no later
# than its admit_after-th request, possibly earlier through collisions.

HASH_ADMIT_ROWS = 4
HASH_ADMIT_CAP = 2 ** 30    # counters saturate here


def _admit_width_check(width):
    if width < 64 or width & (width - 1):
        raise ValueError("admission sketch: width must be a power of two "
                         ">= 64, got %r" % (width,))


def hash_admit_cells(keys, width):
    """The sketch cells of every key: int64 [4, n] on the CPU, row j the
    cells in sketch row j. Like ``hash_home`` an internal detail, exposed so
    that a test can build collisions."""
    _hash_keys_check(keys)
    _admit_width_check(width)
    k = _u64_array(keys)
    cells = [_mix64(k + np.array([(j + 1) * _HASH_GOLD % _U64],
                                 dtype=np.uint64)) & np.uint64(width - 1)
             for j in range(HASH_ADMIT_ROWS)]
    return torch.from_numpy(np.stack(cells).astype(np.int64))


class HashAdmission(object):
    """Count-min sketch of an admission policy: ``counters`` int32
    [4, width] and ``filtered`` int64 [1] (distinct keys of a request that
    were counted but not admitted, summed over the requests) on ``device``;
    reading either is the caller's sync."""

    def __init__(self, width, device="cpu"):
        width = int(width)
        _admit_width_check(width)
        self.width = width
        self.device = torch.device(device)
        self.counters = torch.zeros(HASH_ADMIT_ROWS, width, dtype=torch.int32,
                                    device=self.device)
        self.filtered = torch.zeros(1, dtype=torch.int64, device=self.device)

    def decay(self):
        """Halve every counter (ageing; plumbing, one torch op)."""
        self.counters.bitwise_right_shift_(1)


@torch.no_grad()
def hash_find_or_admit(index, sketch, keys, admit_after):
    """(rows int64 [n], is_new bool [n]): ``hash_find_or_insert`` behind the
    admission sketch. A key that has a row behaves as there. Each DISTINCT
    absent key of the request (HASH_EMPTY excluded) is counted once — its
    four cells get +1, saturating: min(old + adds, 2**30) — whatever the
    number of its occurrences, so coalescing a request does not change
    which request admits a key. With all counts of the request in, an
    absent key whose estimate (the minimum of its four cells) is >=
    ``admit_after`` (in [1, 2**30]) is admitted: it is a new key of
    ``hash_find_or_insert`` (rows in first-occurrence order among the
    admitted keys, is_new at the first occurrence, -1 and ``dropped`` when
    no room is left). Every other absent key gets -1 and
    ``sketch.filtered`` grows by their number. Deterministic: the GPU
    (csrc/hash.hip; integer atomics, decisions read in a later kernel)
    equals this reference integer for integer, counters included."""
    _hash_index_check(index, keys)
    admit_after = int(admit_after)
    if not 1 <= admit_after <= HASH_ADMIT_CAP:
        raise ValueError("admit_after must lie in [1, 2**30], got %r"
                         % (admit_after,))
    if not isinstance(sketch, HashAdmission) or \
            sketch.device != index.device:
        raise ValueError("hash_find_or_admit: need a HashAdmission on the "
                         "index's device")
    if keys.is_cuda:
        rows, is_new = _ext().hash_find_or_admit(
            index.slot_keys, index.slot_rows, index.row_keys, index.size,
            index.dropped, sketch.counters, sketch.filtered,
            keys.contiguous(), admit_after)
        return rows, is_new
    m, cap = index._map, index.capacity
    klist = keys.tolist()
    first = {}                  # distinct absent keys -> first position
    for i, k in enumerate(klist):
        if k != HASH_EMPTY and k not in m and k not in first:
            first[k] = i
    is_new = torch.zeros(len(klist), dtype=torch.bool)
    if first:
        cand = torch.tensor(list(first), dtype=torch.int64)
        cells = hash_admit_cells(cand, sketch.width).numpy()
        counts = sketch.counters.numpy().astype(np.int64)
        for j in range(HASH_ADMIT_ROWS):
            np.add.at(counts[j], cells[j], 1)
        np.minimum(counts, HASH_ADMIT_CAP, out=counts)
        sketch.counters.copy_(torch.from_numpy(counts.astype(np.int32)))
        est = np.stack([counts[j][cells[j]]
                        for j in range(HASH_ADMIT_ROWS)]).min(axis=0)
        admitted = est >= admit_after
        sketch.filtered += int((~admitted).sum())
        size, lost = int(index.size), 0
        for k, ok in zip(first, admitted.tolist()):
            if not ok:
                continue
            if size < cap:
                m[k] = size
                index.row_keys[size] = k
                is_new[first[k]] = True
                size += 1
            else:
                lost += 1
        index.size.fill_(size)
        index.dropped += lost
    rows = torch.tensor([-1 if k == HASH_EMPTY else m.get(k, -1)
                         for k in klist], dtype=torch.int64)
    return rows, is_new


@torch.no_grad()
def hash_rebuild(index):
    """Rebuild the key -> row mapping from row_keys[0:size] (after
    ``reserve`` or a checkpoint load). GPU: clears the slot arrays and
    inserts the keys with their known rows, no host sync."""
    if index.device.type != "cpu":
        _ext().hash_rebuild(index.slot_keys, index.slot_rows, index.row_keys,
                            index.size)
        return
    n = int(index.size)
    index._map = {k: r for r, k in enumerate(index.row_keys[:n].tolist())}


# Eviction. The GPU index has no deletion (a key sits before the first empty
# slot of its probe sequence), so keys leave by COMPACTION: the caller says
# which rows stay, the survivors are made dense again in every tensor that
# is indexed by row, and the key -> row mapping is rebuilt.

@torch.no_grad()
def hash_touch(rows, last_used, step):
    """Use stamps: last_used[rows[i]] = step for every position with
    0 <= rows[i] < capacity; last_used int64 [capacity] on the rows' device.
    GPU: one lane per position, plain stores, nothing read back."""
    if rows.dim() != 1 or rows.dtype != torch.int64:
        raise ValueError("hash_touch: rows must be int64 [n]")
    if last_used.dim() != 1 or last_used.dtype != torch.int64 or \
            last_used.device != rows.device or not last_used.is_contiguous():
        raise ValueError("hash_touch: last_used must be a contiguous int64 "
                         "[capacity] on the rows' device")
    if rows.is_cuda:
        _ext().hash_touch(rows.contiguous(), last_used, int(step))
        return
    ok = (rows >= 0) & (rows < last_used.numel())
    last_used[rows[ok]] = int(step)


def _hash_compact_check(index, keep, tables, last_used):
    cap, dev = index.capacity, index.row_keys.device
    if keep.dtype != torch.bool or tuple(keep.shape) != (cap,) or \
            keep.device != dev:
        raise ValueError("hash_compact: keep must be bool [capacity] = [%d] "
                         "on %s, got %s %s on %s"
                         % (cap, dev, keep.dtype, tuple(keep.shape),
                            keep.device))
    tables = list(tables)
    if len(tables) > 4:
        raise ValueError("hash_compact: at most 4 row tensors")
    for t in tables:
        if t.dim() != 2 or t.shape[0] != cap or t.device != dev or \
                t.dtype not in (torch.float32, torch.bfloat16) or \
                t.shape[1] != tables[0].shape[1] or not t.is_contiguous():
            raise ValueError("hash_compact: every row tensor must be a "
                             "contiguous fp32 or bf16 [capacity, D] = [%d, "
                             "D] on %s, got %s %s on %s"
                             % (cap, dev, t.dtype, tuple(t.shape), t.device))
    if last_used is not None and (
            last_used.dtype != torch.int64 or last_used.device != dev or
            tuple(last_used.shape) != (cap,) or
            not last_used.is_contiguous()):
        raise ValueError("hash_compact: last_used must be a contiguous int64 "
                         "[capacity] on the index's device")
    return tables


@torch.no_grad()
def hash_compact(index, keep, tables, last_used=None):
    """Keep the rows r < size with keep[r] and evict the others, in place:
    afterwards the K survivors own rows 0 .. K-1 of ``index.row_keys``, of
    every tensor of ``tables`` (at most four fp32 or bf16 [capacity, D]: a
    table's master, shadow and optimizer state) and of ``last_used`` (int64
    [capacity], optional). keep is bool [capacity] on the index's device;
    what it says at and beyond size is ignored. Returns nothing, reads
    nothing back.

    Hole filling, not a stable shift: the evicted rows below K (ascending)
    receive the kept rows at or above K (ascending), pair by pair, so a
    survivor below K keeps its row, at most min(evicted, survivors) rows
    move and no second copy of a tensor is needed. Then row_keys[K:size] =
    HASH_EMPTY, size = K, ``index.evicted`` grows by size - K and the
    key -> row mapping is rebuilt. Rows >= K of the row tensors are not
    written: they keep stale data until ``hash_init_new_rows`` hands them
    out again. The GPU (csrc/hash.hip) equals this reference integer for
    integer and bit for bit."""
    tables = _hash_compact_check(index, keep, tables, last_used)
    if index.device.type != "cpu":
        _ext().hash_compact(
            index.slot_keys, index.slot_rows, index.row_keys, index.size,
            index.evicted, keep.contiguous(), tables,
            last_used if last_used is not None
            else torch.empty(0, dtype=torch.int64, device=keep.device))
        return
    size = min(max(int(index.size), 0), index.capacity)
    kept = keep[:size]
    K = int(kept.sum())
    r = torch.arange(size)
    holes = r[:K][~kept[:K]]
    movers = r[K:][kept[K:]]
    for t in [index.row_keys] + tables + \
            ([last_used] if last_used is not None else []):
        t[holes] = t[movers]
    index.row_keys[K:size] = HASH_EMPTY
    index.size.fill_(K)
    index.evicted += size - K
    hash_rebuild(index)


@torch.no_grad()
def hash_remove(index, keys, tables, last_used=None):
    """Remove ``keys`` from the index: ``hash_compact`` with keep = every
    row but the ones ``hash_find`` returns for the keys. Absent keys,
    duplicates and HASH_EMPTY are ignored. No host sync."""
    rows = hash_find(index, keys)
    cap = index.capacity
    keep = torch.ones(cap + 1, dtype=torch.bool, device=rows.device)
    keep[torch.where(rows < 0, torch.full_like(rows, cap), rows)] = False
    hash_compact(index, keep[:cap], tables, last_used)


def _rows_or_zero(table, rows):
    """table[rows] with a zero row for every row outside [0, V) (CPU)."""
    keep = (rows >= 0) & (rows < table.shape[0])
    out = torch.zeros(rows.numel(), table.shape[1], dtype=table.dtype)
    out[keep] = table.index_select(0, rows[keep])
    return out


@torch.no_grad()
def hash_gather(index, table, keys):
    """The serving pull: out[i] = table[row of keys[i]], a zero row for an
    absent key — hash_find followed by embedding_gather, in ONE launch on
    the GPU (one wave per key probes 64 slots per step and copies the row).
    table bf16 [V,D]."""
    _hash_index_check(index, keys)
    if table.dim() != 2 or table.dtype != torch.bfloat16:
        raise ValueError("hash_gather: table must be bf16 [V,D]")
    if keys.is_cuda:
        return _ext().hash_gather(index.slot_keys, index.slot_rows, table,
                                  keys.contiguous())
    return _rows_or_zero(table, hash_find(index, keys))


def _hash_scale(dim):
    return np.float32(dim ** -0.5)


def hash_init_rows(keys, dim, seed, key_mul=1, key_add=0):
    """The initial rows of ``keys``: fp32 [n, dim] on the CPU (the
    reference of the init kernel, equal to it bit for bit). Column c of the
    row of key k is a pure function of (seed, k, c) — not of insertion
    order, capacity or sharding:

        G = 0x9E3779B97F4A7C15
        mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9
                z = (z ^ z >> 27) * 0x94D049BB133111EB
                return z ^ z >> 31                      (splitmix64)
        k = key * key_mul + key_add
        z = mix(mix(mix(seed + G) ^ k) + c * G)         (wrapping uint64)
        value = float32(z >> 40) * 2**-24 * float32(dim ** -0.5)

    The top 24 bits are an exact fp32 integer and the product by 2**-24 is
    exact; the product by the scale is one fp32 rounding: uniform in
    [0, dim**-0.5), the distribution of EmbeddingTable's rand / sqrt(dim).
    key_mul / key_add turn the local key of a shard into its global key."""
    _hash_keys_check(keys)
    k = _u64_array(keys) * np.array([key_mul % _U64], dtype=np.uint64) \
        + np.array([key_add % _U64], dtype=np.uint64)
    a = _mix64(np.array([(seed + _HASH_GOLD) % _U64], dtype=np.uint64))
    b = _mix64(a ^ k)
    cols = np.arange(dim, dtype=np.uint64) * np.uint64(_HASH_GOLD)
    z = _mix64(b[:, None] + cols[None, :])
    u = (z >> np.uint64(40)).astype(np.float32)
    return torch.from_numpy(u * np.float32(2.0 ** -24) * _hash_scale(dim))


def _stamps_arg(op, last_used, keys):
    if last_used is None:
        return None
    if last_used.dim() != 1 or last_used.dtype != torch.int64 or \
            last_used.device != keys.device or not last_used.is_contiguous():
        raise ValueError("%s: last_used must be a contiguous int64 "
                         "[capacity] on the keys' device" % op)
    return last_used


def _absent_init_rows(rows, keys, dim, seed, key_mul, key_add):
    """CPU: (which positions hold a real key without a row, the bf16
    initial rows of those keys)."""
    miss = (rows < 0) & (keys != HASH_EMPTY)
    init = hash_init_rows(keys[miss], dim, seed, key_mul, key_add)
    return miss, init.to(torch.bfloat16)


@torch.no_grad()
def hash_gather_init(index, table, keys, seed, key_mul=1, key_add=0,
                     last_used=None, step=0):
    """The training pull of a table with admission: ``hash_gather``, but a
    key that has no row (HASH_EMPTY excepted, it still reads zeros) reads
    bf16(its initial row) — ``hash_init_rows(keys, D, seed, key_mul,
    key_add)``, the bits ``hash_init_new_rows`` would put into the shadow —
    computed in registers, nothing stored. With ``last_used`` (int64
    [capacity]) a hit stores ``step`` into last_used[row]. One launch on the
    GPU. table bf16 [V,D]."""
    _hash_index_check(index, keys)
    if table.dim() != 2 or table.dtype != torch.bfloat16:
        raise ValueError("hash_gather_init: table must be bf16 [V,D]")
    last_used = _stamps_arg("hash_gather_init", last_used, keys)
    if keys.is_cuda:
        return _ext().hash_gather_init(
            index.slot_keys, index.slot_rows, table, keys.contiguous(),
            last_used if last_used is not None
            else torch.empty(0, dtype=torch.int64, device=keys.device),
            int(step), int(seed), int(key_mul), int(key_add),
            float(_hash_scale(table.shape[1])))
    rows = hash_find(index, keys)
    out = _rows_or_zero(table, rows)
    miss, init = _absent_init_rows(rows, keys, table.shape[1], seed, key_mul,
                                   key_add)
    out[miss] = init
    if last_used is not None:
        hash_touch(torch.where(rows < table.shape[0], rows,
                               torch.full_like(rows, -1)), last_used, step)
    return out


@torch.no_grad()
def hash_embedding_bag(index, table, keys, offsets, weights=None,
                       combiner="sum", out_dtype=None, init=None,
                       last_used=None, step=0):
    """``embedding_bag`` by key, the lookup fused in (one launch on the
    GPU): position i contributes c_i * table[row of keys[i]]. A key without
    a row contributes nothing — but still counts in a mean's weight sum —
    unless ``init=(seed, key_mul, key_add)`` is given: then it contributes
    its initial row rounded to bf16 (``hash_init_rows``), computed in
    registers. HASH_EMPTY never contributes. Bit for bit
    ``embedding_bag(cat([table, bf16 initial rows of the absent keys]),
    ids)`` with ids = the rows and the absent keys pointed at the appended
    rows: same accumulation order, same arithmetic. With ``last_used`` the
    rows of the keys inside the bags get ``step``. table bf16 [V,D], V >= 1;
    out_dtype bf16 (default) or torch.float32."""
    _hash_index_check(index, keys)
    _bag_check(keys, offsets, weights, combiner)
    if table.dim() != 2 or table.dtype != torch.bfloat16 or \
            table.shape[0] < 1:
        raise ValueError("hash_embedding_bag: table must be bf16 [V,D] with "
                         "V >= 1")
    out_dtype = table.dtype if out_dtype is None else out_dtype
    if out_dtype not in (table.dtype, torch.float32):
        raise ValueError("hash_embedding_bag: out_dtype must be "
                         "torch.bfloat16 or torch.float32")
    last_used = _stamps_arg("hash_embedding_bag", last_used, keys)
    seed, key_mul, key_add = (0, 1, 0) if init is None else init
    if keys.is_cuda:
        return _ext().hash_embedding_bag(
            index.slot_keys, index.slot_rows, table, keys.contiguous(),
            offsets.contiguous(), _bag_weights(weights, table.device),
            combiner == "mean", out_dtype == torch.float32,
            last_used if last_used is not None
            else torch.empty(0, dtype=torch.int64, device=keys.device),
            int(step), init is not None, int(seed), int(key_mul),
            int(key_add), float(_hash_scale(table.shape[1])))
    rows = hash_find(index, keys)
    V = table.shape[0]
    if init is not None:
        miss, extra = _absent_init_rows(rows, keys, table.shape[1], seed,
                                        key_mul, key_add)
        ids = rows.clone()
        ids[miss] = V + torch.arange(int(miss.sum()))
        ids[rows >= V] = -1     # a row the table cannot hold: nothing
        out = embedding_bag(torch.cat([table, extra]), ids, offsets,
                            weights=weights, combiner=combiner,
                            out_dtype=out_dtype)
    else:
        out = embedding_bag(table, rows, offsets, weights=weights,
                            combiner=combiner, out_dtype=out_dtype)
    if last_used is not None:
        hash_touch(torch.where(rows < V, rows, torch.full_like(rows, -1)),
                   last_used, step)
    return out


@torch.no_grad()
def hash_init_new_rows(keys, rows, is_new, master, shadow, states, seed,
                       key_mul=1, key_add=0):
    """In place, for every position i with is_new[i] (a find_or_insert that
    allocated rows[i]): master[rows[i]] = hash_init_rows(keys[i]), shadow
    the bf16 of it, and a zero row in every tensor of ``states`` (at most
    two). master fp32, shadow bf16, states fp32, all [V, D]. GPU: one
    kernel, grid sized from n, nothing read back."""
    _hash_keys_check(keys)
    n = keys.numel()
    if tuple(rows.shape) != (n,) or rows.dtype != torch.int64 or \
            tuple(is_new.shape) != (n,) or is_new.dtype != torch.bool:
        raise ValueError("hash_init_new_rows: need rows int64 [n] and is_new "
                         "bool [n] for n = %d keys" % n)
    if master.dim() != 2 or master.dtype != torch.float32 or \
            shadow.dtype != torch.bfloat16 or shadow.shape != master.shape:
        raise ValueError("hash_init_new_rows: master must be fp32 [V,D] and "
                         "shadow bf16 [V,D]")
    states = list(states)
    if len(states) > 2 or any(s.dtype != torch.float32 or
                              s.shape != master.shape for s in states):
        raise ValueError("hash_init_new_rows: states must be at most two "
                         "fp32 [V,D] tensors")
    if master.is_cuda:
        _ext().hash_init_new_rows(
            keys.contiguous(), rows.contiguous(), is_new.contiguous(),
            master, shadow, states, int(seed), int(key_mul), int(key_add),
            float(_hash_scale(master.shape[1])))
        return
    sel = is_new & (rows >= 0) & (rows < master.shape[0])
    r = rows[sel]
    vals = hash_init_rows(keys[sel], master.shape[1], seed, key_mul, key_add)
    master[r] = vals
    shadow[r] = vals.to(torch.bfloat16)
    for s in states:
        s[r] = 0.0


# ------------------------------------------------- sparse optimizer applies
#
# TF SparseApply* semantics: per touched row r the summed gradient is
# G = grad_scale * sum_{i: ids[i]==r} grads[i] (+ weight_decay * p), then
# the dense per-element formula runs ONCE on that row; ids outside [0, V)
# are ignored; untouched rows (and their state) never move. GPU: one fused
# HIP pass over master + state + bf16 shadow (csrc/sparse_apply.hip), no
# float atomics, bit-reproducible, no host sync.
#
# Pooled push (``offsets=`` given): ids/offsets/weights/combiner describe
# bags as for embedding_bag, grads is [B,D] BAG gradients and position i of
# bag b contributes c_i * grads[b]; everything above then holds unchanged.
# The GPU kernel reads the bag rows through the indirection (the n x D
# expanded rows are never built); the CPU reference builds them.

_SPARSE_SGD, _SPARSE_SGD_MOM, _SPARSE_ADAGRAD, _SPARSE_ADAM = 0, 1, 2, 3
_SPARSE_FTRL = 4


def _sparse_hip(code, param, ids, grads, s1, s2, bf16_out, step, lr, beta1,
                beta2, eps, weight_decay, grad_scale, bag=None,
                ftrl=(0.0, 0.0, 0.1)):
    """ftrl: (l1, l2, initial_accumulator_value), read by _SPARSE_FTRL."""
    dev = param.device
    l1, l2, acc0 = (float(x) for x in ftrl)
    ef = torch.empty(0, device=dev)
    if bag is not None:
        offsets, weights, combiner = bag
        _ext().sparse_apply_bag(
            param, ids.contiguous(), offsets.contiguous(),
            _bag_weights(weights, dev), grads,
            s1 if s1 is not None else ef, s2 if s2 is not None else ef,
            bf16_out if bf16_out is not None
            else torch.empty(0, dtype=torch.bfloat16, device=dev),
            code, int(step), combiner == "mean", float(lr), float(beta1),
            float(beta2), float(eps), float(weight_decay), float(grad_scale),
            l1, l2, acc0)
        return
    _ext().sparse_apply(
        param, ids, grads, s1 if s1 is not None else ef,
        s2 if s2 is not None else ef,
        bf16_out if bf16_out is not None
        else torch.empty(0, dtype=torch.bfloat16, device=dev),
        code, int(step), float(lr), float(beta1), float(beta2), float(eps),
        float(weight_decay), float(grad_scale), l1, l2, acc0)


def _bag_of_call(ids, grads, offsets, weights, combiner):
    """(offsets, weights, combiner) of a pooled call, None for a row call."""
    if offsets is None:
        if weights is not None:
            raise ValueError("weights need offsets (a pooled push)")
        return None
    _bag_check(ids, offsets, weights, combiner)
    if grads.dim() != 2 or grads.shape[0] != offsets.numel() - 1:
        raise ValueError("pooled push: grads must be [B,D] = [%d,D], got %s"
                         % (offsets.numel() - 1, tuple(grads.shape)))
    return offsets, weights, combiner


def _bag_rows_cpu(ids, grads, bag):
    """CPU reference: the per-position rows c_i * grads[bag_of[i]], fp32."""
    bag_of, c = _bag_expand_cpu(ids, *bag)
    return c[:, None] * grads.float()[bag_of]


def _sparse_cpu(param, ids, grads, states, bf16_out, dense_step):
    """CPU reference: drop out-of-range ids, sum duplicates (unique +
    index_add_), run the dense CPU formula on the gathered rows and
    scatter them back. dense_step(p, G, *state_rows) updates in place."""
    keep = (ids >= 0) & (ids < param.shape[0])
    ids = ids[keep]
    if ids.numel() == 0:
        return
    uniq, inv = torch.unique(ids, return_inverse=True)
    G = torch.zeros(uniq.numel(), param.shape[1])
    G.index_add_(0, inv, grads[keep].float())
    p = param.index_select(0, uniq)
    rows = [s.index_select(0, uniq) for s in states]
    dense_step(p, G, *rows)
    param.index_copy_(0, uniq, p)
    for s, r in zip(states, rows):
        s.index_copy_(0, uniq, r)
    if bf16_out is not None:
        bf16_out.index_copy_(0, uniq, p.to(torch.bfloat16))


@torch.no_grad()
def sparse_sgd(param, ids, grads, lr, momentum=0.0, momentum_buf=None,
               weight_decay=0.0, bf16_out=None, grad_scale=1.0, *,
               offsets=None, weights=None, combiner="sum"):
    """Sparse SGD(+momentum, +wd) on the rows ``ids`` of an fp32 [V,D]
    master; grads [n,D] bf16 or fp32. bf16_out ([V,D] shadow) gets the
    touched rows refreshed in the same pass. With ``offsets``: a pooled
    push, grads [B,D] bag gradients."""
    if momentum and momentum_buf is None:
        raise ValueError("sparse_sgd: momentum needs a momentum_buf")
    if not momentum:
        momentum_buf = None
    bag = _bag_of_call(ids, grads, offsets, weights, combiner)
    if param.is_cuda:
        _sparse_hip(_SPARSE_SGD_MOM if momentum else _SPARSE_SGD, param, ids,
                    grads, momentum_buf, None, bf16_out, 1, lr, momentum, 0.0,
                    0.0, weight_decay, grad_scale, bag=bag)
        return
    if bag is not None:
        grads = _bag_rows_cpu(ids, grads, bag)

    def step(p, g, *mb):
        fused_sgd(p, g, lr, momentum=momentum, weight_decay=weight_decay,
                  momentum_buf=mb[0] if mb else None, grad_scale=grad_scale)
    _sparse_cpu(param, ids, grads,
                [momentum_buf] if momentum else [], bf16_out, step)


@torch.no_grad()
def sparse_adagrad(param, ids, grads, accum, lr, eps=1e-10,
                   weight_decay=0.0, bf16_out=None, grad_scale=1.0, *,
                   offsets=None, weights=None, combiner="sum"):
    """Sparse Adagrad: a += G^2; p -= lr*G/(sqrt(a)+eps) per touched row
    (ids [3,3] with grads g,-g leave row and accumulator untouched).
    With ``offsets``: a pooled push, grads [B,D] bag gradients."""
    bag = _bag_of_call(ids, grads, offsets, weights, combiner)
    if param.is_cuda:
        _sparse_hip(_SPARSE_ADAGRAD, param, ids, grads, accum, None,
                    bf16_out, 1, lr, 0.0, 0.0, eps, weight_decay, grad_scale,
                    bag=bag)
        return
    if bag is not None:
        grads = _bag_rows_cpu(ids, grads, bag)

    def step(p, g, a):
        fused_adagrad(p, g, a, lr, eps=eps, weight_decay=weight_decay,
                      grad_scale=grad_scale)
    _sparse_cpu(param, ids, grads, [accum], bf16_out, step)


@torch.no_grad()
def sparse_adam(param, ids, grads, exp_avg, exp_avg_sq, step, lr,
                beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
                bf16_out=None, grad_scale=1.0, *, offsets=None, weights=None,
                combiner="sum"):
    """Lazy sparse Adam: only touched rows (and their m, v) move; the
    bias corrections come from ``step`` (>= 1). With ``offsets``: a
    pooled push, grads [B,D] bag gradients."""
    bag = _bag_of_call(ids, grads, offsets, weights, combiner)
    if param.is_cuda:
        _sparse_hip(_SPARSE_ADAM, param, ids, grads, exp_avg, exp_avg_sq,
                    bf16_out, step, lr, beta1, beta2, eps, weight_decay,
                    grad_scale, bag=bag)
        return
    if bag is not None:
        grads = _bag_rows_cpu(ids, grads, bag)

    def dense(p, g, m, v):
        fused_adam(p, g, m, v, step, lr, beta1=beta1, beta2=beta2, eps=eps,
                   weight_decay=weight_decay, grad_scale=grad_scale)
    _sparse_cpu(param, ids, grads, [exp_avg, exp_avg_sq], bf16_out, dense)


@torch.no_grad()
def sparse_ftrl(param, ids, grads, accum, linear, lr, l1=0.0, l2=0.0,
                initial_accumulator_value=0.1, bf16_out=None, grad_scale=1.0,
                *, offsets=None, weights=None, combiner="sum"):
    """Sparse FTRL-Proximal: the rule of ``fused_ftrl`` once per touched
    row on its summed gradient; accum and linear ([V,D], zeros at the
    start) move only on touched rows. A touched row whose summed gradient
    is zero (ids [3,3] with grads g,-g) keeps its weights up to rounding
    but gets its linear term seeded. With ``offsets``: a pooled push,
    grads [B,D] bag gradients."""
    acc0 = initial_accumulator_value
    _ftrl_check(lr, l1, l2, acc0)
    bag = _bag_of_call(ids, grads, offsets, weights, combiner)
    if param.is_cuda:
        _sparse_hip(_SPARSE_FTRL, param, ids, grads, accum, linear, bf16_out,
                    1, lr, 0.0, 0.0, 0.0, 0.0, grad_scale, bag=bag,
                    ftrl=(l1, l2, acc0))
        return
    if bag is not None:
        grads = _bag_rows_cpu(ids, grads, bag)

    def step(p, g, a, c):
        fused_ftrl(p, g, a, c, lr, l1=l1, l2=l2,
                   initial_accumulator_value=acc0, grad_scale=grad_scale)
    _sparse_cpu(param, ids, grads, [accum, linear], bf16_out, step)


# --------------------------------------------------------------- relu bwd

def relu_bwd(grad_out, act):
    """dx = grad_out * (act > 0)."""
    if grad_out.is_cuda:
        return _ext().relu_bwd(grad_out, act)
    return (grad_out.float() * (act.float() > 0)).to(grad_out.dtype)


# --------------------------------------------------------------------- conv

class _Conv2dFn(torch.autograd.Function):
    """Autograd wrapper over the implicit-GEMM HIP conv kernels (NCHW,
    bf16 activations/weights, fp32 weight grads). The Inception path
    (BASELINE.json conv config) builds on this; CPU falls back to the
    torch fp32 reference so model code runs in CI."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, padding, krsc, dw_out=None,
                dw_cb=None):
        ctx.stride = stride
        ctx.padding = padding
        ctx.has_bias = bias is not None
        ctx.krsc = krsc
        ctx.dw_out = dw_out
        ctx.dw_cb = dw_cb
        ctx.pw = False
        if x.is_cuda:
            # channels-last memory: gathers become contiguous channel
            # runs (csrc/conv.hip); weights are tap-major [K,R,S,C] —
            # either natively (krsc params skip the per-call permute)
            # or permuted here from KCRS
            xm = x.contiguous(memory_format=torch.channels_last)
            wm = w.contiguous() if krsc else \
                w.permute(0, 2, 3, 1).contiguous()
            ctx.save_for_backward(xm, w)
            ctx.pw = (wm.shape[1] == 1 and wm.shape[2] == 1
                      and stride == (1, 1) and padding == (0, 0))
            if ctx.pw:
                # pointwise conv IS a GEMM over pixels; the tuned GEMM
                # kernel (csrc/gemm.hip) beats the implicit-GEMM conv
                # path on the large-P Inception shapes (tools/
                # bench_1x1.py: 7.3 vs 9.2 us fwd at 35^2) but loses on
                # 8^2 (its tile grid is too small without split-tap),
                # hence the P gate
                N, C, H, W = xm.shape
                P = N * H * W
                if P >= 4096:
                    x2 = xm.permute(0, 2, 3, 1).reshape(P, C)
                    eb = bias.float() if bias is not None else None
                    y2 = gemm_bias_act(x2, wm.view(wm.shape[0], C),
                                       bias=eb, trans_b=True)
                    return y2.view(N, H, W, -1).permute(0, 3, 1, 2)
            eb = bias.float() if bias is not None else \
                torch.empty(0, device=x.device)
            return _ext().conv2d_fwd(xm, wm, eb, stride[0], stride[1],
                                     padding[0], padding[1], False)
        ctx.save_for_backward(x, w)
        wf = w.permute(0, 3, 1, 2).float() if krsc else w.float()
        y = torch.nn.functional.conv2d(
            x.float(), wf, bias.float() if bias is not None else None,
            stride=stride, padding=padding)
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        krsc = ctx.krsc
        if x.is_cuda:
            # channel-narrow concat-grad views are read strided by the
            # conv kernels (ConvShape.LDY) — no contiguous() copy
            if not _is_cl_narrow(dy):
                dy = dy.contiguous(memory_format=torch.channels_last)
            R, S = (w.shape[1], w.shape[2]) if krsc \
                else (w.shape[2], w.shape[3])
            dx = None
            if ctx.needs_input_grad[0]:
                # kernel reads W in its native [K,R,S,C] layout (the
                # fwd tensor) — krsc params pass straight through
                wk = w if krsc else w.permute(0, 2, 3, 1).contiguous()
                if ctx.pw:
                    # pointwise: dX = dY @ W on the tuned GEMM kernel
                    # (faster than the conv bwd-data path on every
                    # Inception 1x1 shape — tools/bench_1x1.py); the
                    # GEMM path needs a dense 2-D view
                    dy = dy.contiguous(memory_format=torch.channels_last)
                    N, K, Ho, Wo = dy.shape
                    dy2 = dy.permute(0, 2, 3, 1).reshape(N * Ho * Wo, K)
                    dx2 = gemm_bias_act(dy2, wk.reshape(K, -1))
                    dx = dx2.view(N, Ho, Wo, -1).permute(0, 3, 1, 2)
                else:
                    dx = _ext().conv2d_bwd_data(
                        dy, wk, x.shape[2], x.shape[3],
                        ctx.stride[0], ctx.stride[1],
                        ctx.padding[0], ctx.padding[1])
            if ctx.dw_out is not None:
                # grad-arena path (krsc only): atomically accumulate
                # into the model's pre-zeroed fp32 buffer; the trainer
                # gathers it with one batched bf16 copy — no per-layer
                # fill / cast kernels, and autograd sees no w grad.
                _ext().conv2d_bwd_weight_out(
                    dy, x, R, S, ctx.stride[0], ctx.stride[1],
                    ctx.padding[0], ctx.padding[1], ctx.dw_out)
                dw = None
                if ctx.dw_cb is not None:
                    # comm-overlap hook: the dW kernel for this layer is
                    # now ENQUEUED on the compute stream, so a reduce
                    # issued here is stream-ordered after it — the
                    # bucket manager uses this to overlap the PS push
                    # with the rest of backward (ps/module_trainer.py)
                    ctx.dw_cb()
            else:
                dwm = _ext().conv2d_bwd_weight(
                    dy, x, R, S, ctx.stride[0], ctx.stride[1],
                    ctx.padding[0], ctx.padding[1])
                # kernel emits tap-major [K,R,S,C]: native for krsc
                dw = dwm.to(w.dtype) if krsc \
                    else dwm.permute(0, 3, 1, 2).to(w.dtype)
        else:
            dy = dy.contiguous()
            wk = w.permute(0, 3, 1, 2) if krsc else w
            dyf, xf, wf = dy.float(), x.float(), wk.float()
            dx = None
            if ctx.needs_input_grad[0]:
                dx = torch.nn.grad.conv2d_input(
                    x.shape, wf, dyf, stride=ctx.stride,
                    padding=ctx.padding).to(x.dtype)
            dw = torch.nn.grad.conv2d_weight(
                xf, wk.shape, dyf, stride=ctx.stride, padding=ctx.padding)
            if krsc:
                dw = dw.permute(0, 2, 3, 1)
            dw = dw.contiguous().to(w.dtype)
        db = dy.float().sum(dim=(0, 2, 3)) if ctx.has_bias else None
        return dx, dw, db, None, None, None, None, None


def conv2d(x, w, bias=None, stride=1, padding=0, weight_format="kcrs",
           dw_out=None, dw_cb=None):
    """2-D convolution (NCHW activations): hand-written implicit-GEMM
    MFMA kernels on GPU (csrc/conv.hip), torch fp32 reference on CPU.
    Differentiable. weight_format "kcrs" (torch layout) or "krsc"
    (tap-major — the kernels' native layout; parameters stored this way
    skip a permute+copy per call in fwd AND in the weight-grad path).

    dw_out (GPU + krsc only): a pre-zeroed fp32 [K,R,S,C] buffer the
    weight grad is atomically accumulated into instead of being returned
    through autograd (w.grad stays None) — the model grad-arena path
    that batches ~90 per-layer fill/cast kernels into one bulk zero and
    one foreach gather copy per step."""
    if isinstance(stride, int):
        stride = (stride, stride)
    if isinstance(padding, int):
        padding = (padding, padding)
    if dw_out is not None:
        assert weight_format == "krsc" and x.is_cuda, \
            "dw_out requires krsc weights on GPU"
    return _Conv2dFn.apply(x, w, bias, tuple(stride), tuple(padding),
                           weight_format == "krsc", dw_out, dw_cb)


class _SoftmaxXentFn(torch.autograd.Function):
    """Differentiable fused softmax cross-entropy (mean over batch) on
    the HIP kernels; used by autograd models (Inception classifier)."""

    @staticmethod
    def forward(ctx, logits, labels):
        if logits.is_cuda:
            loss, probs = _ext().softmax_xent_fwd(logits, labels)
        else:
            lg = logits.float()
            probs = torch.softmax(lg, 1).to(logits.dtype)
            loss = torch.nn.functional.cross_entropy(lg, labels)
        ctx.save_for_backward(probs, labels)
        return loss

    @staticmethod
    def backward(ctx, gl):
        probs, labels = ctx.saved_tensors
        B = probs.shape[0]
        d = softmax_xent_bwd(probs, labels, scale=1.0 / B)
        if not torch.equal(gl, torch.ones_like(gl)):
            d = d * gl.to(d.dtype)
        return d, None


def softmax_xent_loss(logits, labels):
    """Mean softmax cross-entropy, differentiable w.r.t. logits."""
    return _SoftmaxXentFn.apply(logits, labels)


class _LinearFn(torch.autograd.Function):
    """Differentiable y = x @ w + b on the MFMA GEMM kernels (bf16).
    Backward reuses the fused epilogues: dx = dy w^T, dw = x^T dy with
    the bias-grad colsum fused into the dw GEMM."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        if x.is_cuda:
            return gemm_bias_act(x, w, b)
        y = x.float() @ w.float()
        if b is not None:
            y = y + b.float()
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        if x.is_cuda:
            db = torch.empty(w.shape[1], dtype=torch.float32,
                             device=x.device) if ctx.has_bias else None
            dw = torch.empty(w.shape, dtype=torch.float32, device=x.device)
            gemm_bias_act(x, dy, trans_a=True, out=dw, colsum_out=db)
            dx = gemm_bias_act(dy, w, trans_b=True)
            dw = dw.to(w.dtype)
        else:
            dyf = dy.float()
            dx = (dyf @ w.float().t()).to(x.dtype)
            dw = (x.float().t() @ dyf).to(w.dtype)
            db = dyf.sum(0) if ctx.has_bias else None
        return dx, dw, db


def linear(x, w, b=None):
    """Differentiable linear layer on the hand-written MFMA GEMM."""
    return _LinearFn.apply(x, w, b)


def _is_cl_narrow(t):
    """Channels-last tensor OR a channel-narrow view of one (torch.cat's
    backward hands out such views; the HIP BN/pool backward kernels read
    them in place instead of copying)."""
    if t.dim() != 4:
        return False
    s = t.stride()
    return (s[1] == 1 and s[3] >= t.shape[1] and s[2] == t.shape[3] * s[3]
            and s[0] == t.shape[2] * s[2])


class _BatchNormActFn(torch.autograd.Function):
    """Fused train-mode batch-norm (+ optional relu) on the HIP kernels
    (csrc/bn.hip); fp32 torch reference on CPU."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, relu, out=None):
        if x.is_cuda:
            x = x.contiguous(memory_format=torch.channels_last)
            eout = out if out is not None \
                else torch.empty(0, device=x.device, dtype=torch.bfloat16)
            y, mean, invstd = _ext().bn_fwd(
                x, weight.to(torch.bfloat16), bias.to(torch.bfloat16),
                eps, relu, eout)
            if out is not None:
                # the apply wrote into the caller's concat-buffer view;
                # detach severs the view metadata so autograd attaches
                # this Function's backward instead of rejecting the
                # aliased output (see _JoinViews in models/inception.py)
                ctx.save_for_backward(x, None, weight, bias, mean, invstd)
                ctx.relu = relu
                return y.detach()
            # y is NOT saved for backward: the relu mask is recomputed
            # from sign(g*xhat + b) inside the bwd kernels
        else:
            xf = x.float()
            mean = xf.mean(dim=(0, 2, 3))
            var = xf.var(dim=(0, 2, 3), unbiased=False)
            invstd = torch.rsqrt(var + eps)
            y = (xf - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
            y = y * weight.float().view(1, -1, 1, 1) \
                + bias.float().view(1, -1, 1, 1)
            if relu:
                y = torch.relu(y)
            y = y.to(x.dtype)
            if out is not None:
                with torch.no_grad():
                    out.copy_(y)
                ctx.save_for_backward(x, out, weight, bias, mean, invstd)
                ctx.relu = relu
                return out.detach()
        ctx.save_for_backward(x, y, weight, bias, mean, invstd)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, bias, mean, invstd = ctx.saved_tensors
        if x.is_cuda:
            if not _is_cl_narrow(dy):
                dy = dy.contiguous(memory_format=torch.channels_last)
            dx, dgamma, dbeta = _ext().bn_bwd(
                x, dy, weight.to(torch.bfloat16), bias.to(torch.bfloat16),
                mean, invstd, ctx.relu)
        else:
            dyf = dy.contiguous().float()
            if ctx.relu:
                dyf = dyf * (y.float() > 0)
            xf = x.float()
            nhw = x.numel() / x.shape[1]
            xhat = (xf - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
            s1 = dyf.sum(dim=(0, 2, 3))
            s2 = (dyf * xhat).sum(dim=(0, 2, 3))
            dgamma, dbeta = s2, s1
            dx = (weight.float() * invstd).view(1, -1, 1, 1) * (
                dyf - (s1 / nhw).view(1, -1, 1, 1)
                - xhat * (s2 / nhw).view(1, -1, 1, 1))
            dx = dx.to(x.dtype)
        return (dx, dgamma.to(weight.dtype), dbeta.to(weight.dtype), None,
                None, None)


class _GroupBNFn(torch.autograd.Function):
    """Grouped train-mode BN(+relu) over parallel branches of an
    Inception block: ONE stats/finalize/apply launch triple for ALL
    branches (per-channel math — results identical to per-branch BNs;
    at these layer sizes the per-kernel execution floor made launch
    count the dominant BN cost).

    out_view None: the branches get separate dense outputs, returned as
    a tuple (inner-stage BNs feeding different consumers). Otherwise the
    results go into consecutive channel slices of out_view, a
    channel-narrow view of the block's concat buffer, which is returned
    (same .detach() contract as _BatchNormActFn's out= path; see
    _JoinViews)."""

    @staticmethod
    def forward(ctx, out_view, eps, relu, n, *args):
        xs = [a.contiguous(memory_format=torch.channels_last)
              for a in args[:n]]
        gs = [g.to(torch.bfloat16) for g in args[n:2 * n]]
        bs = [b.to(torch.bfloat16) for b in args[2 * n:3 * n]]
        outs = [] if out_view is None else [out_view]
        *ys, mean, invstd = _ext().bn_group_fwd(xs, gs, bs, outs, eps, relu)
        ctx.save_for_backward(mean, invstd, *xs, *gs, *bs)
        ctx.n = n
        ctx.relu = relu
        return tuple(ys) if out_view is None else out_view.detach()

    @staticmethod
    def backward(ctx, *dys):
        n = ctx.n
        saved = ctx.saved_tensors
        mean, invstd = saved[0], saved[1]
        xs = list(saved[2:2 + n])
        gs = list(saved[2 + n:2 + 2 * n])
        bs = list(saved[2 + 2 * n:2 + 3 * n])
        # one dy per output: per branch, or the one over the concat view
        dys = [d if _is_cl_narrow(d)
               else d.contiguous(memory_format=torch.channels_last)
               for d in dys]
        widths = [g.numel() for g in gs]
        *dxs, dgamma, dbeta = _ext().bn_group_bwd(
            xs, dys, gs, bs, mean, invstd, ctx.relu)
        return (None, None, None, None, *dxs, *dgamma.split(widths),
                *dbeta.split(widths))


def bn_group_multi(xs, weights, biases, eps=1e-3, relu=True):
    """Grouped BN for parallel branches with separate outputs (GPU
    only). Returns the per-branch normalized tensors."""
    return _GroupBNFn.apply(None, eps, relu, len(xs), *xs,
                            *weights, *biases)


def bn_group_apply(out_view, xs, weights, biases, eps=1e-3, relu=True):
    """Grouped BN over parallel branches (GPU only): normalizes each
    xs[i] with (weights[i], biases[i]) and writes the results into
    consecutive channel slices of ``out_view`` (a channels-last or
    channel-narrow view whose C == sum of branch channels)."""
    return _GroupBNFn.apply(out_view, eps, relu, len(xs),
                            *xs, *weights, *biases)


def batch_norm_act(x, weight, bias, eps=1e-3, relu=False, out=None):
    """Differentiable fused train-mode BN (+relu); channels-last on GPU.

    out (optional): a channel-narrow channels-last view the normalized
    output is written into (strided store) — the Inception blocks pass
    slices of a pre-allocated concat buffer so the block concat costs
    zero copies (see models/inception.py _fused_cat)."""
    if not x.is_cuda:
        x = x.contiguous()
    return _BatchNormActFn.apply(x, weight, bias, eps, relu, out)


def mlp_head_fused(h, w, b, labels, scale=None, dw2=None, db2=None):
    """Fused classifier head (one kernel): logits = h@w+b, softmax,
    mean xent loss, dlogits = (p-onehot)*scale, dh = (dlogits@w^T)
    masked by h>0 (h is a relu output), and — when dw2/db2 (fp32 or
    bf16 grad views) are given on the MFMA path (B<=128, H<=128) —
    dW2 = h^T@dlogits and db2 = colsum(dlogits) in the SAME kernel.
    Returns (loss, dlogits, dh). GPU limits C<=16, H<=512, B<=512;
    CPU reference otherwise."""
    B = h.shape[0]
    s = float(scale if scale is not None else 1.0 / B)
    if h.is_cuda:
        e = torch.empty(0, device=h.device)
        return _ext().mlp_head_fused(h, w, b, labels, s,
                                     dw2 if dw2 is not None else e,
                                     db2 if db2 is not None else e)
    hf, wf = h.float(), w.float()
    logits = hf @ wf + b.float()
    probs = torch.softmax(logits, 1)
    loss = torch.nn.functional.cross_entropy(logits, labels)
    d = probs.clone()
    d[torch.arange(B), labels] -= 1.0
    d *= s
    dh = (d @ wf.t()) * (hf > 0)
    db = d.to(h.dtype)
    if dw2 is not None:
        dw2.copy_((hf.t() @ db.float()).reshape(dw2.shape).to(dw2.dtype))
        db2.copy_(db.float().sum(0).to(db2.dtype))
    return loss, db, dh.to(h.dtype)


def mlp_tail_sgd(x, dh, w1_m, w1_s, b1_m, b1_s, g_w2, w2_m, w2_s,
                 g_b2, b2_m, b2_s, lr):
    """mnist single-GPU fused tail (one kernel): dW1 = x^T @ dh on the
    small-tile GEMM with the plain-SGD apply of ALL FOUR params fused
    into the epilogue — W1/b1 straight from the fp32 accumulators
    (the gradient never materializes), W2/b2 by re-reading the small
    bf16 classifier grads the head kernel wrote. Masters are fp32
    flat-store views; shadows the matching bf16 views. Only valid for
    sgd with no momentum/weight-decay and grad_scale 1 (the world==1
    colocated bench config); the PS path applies via fused_sgd.
    GPU-only (raises elsewhere — keep the HIP path the one that runs).
    """
    return _ext().mlp_tail_sgd(x, dh, w1_m, w1_s, b1_m, b1_s,
                               g_w2, w2_m, w2_s, g_b2, b2_m, b2_s,
                               float(lr))


def mlp_head_tail_grads(x, h, w2, b2, y, dw1, db1, dw2, db2):
    """Classifier head + dW1 tail in ONE kernel (GPU, csrc/gemm.hip
    mlp_head_tail_kernel): every block of the dW1 = x^T @ dh GEMM
    recomputes the logits / softmax / dh slice it consumes, so dh never
    touches global memory; blocks of their own produce db1, dW2, and db2
    with the loss. Fills dw1, db1, dw2, db2 (one dtype, fp32 or bf16)
    and returns the mean loss — bit-identical to mlp_head_fused +
    gemm_bias_act's dW1 GEMM (the small-tile kernel's sum order from 32
    tiles up, the 64x64 kernel's below). Limits: B<=128, H<=128
    (H%4==0), C<=16, 2..512 32x32 tiles. CPU: composed fp32 reference."""
    if x.is_cuda:
        return _ext().mlp_head_tail_grads(x, h, w2, b2, y, dw1, db1,
                                          dw2, db2)
    loss, _, dh = mlp_head_fused(h, w2, b2, y, dw2=dw2, db2=db2)
    dhf = dh.float()
    dw1.copy_((x.float().t() @ dhf).to(dw1.dtype))
    db1.copy_(dhf.sum(0).to(db1.dtype))
    return loss


def mlp_fwd_snap(x, w1, b1, w2_s, b2_s):
    """mnist fwd hidden layer h = relu(x @ w1 + b1) (same kernels and
    bits as gemm_bias_act) whose launch (the one-launch forward, or the
    split-K stripe reduce) ALSO copies the 2 KB classifier shadow
    (w2_s, b2_s) into a per-device snapshot buffer. Returns (h, snap) for mlp_head_tail_sgd(snap=...): reading
    the snapshot instead of the live shadow lets it apply W2/b2 without
    the arrival ticket (~5 us). snap is None where the GEMM runs a path
    that takes no snapshot, and on CPU."""
    if x.is_cuda:
        h, snap = _ext().mlp_fwd_snap(x, w1, b1, w2_s, b2_s)
        return h, (snap if snap.numel() else None)
    return gemm_bias_act(x, w1, b1, act="relu"), None


@torch.no_grad()
def mlp_head_tail_sgd(x, h, w2_s, b2_s, y, w1_m, b1_m, w2_m, b2_m,
                      w1_s, b1_s, lr, snap=None):
    """mnist single-GPU step, head + tail + plain-SGD apply in ONE kernel
    (GPU): as mlp_head_tail_grads, with W1/b1 applied straight from the
    fp32 accumulators and W2/b2 (read from the live shadows w2_s/b2_s,
    grads rounded to bf16 as the two-kernel path stores them) applied by
    the block that arrives last — or, given mlp_fwd_snap's ``snap`` of
    this step, by a fixed block concurrently (the kernel then reads
    W2/b2 from the snapshot). *_m are the fp32 masters, *_s the bf16
    shadows; all eight are updated in place. Returns the mean loss.
    Only valid for sgd without momentum/weight-decay and grad_scale 1.
    CPU: composed fp32 reference."""
    if x.is_cuda:
        return _ext().mlp_head_tail_sgd(
            x, h, w2_s, b2_s, y, w1_m, b1_m, w2_m, b2_m, w1_s, b1_s,
            float(lr), snap if snap is not None
            else torch.empty(0, dtype=torch.bfloat16, device=x.device))
    dw2 = torch.empty_like(w2_s)
    db2 = torch.empty_like(b2_s)
    loss, _, dh = mlp_head_fused(h, w2_s, b2_s, y, dw2=dw2, db2=db2)
    dhf = dh.float()
    grads = ((w1_m, w1_s, x.float().t() @ dhf), (b1_m, b1_s, dhf.sum(0)),
             (w2_m, w2_s, dw2.float()), (b2_m, b2_s, db2.float()))
    for m, s, g in grads:
        m.add_(g.reshape(m.shape), alpha=-float(lr))
        s.copy_(m.to(s.dtype))
    return loss


def mlp_fwd_head_fused(x, w1, b1, w2, b2, labels, scale=None,
                       dw2=None, db2=None):
    """Whole MLP fwd + classifier head in TWO kernels (GPU): split-K
    GEMM stripes for h = relu(x@w1+b1), then the fused MFMA head
    consumes the stripes directly — h never exists in global memory.
    Returns (loss, dh); dw2/db2 classifier grads are written by the
    head when given. Limits: B<=128, H<=128 (H%4==0), C<=16.
    CPU: composed fp32 reference."""
    B = x.shape[0]
    s = float(scale if scale is not None else 1.0 / B)
    if x.is_cuda:
        e = torch.empty(0, device=x.device)
        return _ext().mlp_fwd_head_fused(
            x, w1, b1, w2, b2, labels, s,
            dw2 if dw2 is not None else e,
            db2 if db2 is not None else e)
    h = torch.relu(x.float() @ w1.float() + b1.float()).to(x.dtype)
    loss, _, dh = mlp_head_fused(h, w2, b2, labels, scale=s,
                                 dw2=dw2, db2=db2)
    return loss, dh


class _AvgPool3x3Fn(torch.autograd.Function):
    """3x3 stride-1 pad-1 average pool (the Inception block pool) on a
    channels-last HIP stencil kernel; the stencil is symmetric so the
    backward is the same kernel applied to dy."""

    @staticmethod
    def forward(ctx, x):
        if x.is_cuda:
            return _ext().avg_pool3x3(
                x.contiguous(memory_format=torch.channels_last))
        return torch.nn.functional.avg_pool2d(
            x.float(), 3, stride=1, padding=1).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        if dy.is_cuda:
            return _ext().avg_pool3x3(
                dy.contiguous(memory_format=torch.channels_last))
        return torch.nn.functional.avg_pool2d(
            dy.float(), 3, stride=1, padding=1).to(dy.dtype)


def avg_pool3x3(x):
    """Differentiable 3x3/s1/p1 average pool (count_include_pad)."""
    return _AvgPool3x3Fn.apply(x)


class _MaxPool3x3s2Fn(torch.autograd.Function):
    """3x3 stride-2 max pool (the Inception reduction pool) — forward
    saves the winning tap; backward gathers deterministically."""

    @staticmethod
    def forward(ctx, x, out=None):
        if x.is_cuda:
            x = x.contiguous(memory_format=torch.channels_last)
            e = out if out is not None \
                else torch.empty(0, device=x.device, dtype=x.dtype)
            y, idx = _ext().maxpool3x3s2_fwd(x, e)
            ctx.save_for_backward(idx)
            ctx.hw = (x.shape[2], x.shape[3])
            ctx.gpu = True
            return y
        ctx.gpu = False
        y, idx = torch.nn.functional.max_pool2d(
            x.float(), 3, stride=2, return_indices=True)
        ctx.save_for_backward(idx)
        ctx.xshape = x.shape
        y = y.to(x.dtype)
        if out is not None:
            out.copy_(y)
            return out
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        if ctx.gpu:
            if not _is_cl_narrow(dy):
                dy = dy.contiguous(memory_format=torch.channels_last)
            return _ext().maxpool3x3s2_bwd(dy, idx, *ctx.hw), None
        return torch.nn.functional.max_unpool2d(
            dy.float(), idx, 3, stride=2,
            output_size=ctx.xshape[2:]).to(dy.dtype), None


def max_pool3x3s2(x, out=None):
    """Differentiable 3x3/s2 max pool (no padding). out (GPU): a
    channel-narrow channels-last view — the kernel stores the block's
    concat slice directly (Inception B/D reduction blocks)."""
    return _MaxPool3x3s2Fn.apply(x, out)
