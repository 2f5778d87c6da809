"""The bound single-GPU mnist step (ops.mlp_sgd_step, csrc/ext.hip
MlpSgdStep): mlp_fwd_snap + mlp_head_tail_sgd with everything that stays
the same from step to step settled once. It launches the same two
kernels with the same arguments, so every comparison with the two ops is
EXACT (torch.equal) on masters, shadows and loss, step by step over five
steps of different batches. What can break: an argument bound wrongly or
left stale (labels, stream, the alignment class of x), a check dropped
from run(), a step that outlives what it was built for in the model's
cache.

The two-op reference of a case is computed once, shared and never
modified."""

import pytest
import torch

from tfmesos_amd import ops
from tfmesos_amd.models import mlp
from tfmesos_amd.models.mlp import MnistMLP
from tfmesos_amd.ps.replica import SyncReplicaTrainer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR = 0.05
STEPS = 5
NAMES = ("w1", "b1", "w2", "b2")

# (B, M, H, C), elements x starts into its storage
CASES = [
    ((100, 784, 100, 10), 0),  # the benchmark's
    ((7, 300, 36, 3), 0),      # ragged: 2 H tiles, M % 8 != 0, odd C
    ((128, 264, 128, 16), 0),  # the limits; M no multiple of the tile
    ((7, 300, 36, 3), 1),      # x a view 2 bytes into its storage
]
IDS = ["%s+%d" % ("x".join(map(str, s)), off) for s, off in CASES]
NO_SNAP = (100, 128, 100, 10)   # K < 256: an unsliced forward, no snapshot


def _on_fwd1(shape):
    B, M, H, C = shape
    return ops._ext().gemm_plan(B, H, M, False, False, 1, False, 0)[0] \
        == "fwd1"


class _Store(object):
    """fp32 masters + bf16 shadows, one plain allocation each."""

    def __init__(self, shape):
        B, M, H, C = shape
        g = torch.Generator().manual_seed(3 + M + H + C)
        shp = {"w1": (M, H), "b1": (H,), "w2": (H, C), "b2": (C,)}
        self.m = {n: (torch.randn(*shp[n], generator=g) * 0.1).to(DEV)
                  for n in NAMES}
        self.s = {n: self.m[n].to(torch.bfloat16) for n in NAMES}

    def clone(self):
        c = object.__new__(_Store)
        c.m = {n: t.clone() for n, t in self.m.items()}
        c.s = {n: t.clone() for n, t in self.s.items()}
        return c


def _assert_stores_equal(a, b):
    for n in NAMES:
        assert torch.equal(a.m[n], b.m[n]), ("master", n)
        assert torch.equal(a.s[n], b.s[n]), ("shadow", n)


def _batches(shape, xoff=0, n=STEPS):
    """n different (x, y); x a view `xoff` elements into its storage."""
    B, M, H, C = shape
    g = torch.Generator().manual_seed(B + M + H + C)
    out = []
    for _ in range(n):
        buf = torch.zeros(xoff + B * M, device=DEV, dtype=torch.bfloat16)
        x = buf[xoff:].view(B, M)
        x.copy_(torch.rand(B, M, generator=g))
        out.append((x, torch.randint(0, C, (B,), generator=g).to(DEV)))
    return out


def _two_ops(x, y, m, s, lr):
    """The reference: the two ops as MnistMLP.fwd_bwd_apply calls them."""
    h, snap = ops.mlp_fwd_snap(x, s["w1"], s["b1"], s["w2"], s["b2"])
    return ops.mlp_head_tail_sgd(
        x, h, s["w2"], s["b2"], y, m["w1"], m["b1"], m["w2"], m["b2"],
        s["w1"], s["b1"], lr, snap=snap)


def _bind(st, shape, lr=LR):
    return ops.mlp_sgd_step(
        st.m["w1"], st.m["b1"], st.m["w2"], st.m["b2"], st.s["w1"],
        st.s["b1"], st.s["w2"], st.s["b2"], lr, *shape)


_REF = {}


def _reference(shape, xoff=0):
    """Store and losses after STEPS two-op steps over _batches."""
    key = (shape, xoff)
    if key not in _REF:
        st = _Store(shape)
        losses = [_two_ops(x, y, st.m, st.s, LR)
                  for x, y in _batches(shape, xoff)]
        torch.cuda.synchronize()
        _REF[key] = (st, losses)
    return _REF[key]


@pytest.mark.parametrize("shape,xoff", CASES, ids=IDS)
def test_five_steps_equal_the_two_ops(shape, xoff):
    assert _on_fwd1(shape)
    ref, ref_losses = _reference(shape, xoff)
    st = _Store(shape)
    step = _bind(st, shape)
    for i, (x, y) in enumerate(_batches(shape, xoff)):
        assert x.data_ptr() % 16 == 2 * xoff
        loss = step.run(x, y)
        assert loss.shape == () and loss.dtype == torch.float32
        assert torch.equal(loss, ref_losses[i]), ("loss", i)
    torch.cuda.synchronize()
    _assert_stores_equal(st, ref)


def test_loss_tensor_is_the_steps_own():
    """run() creates no tensor: one loss tensor, rewritten by each run."""
    shape = CASES[1][0]
    step = _bind(_Store(shape), shape)
    (x0, y0), (x1, y1) = _batches(shape)[:2]
    a = step.run(x0, y0)
    kept = a.clone()
    b = step.run(x1, y1)
    assert b.data_ptr() == a.data_ptr()
    assert torch.equal(kept, _reference(shape)[1][0])
    assert torch.equal(a, _reference(shape)[1][1])


@pytest.mark.parametrize("shape", [CASES[0][0], CASES[1][0]],
                         ids=[IDS[0], IDS[1]])
def test_capture_and_three_replays_equal_four_eager_runs(shape):
    batches = _batches(shape)[:4]
    eager = _Store(shape)
    estep = _bind(eager, shape)
    eager_losses = [estep.run(x, y).clone() for x, y in batches]

    st = _Store(shape)
    step = _bind(st, shape)
    x, y = batches[0][0].clone(), batches[0][1].clone()
    assert torch.equal(step.run(x, y), eager_losses[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):      # capture itself runs nothing
        loss = step.run(x, y)
    for i in (1, 2, 3):
        x.copy_(batches[i][0])
        y.copy_(batches[i][1])
        graph.replay()
        assert torch.equal(loss, eager_losses[i]), ("loss", i)
        assert torch.equal(loss, _reference(shape)[1][i])
    torch.cuda.synchronize()
    _assert_stores_equal(st, eager)


def test_runs_on_the_current_stream():
    shape = CASES[1][0]
    ref, ref_losses = _reference(shape)
    st = _Store(shape)
    step = _bind(st, shape)
    batches = _batches(shape)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    losses = []
    with torch.cuda.stream(side):
        for x, y in batches:
            losses.append(step.run(x, y).clone())
    side.synchronize()
    for i in range(STEPS):
        assert torch.equal(losses[i], ref_losses[i]), ("loss", i)
    _assert_stores_equal(st, ref)


def test_run_rejects_what_it_was_not_built_for_without_launching():
    shape = (16, 264, 36, 3)
    assert _on_fwd1(shape)
    B, M, H, C = shape
    st = _Store(shape)
    before = st.clone()
    step = _bind(st, shape)
    (x, y), = _batches(shape, n=1)
    x8 = _batches(shape, xoff=1, n=1)[0][0]    # M % 8 == 0, 2 bytes off
    bad = [
        (torch.zeros(B + 1, M, device=DEV, dtype=torch.bfloat16), y),
        (torch.zeros(B, M + 8, device=DEV, dtype=torch.bfloat16), y),
        (x.float(), y),
        (x.cpu(), y),
        (torch.zeros(M, B, device=DEV, dtype=torch.bfloat16).t(), y),
        (x8, y),
        (x, y.int()),
        (x, y[:-1]),
        (x, y.cpu()),
    ]
    for xb, yb in bad:
        with pytest.raises(RuntimeError):
            step.run(xb, yb)
    torch.cuda.synchronize()
    _assert_stores_equal(st, before)


def test_binding_checks_the_buffers_once():
    shape = CASES[1][0]
    st = _Store(shape)
    B, M, H, C = shape
    with pytest.raises(RuntimeError):            # geometry != buffers
        _bind(st, (B, M, H + 4, C))
    half = _Store(shape)
    half.m["w1"] = half.m["w1"].to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="masters must be fp32"):
        _bind(half, shape)
    cpu = _Store(shape)
    cpu.s["b2"] = cpu.s["b2"].cpu()
    with pytest.raises(RuntimeError):
        _bind(cpu, shape)


def _trainer(model):
    return SyncReplicaTrainer(model.init_params(), optimizer="sgd",
                              hparams={"lr": LR}, device=torch.device(DEV),
                              grad_dtype=torch.bfloat16)


def _model_two_ops(t, x, y, lr):
    st = t.store
    names = {"w1": "hid_w", "b1": "hid_b", "w2": "sm_w", "b2": "sm_b"}
    m = {k: st.view(n) for k, n in names.items()}
    s = {k: st.view(n, bf16=True) for k, n in names.items()}
    return _two_ops(x, y, m, s, lr)


def _assert_trainers_equal(a, b):
    assert torch.equal(a.store.flat, b.store.flat)
    assert torch.equal(a.store.flat_bf16, b.store.flat_bf16)


def test_no_snapshot_geometry_is_refused_and_the_model_keeps_the_ops():
    B, M, H, C = NO_SNAP
    assert not _on_fwd1(NO_SNAP)
    with pytest.raises(RuntimeError, match="snapshot"):
        _bind(_Store(NO_SNAP), NO_SNAP)
    model = MnistMLP(hidden_units=H, image_pixels=M, classes=C)
    t, twin = _trainer(model), _trainer(model)
    for x, y in _batches(NO_SNAP, n=3):
        assert model._headtail_ok(x)
        loss = model.fwd_bwd_apply(t, x, y, lr=LR)
        assert model._step is None
        assert torch.equal(loss, _model_two_ops(twin, x, y, LR))
    torch.cuda.synchronize()
    assert t.store.global_step == 3
    _assert_trainers_equal(t, twin)


def test_model_rebuilds_the_step_when_lr_or_batch_size_change():
    model = MnistMLP()
    t, twin = _trainer(model), _trainer(model)
    b100 = _batches((100, 784, 100, 10), n=2)
    b64 = _batches((64, 784, 100, 10), n=1)
    plan = [(b100[0], 0.05), (b100[1], 0.05), (b100[0], 0.02),
            (b64[0], 0.02), (b100[1], 0.02)]
    steps = []
    for (x, y), lr in plan:
        loss = model.fwd_bwd_apply(t, x, y, lr=lr)
        assert torch.equal(loss, _model_two_ops(twin, x, y, lr))
        steps.append(model._step)
    torch.cuda.synchronize()
    assert steps[0] is not None and steps[1] is steps[0]
    assert steps[2] is not steps[1] and steps[3] is not steps[2]
    assert steps[4] is not steps[3]
    assert t.store.global_step == len(plan)
    _assert_trainers_equal(t, twin)


def test_env_switch_keeps_the_two_ops(monkeypatch):
    monkeypatch.setattr(mlp, "_STEP", False)
    model = MnistMLP()
    t, twin = _trainer(model), _trainer(model)
    (x, y), = _batches((100, 784, 100, 10), n=1)
    loss = model.fwd_bwd_apply(t, x, y, lr=LR)
    assert model._step is None
    assert torch.equal(loss, _model_two_ops(twin, x, y, LR))
    _assert_trainers_equal(t, twin)


def test_bound_step_survives_store_load(tmp_path):
    """PStore.load copies into the buffers the step is bound to."""
    model = MnistMLP()
    t = _trainer(model)
    batches = _batches((100, 784, 100, 10))
    for x, y in batches[:2]:
        model.fwd_bwd_apply(t, x, y, lr=LR)
    step = model._step
    path = str(tmp_path / "ck.pt")
    t.store.save(path)
    losses = [model.fwd_bwd_apply(t, x, y, lr=LR).clone()
              for x, y in batches[2:]]
    flat, flat_bf16 = t.store.flat.clone(), t.store.flat_bf16.clone()

    t.store.load(path)
    assert t.store.global_step == 2
    assert not torch.equal(t.store.flat, flat)
    for i, (x, y) in enumerate(batches[2:]):
        assert torch.equal(model.fwd_bwd_apply(t, x, y, lr=LR), losses[i])
        assert model._step is step
    torch.cuda.synchronize()
    assert torch.equal(t.store.flat, flat)
    assert torch.equal(t.store.flat_bf16, flat_bf16)
