"""MnistMLP._bound_step: when the model builds, keeps and rebuilds its
bound step (ops.mlp_sgd_step), checked on CPU with a stub in the op's
place."""

import torch

from tfmesos_amd import ops
from tfmesos_amd.models import mlp
from tfmesos_amd.models.mlp import MnistMLP
from tfmesos_amd.ps.store import PStore


class _Stub(object):
    def __init__(self, *args):
        self.args = args


def _store(model):
    st = PStore(device="cpu")
    st.init_params(model.init_params(), optimizer="sgd", lr=0.01)
    return st


def _setup(monkeypatch, snapshot=True):
    built = []
    monkeypatch.setattr(mlp, "_fwd_takes_snapshot",
                        lambda B, M, H: snapshot)
    monkeypatch.setattr(ops, "mlp_sgd_step",
                        lambda *a: built.append(_Stub(*a)) or built[-1])
    return built


def test_step_is_built_once_from_the_stores_views(monkeypatch):
    built = _setup(monkeypatch)
    model = MnistMLP()
    st = _store(model)
    x = torch.zeros(100, 784)
    s = model._bound_step(st, x, 0.01)
    assert model._bound_step(st, x, 0.01) is s and len(built) == 1
    assert model._bound_step(st, torch.ones(100, 784), 0.01) is s
    tensors, rest = s.args[:8], s.args[8:]
    assert rest == (0.01, 100, 784, 100, 10)
    want = [st.view(n, bf16=b) for b in (False, True)
            for n in ("hid_w", "hid_b", "sm_w", "sm_b")]
    for got, w in zip(tensors, want):
        assert got.data_ptr() == w.data_ptr() and got.shape == w.shape
        assert got.dtype == w.dtype


def test_step_is_rebuilt_for_another_lr_shape_or_store(monkeypatch):
    built = _setup(monkeypatch)
    model = MnistMLP()
    st = _store(model)
    x = torch.zeros(100, 784)
    a = model._bound_step(st, x, 0.01)
    b = model._bound_step(st, x, 0.02)
    c = model._bound_step(st, torch.zeros(64, 784), 0.02)
    d = model._bound_step(_store(model), torch.zeros(64, 784), 0.02)
    assert len({id(s) for s in (a, b, c, d)}) == 4 and len(built) == 4
    assert c.args[8:] == (0.02, 64, 784, 100, 10)
    # a restore into the same buffers keeps the step
    st2 = _store(model)
    e = model._bound_step(st2, x, 0.01)
    st2.flat.copy_(torch.ones_like(st2.flat))
    assert model._bound_step(st2, x, 0.01) is e


def test_no_step_where_the_forward_takes_no_snapshot(monkeypatch):
    built = _setup(monkeypatch, snapshot=False)
    model = MnistMLP()
    st = _store(model)
    x = torch.zeros(100, 784)
    assert model._bound_step(st, x, 0.01) is None
    assert model._bound_step(st, x, 0.01) is None
    assert built == []
