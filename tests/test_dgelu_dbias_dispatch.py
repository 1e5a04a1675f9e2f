"""Routing of the fused GELU-backward + fc1-bias-gradient pass
(ops/linear.py TunedGemmMode, csrc/gelu.hip) on the CPU, through the
mode's ``dgelu_handler`` seam with a fake kernel in plain torch: which
ops are answered, that gradients are unchanged, and that the one-entry
stash never answers the wrong sum or outlives its step."""

import pytest
import torch
import torch.nn.functional as F

from vit_10b_fsdp_example_amd.ops import linear as linmod

B, T, D, HID = 2, 3, 4, 16


@pytest.fixture()
def fake_kernel(monkeypatch):
    calls = {"dgelu": 0}

    def handler(dy, x):
        calls["dgelu"] += 1
        dx = torch.ops.aten.gelu_backward(dy, x, approximate="none")
        return dx, dx.reshape(-1, dx.shape[-1]).sum(0)

    monkeypatch.delenv("VITFSDP_FUSED_DGELU_DBIAS", raising=False)
    monkeypatch.delenv("VITFSDP_FUSED_GELU", raising=False)
    monkeypatch.setitem(linmod._GELU_CFG, "d", D)
    monkeypatch.setitem(linmod._GELU_CFG, "hid", HID)
    return calls, handler


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g, requires_grad=True)
            for s in ((HID, D), (HID,), (D, HID), (D,))]


def _mlp(x, p):
    w1, b1, w2, b2 = p
    return F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2)


def _mode(handler):
    return linmod.TunedGemmMode(table={}, native_wgrad=False,
                                dgelu_handler=handler)


def _grads(x, p):
    return [x.grad] + [t.grad for t in p]


def test_one_gelu_backward_and_one_sum_per_mlp(fake_kernel):
    calls, handler = fake_kernel
    p1, p2 = _params(0), _params(1)
    x = torch.randn(B, T, D, requires_grad=True)
    with _mode(handler) as m:
        y = _mlp(_mlp(x, p1), p2)  # two MLPs back to back
        y.pow(2).sum().backward()
    assert calls["dgelu"] == 2
    assert m.dgelu_hits == 2
    assert m.dbias_hits == 2  # fc1's bias sums only, not fc2's
    assert m._dgelu_stash is None


def test_gradients_equal_switch_off(fake_kernel, monkeypatch):
    calls, handler = fake_kernel
    p = _params(2)
    x = torch.randn(B, T, D, requires_grad=True)
    with _mode(handler) as m:
        _mlp(x, p).pow(2).sum().backward()
    assert m.dgelu_hits == 1 and m.dbias_hits == 1
    on = [g.clone() for g in _grads(x, p)]

    monkeypatch.setenv("VITFSDP_FUSED_DGELU_DBIAS", "0")
    for t in [x] + p:
        t.grad = None
    with _mode(handler) as m:
        assert not m.fused_dgelu
        _mlp(x, p).pow(2).sum().backward()
    assert m.dgelu_hits == 0 and m.dbias_hits == 0 and calls["dgelu"] == 1
    for a, b in zip(on, _grads(x, p)):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-6), a.shape


def test_switch_and_config_gate_the_context(fake_kernel, monkeypatch):
    """gemm_dispatch_context() activates the mode for this hook alone
    (no tuned table), and not when it is switched off."""
    monkeypatch.setattr(linmod, "lt_algo_table", lambda: {})
    monkeypatch.setattr(linmod, "_NATIVE_WGRAD_DISPATCH", False)
    assert isinstance(linmod.gemm_dispatch_context(), linmod.TunedGemmMode)
    monkeypatch.setenv("VITFSDP_FUSED_DGELU_DBIAS", "0")
    assert not isinstance(linmod.gemm_dispatch_context(),
                          linmod.TunedGemmMode)
    monkeypatch.delenv("VITFSDP_FUSED_DGELU_DBIAS")
    monkeypatch.setitem(linmod._GELU_CFG, "hid", 0)
    assert not isinstance(linmod.gemm_dispatch_context(),
                          linmod.TunedGemmMode)


def test_unrelated_sum_not_answered_from_stash(fake_kernel):
    _, handler = fake_kernel
    dy = torch.randn(B, T, HID)
    pre = torch.randn(B, T, HID)
    with _mode(handler) as m:
        dx = torch.ops.aten.gelu_backward(dy, pre, approximate="none")
        assert m.dgelu_hits == 1 and m._dgelu_stash is not None
        other = torch.randn(B * T, HID)  # same shape, different storage
        s_other = other.sum(0, keepdim=True)
        assert m.dbias_hits == 0
        # same tensor, but not the row reduction
        s_cols = dx.view(B * T, HID).sum(1)
        s_all = dx.view(B * T, HID).sum((0, 1))
        assert m.dbias_hits == 0 and m._dgelu_stash is not None
        # a slice shares the storage pointer but not the element count
        s_part = dx.view(B * T, HID)[:3].sum(0, keepdim=True)
        assert m.dbias_hits == 0
        s_dx = dx.view(B * T, HID).sum(0, keepdim=True)
        assert m.dbias_hits == 1 and m._dgelu_stash is None
    assert torch.equal(s_other, other.sum(0, keepdim=True))
    assert torch.equal(s_cols, dx.view(B * T, HID).sum(1))
    assert torch.equal(s_all, dx.sum())
    assert torch.equal(s_part, dx.view(B * T, HID)[:3].sum(0, keepdim=True))
    assert s_dx.shape == (1, HID)
    assert torch.allclose(s_dx, dx.view(B * T, HID).sum(0, keepdim=True))


def test_keepdim_false_shape(fake_kernel):
    _, handler = fake_kernel
    dy, pre = torch.randn(B * T, HID), torch.randn(B * T, HID)
    with _mode(handler) as m:
        dx = torch.ops.aten.gelu_backward(dy, pre, approximate="none")
        s = dx.sum(0)
        assert m.dbias_hits == 1
    assert s.shape == (HID,)
    assert torch.allclose(s, dx.sum(0))


def test_other_gelu_backward_falls_through(fake_kernel):
    calls, handler = fake_kernel
    with _mode(handler) as m:
        # last dim is not the MLP hidden dim
        torch.ops.aten.gelu_backward(torch.randn(5, D), torch.randn(5, D),
                                     approximate="none")
        # tanh approximation
        torch.ops.aten.gelu_backward(torch.randn(5, HID), torch.randn(5, HID),
                                     approximate="tanh")
    assert calls["dgelu"] == 0 and m.dgelu_hits == 0


def test_stash_empty_after_mode_exit(fake_kernel):
    _, handler = fake_kernel
    m = _mode(handler)
    with m:
        torch.ops.aten.gelu_backward(torch.randn(B * T, HID),
                                     torch.randn(B * T, HID),
                                     approximate="none")
        assert m._dgelu_stash is not None
    assert m._dgelu_stash is None


def test_unanswered_stash_does_not_leak_into_next_step(fake_kernel):
    """A gelu_backward whose sum never arrives (no bias on fc1): the next
    step's gelu_backward replaces the entry and that step's bias gradient
    is its own."""
    _, handler = fake_kernel
    m = _mode(handler)
    with m:
        stale = torch.ops.aten.gelu_backward(
            torch.randn(B * T, HID), torch.randn(B * T, HID),
            approximate="none")
        stale_sum = stale.sum(0)  # computed by torch below, not stashed
    assert m._dgelu_stash is None  # consumed here; now leave one parked:
    with m:
        torch.ops.aten.gelu_backward(torch.randn(B * T, HID),
                                     torch.randn(B * T, HID),
                                     approximate="none")
    assert m._dgelu_stash is None  # cleared by the exit

    p = _params(5)
    x = torch.randn(B, T, D, requires_grad=True)
    with m:
        parked = torch.ops.aten.gelu_backward(
            torch.randn(B * T, HID), torch.randn(B * T, HID),
            approximate="none")  # never summed
        _mlp(x, p).pow(2).sum().backward()
        assert m._dgelu_stash is None
    got = p[1].grad.clone()
    for t in [x] + p:
        t.grad = None
    _mlp(x, p).pow(2).sum().backward()
    assert torch.allclose(got, p[1].grad, rtol=1e-6, atol=1e-6)
    assert not torch.allclose(got, parked.sum(0))
    assert not torch.allclose(got, stale_sum)
