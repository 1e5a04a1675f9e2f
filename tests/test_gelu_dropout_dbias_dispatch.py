"""Routing of the fused GELU+dropout backward + fc1-bias-gradient pass
(ops/linear.py TunedGemmMode, the DROP kernels of csrc/gelu.hip) on the
CPU: the registered op vitfsdp::gelu_dropout_bwd reaches the mode from an
autograd backward, the ``dgelu_drop_handler`` seam answers it with a fake
kernel in plain torch, the parked sums and dx^T are consumed by the bias
sum and the TN weight gradient of fc1 exactly as the p = 0 route's are,
and gradients are unchanged."""

import pytest
import torch
import torch.nn.functional as F

from vit_10b_fsdp_example_amd.ops import dropout as dropmod
from vit_10b_fsdp_example_amd.ops import linear as linmod

B, T, D, HID = 2, 4, 8, 24
P, SEED = 0.25, 1234


def _reference(dy, x, p, seed):
    """The composition the op stands for: the GELU backward of the scaled
    gradient, selected to 0 under the hash mask."""
    mask = dropmod.hidden_dropout_mask(seed, x.numel() // x.shape[-1],
                                       x.shape[-1], p).reshape(x.shape)
    dx = torch.ops.aten.gelu_backward(dy * (1.0 / (1.0 - p)), x,
                                      approximate="none")
    return torch.where(mask, dx, torch.zeros_like(dx))


class _GeluDrop(torch.autograd.Function):
    """dropout(gelu(x)) under the hash mask; the backward issues the
    registered op, as ops.dropout._GeluDropoutFn does on the GPU."""

    @staticmethod
    def forward(ctx, x, p, seed):
        ctx.save_for_backward(x)
        ctx.p, ctx.seed = p, seed
        mask = dropmod.hidden_dropout_mask(
            seed, x.numel() // x.shape[-1], x.shape[-1], p).reshape(x.shape)
        y = F.gelu(x) * (1.0 / (1.0 - p))
        return torch.where(mask, y, torch.zeros_like(y))

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dx = torch.ops.vitfsdp.gelu_dropout_bwd(
            dy.contiguous(), x, ctx.p, ctx.seed)
        return dx, None, None


class _Fakes:
    """Fake kernels that log what the routes ask of them."""

    def __init__(self):
        self.log = []

    def dgelu_drop(self, dy, x, p, seed):
        self.log.append(("dgelu_drop", tuple(dy.shape), p, seed))
        dx = _reference(dy, x, p, seed)
        return dx, dx.reshape(-1, dx.shape[-1]).sum(0)

    def gemm(self, a, b, idx, bias):
        self.log.append(("gemm", a, b))
        out = torch.mm(a, b)
        return out + bias if bias is not None else out

    def transpose(self, t, want_colsum):
        assert t.dim() == 2 and t.is_contiguous()
        self.log.append(("transpose", tuple(t.shape), want_colsum))
        return t.t().contiguous(), (t.sum(0) if want_colsum else None)

    def count(self, name):
        return len([e for e in self.log if e[0] == name])


@pytest.fixture()
def fakes(monkeypatch):
    for name in ("VITFSDP_FUSED_DGELU_DBIAS", "VITFSDP_FUSED_GELU",
                 "VITFSDP_TN_WGRAD", "VITFSDP_TN_DGELU_T"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", -1)  # TN gate: 10B shapes
    monkeypatch.setitem(linmod._GELU_CFG, "d", D)
    monkeypatch.setitem(linmod._GELU_CFG, "hid", HID)
    return _Fakes()


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g, requires_grad=True)
            for s in ((HID, D), (HID,), (D, HID), (D,))]


def _mlp(x, p, seed=SEED):
    w1, b1, w2, b2 = p
    return F.linear(_GeluDrop.apply(F.linear(x, w1, b1), P, seed), w2, b2)


def _mode(fakes, **kw):
    return linmod.TunedGemmMode(table={}, native_wgrad=False,
                                dgelu_drop_handler=fakes.dgelu_drop, **kw)


def _grads(x, p):
    return [x.grad] + [t.grad for t in p]


def test_one_fake_call_and_one_answered_sum_per_mlp(fakes):
    p1, p2 = _params(0), _params(1)
    x = torch.randn(B, T, D, requires_grad=True)
    m = _mode(fakes)
    with m:
        y = _mlp(_mlp(x, p1, seed=1), p2, seed=2)  # two MLPs back to back
        y.pow(2).sum().backward()
        assert m._dgelu_stash is None  # after the step
    assert fakes.log == [("dgelu_drop", (B, T, HID), P, 2),
                         ("dgelu_drop", (B, T, HID), P, 1)]
    assert m.dgelu_drop_hits == 2 and m.dgelu_hits == 0
    assert m.dbias_hits == 2  # fc1's bias sums only, not fc2's
    assert m._dgelu_stash is None

    # parked, never summed: the exit clears it
    with m:
        torch.ops.vitfsdp.gelu_dropout_bwd(
            torch.randn(B * T, HID), torch.randn(B * T, HID), P, SEED)
        assert m._dgelu_stash is not None
    assert m._dgelu_stash is None


def test_gradients_equal_switch_off(fakes, monkeypatch):
    p = _params(2)
    x = torch.randn(B, T, D, requires_grad=True)
    with _mode(fakes) as m:
        _mlp(x, p).pow(2).sum().backward()
    assert m.dgelu_drop_hits == 1 and m.dbias_hits == 1
    on = [g.clone() for g in _grads(x, p)]

    monkeypatch.setenv("VITFSDP_FUSED_DGELU_DBIAS", "0")
    for t in [x] + p:
        t.grad = None
    with _mode(fakes) as m:
        assert not m.fused_dgelu_drop
        _mlp(x, p).pow(2).sum().backward()
    assert m.dgelu_drop_hits == 0 and m.dbias_hits == 0
    assert fakes.count("dgelu_drop") == 1
    for a, b in zip(on, _grads(x, p)):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-6), a.shape


@pytest.mark.parametrize("dgelu_t", [True, False])
def test_tn_route_takes_the_parked_transpose(fakes, monkeypatch, dgelu_t):
    """fc1's weight-gradient GEMM gets the dx^T the route parked; with
    VITFSDP_TN_DGELU_T=0 it is one transpose call without sums instead.
    Either way no pass over fc1's dy makes sums again."""
    monkeypatch.setenv("VITFSDP_TN_DGELU_T", "1" if dgelu_t else "0")
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", 0)
    monkeypatch.setattr(linmod, "_DGELU_DROP_T", True)  # route the _t kernel
    p = _params(3)
    x = torch.randn(B, T, D, requires_grad=True)
    with _mode(fakes, handler=fakes.gemm, tn_handler=fakes.transpose) as m:
        _mlp(x, p).pow(2).sum().backward()
        assert m._tn_stash is None and m._dgelu_stash is None
    assert m.dgelu_drop_hits == 1 and m.dbias_hits == 1
    assert m.tn_hits == 2 and m.tn_dbias_hits == 1  # fc2's sum
    tr = [e[1:] for e in fakes.log if e[0] == "transpose"]
    rows = B * T
    # fc2: dy with sums, then x; fc1: x only, or dy without sums and x
    fc1 = [((rows, D), False)] if dgelu_t else [((rows, HID), False),
                                               ((rows, D), False)]
    assert tr == [((rows, D), True), ((rows, HID), False)] + fc1
    # fc1's GEMM: first operand dx^T [hid, rows], row-contiguous, equal to
    # the transpose of the dx the fake kernel returned
    a = [e[1] for e in fakes.log
         if e[0] == "gemm" and tuple(e[1].shape) == (HID, rows)]
    assert len(a) == 1 and a[0].is_contiguous()
    # the gradients are those of the stock backward
    got = _grads(x, p)
    x2 = x.detach().clone().requires_grad_(True)
    p2 = [t.detach().clone().requires_grad_(True) for t in p]
    _mlp(x2, p2).pow(2).sum().backward()
    for u, v in zip(got, _grads(x2, p2)):
        assert torch.allclose(u, v, rtol=1e-5, atol=1e-5)
    # dx^T . 1 = column sums of dx = fc1's bias gradient
    assert torch.allclose(a[0].sum(1), p2[1].grad, rtol=1e-5, atol=1e-5)


def test_t_kernel_is_not_routed_by_default(fakes, monkeypatch):
    """_DGELU_DROP_T is off (the _t kernel did not clear its measurement):
    where fc1's weight gradient wants dx^T the route declines, and the
    sequence is the two-pass one, the stock op and one pass over its
    result for the sums and the transpose."""
    assert linmod._DGELU_DROP_T is False
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", 0)
    p = _params(3)
    x = torch.randn(B, T, D, requires_grad=True)
    with _mode(fakes, handler=fakes.gemm, tn_handler=fakes.transpose) as m:
        _mlp(x, p).pow(2).sum().backward()
        assert m._tn_stash is None and m._dgelu_stash is None
    assert m.dgelu_drop_hits == 0 and m.dbias_hits == 0
    assert fakes.count("dgelu_drop") == 0
    assert m.tn_hits == 2 and m.tn_dbias_hits == 2
    rows = B * T
    assert [e[1:] for e in fakes.log if e[0] == "transpose"] == [
        ((rows, D), True), ((rows, HID), False),
        ((rows, HID), True), ((rows, D), False)]
    x2 = x.detach().clone().requires_grad_(True)
    p2 = [t.detach().clone().requires_grad_(True) for t in p]
    _mlp(x2, p2).pow(2).sum().backward()
    for u, v in zip(_grads(x, p), _grads(x2, p2)):
        assert torch.allclose(u, v, rtol=1e-5, atol=1e-5)


def test_unrelated_sum_not_answered_from_stash(fakes):
    dy = torch.randn(B, T, HID)
    pre = torch.randn(B, T, HID)
    with _mode(fakes) as m:
        dx = torch.ops.vitfsdp.gelu_dropout_bwd(dy, pre, P, SEED)
        assert m.dgelu_drop_hits == 1 and m._dgelu_stash is not None
        other = torch.randn(B * T, HID)  # same shape, different storage
        s_other = other.sum(0, keepdim=True)
        # same tensor, but not the row reduction
        s_cols = dx.view(B * T, HID).sum(1)
        s_all = dx.view(B * T, HID).sum((0, 1))
        # a slice shares the storage pointer but not the element count
        s_part = dx.view(B * T, HID)[:3].sum(0, keepdim=True)
        assert m.dbias_hits == 0 and m._dgelu_stash is not None
        s_dx = dx.view(B * T, HID).sum(0, keepdim=True)
        assert m.dbias_hits == 1 and m._dgelu_stash is None
    assert torch.equal(s_other, other.sum(0, keepdim=True))
    assert torch.equal(s_cols, dx.view(B * T, HID).sum(1))
    assert torch.equal(s_all, dx.sum())
    assert torch.equal(s_part, dx.view(B * T, HID)[:3].sum(0, keepdim=True))
    assert s_dx.shape == (1, HID)
    assert torch.allclose(s_dx, dx.view(B * T, HID).sum(0, keepdim=True))


def test_op_outside_any_mode_is_the_reference_composition():
    g = torch.Generator().manual_seed(4)
    dy = torch.randn(B * T, HID, generator=g)
    x = torch.randn(B * T, HID, generator=g) * 2.0
    for p, seed in ((0.1, 0), (0.5, 2 ** 31 - 2)):
        dx = torch.ops.vitfsdp.gelu_dropout_bwd(dy, x, p, seed)
        ref = _reference(dy, x, p, seed)
        assert torch.equal(dx, ref)
        mask = dropmod.hidden_dropout_mask(seed, B * T, HID, p)
        assert bool((dx[~mask] == 0).all()) and 0 < int((~mask).sum())
    # and from an autograd backward
    xr = x.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(_GeluDrop.apply(xr, P, SEED), xr, dy)
    assert torch.equal(gx, _reference(dy, x, P, SEED))


def test_gated_out_calls_run_the_stock_implementation(fakes, monkeypatch):
    # last dim is not the MLP hidden dim
    dy, x = torch.randn(5, D), torch.randn(5, D)
    with _mode(fakes) as m:
        dx = torch.ops.vitfsdp.gelu_dropout_bwd(dy, x, P, SEED)
        assert m._dgelu_stash is None
    assert m.dgelu_drop_hits == 0 and fakes.log == []
    assert torch.equal(dx, _reference(dy, x, P, SEED))

    # mismatched shapes are not the route's either
    with _mode(fakes) as m:
        with pytest.raises(RuntimeError):
            torch.ops.vitfsdp.gelu_dropout_bwd(
                torch.randn(5, HID), torch.randn(4, HID), P, SEED)
    assert m.dgelu_drop_hits == 0 and fakes.log == []

    # no fake: the real kernel's gate (GPU bf16, hid % 8 == 0) decides,
    # and CPU tensors of a width that is no multiple of 8 pass neither
    monkeypatch.setitem(linmod._GELU_CFG, "hid", 20)
    dy, x = torch.randn(6, 20), torch.randn(6, 20)
    with linmod.TunedGemmMode(table={}, native_wgrad=False) as m:
        assert m.fused_dgelu_drop
        dx = torch.ops.vitfsdp.gelu_dropout_bwd(dy, x, P, SEED)
        assert m._dgelu_stash is None
        s = dx.sum(0)
    assert m.dgelu_drop_hits == 0 and m.dbias_hits == 0
    assert torch.equal(dx, _reference(dy, x, P, SEED))
    assert torch.equal(s, dx.sum(0))
