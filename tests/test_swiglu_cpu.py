"""--mlp_type swiglu away from the GPU: the flag, the shapes it gives fc1
and fc2, the composition route with its gradients, and the routing of
vitfsdp::swiglu_bwd through TunedGemmMode with fake kernels."""

import pytest
import torch
import torch.nn.functional as F

from vit_10b_fsdp_example_amd.cli import parse_args
from vit_10b_fsdp_example_amd.models import (
    Block, FSDPViTModel, count_vit_params,
)
from vit_10b_fsdp_example_amd.ops import linear as linmod
from vit_10b_fsdp_example_amd.ops import (
    swiglu, swiglu_bwd_reference, swiglu_hidden_dim,
)
from vit_10b_fsdp_example_amd.parallel.checkpoint import n_open_mlp_blocks


def _model(**kw):
    torch.manual_seed(0)
    return FSDPViTModel(
        image_size=32, patch_size=4, embed_dim=64, num_heads=4, num_blocks=2,
        mlp_ratio=4.0, pos_dropout=0.0, mlp_dropout=0.0, att_dropout=0.0,
        num_classes=10, grad_ckpt_wrap=lambda m: m, fsdp_wrap=lambda m: m,
        **kw)


def test_flag_shapes_and_param_count(monkeypatch):
    assert parse_args([]).mlp_type == "gelu"
    assert parse_args(["--mlp_type", "swiglu"]).mlp_type == "swiglu"
    with pytest.raises(SystemExit):
        parse_args(["--mlp_type", "relu"])
    assert swiglu_hidden_dim(5120, 4.0) == 13824
    assert swiglu_hidden_dim(64, 4.0) == 256  # 170.67 rounded up to 256
    shapes = {k: tuple(v.shape) for k, v in
              _model(mlp_type="swiglu").state_dict().items()}
    assert list(shapes) == list(_model().state_dict())  # the same names
    assert shapes["blocks.1.mlp.fc1.weight"] == (512, 64)
    assert shapes["blocks.1.mlp.fc1.bias"] == (512,)
    assert shapes["blocks.1.mlp.fc2.weight"] == (64, 256)
    assert shapes["blocks.1.mlp.fc2.bias"] == (64,)
    n = sum(v.numel() for v in _model(mlp_type="swiglu").parameters())
    assert n == count_vit_params(32, 4, 64, 2, 4.0, 10, mlp_type="swiglu")
    # H happens to be the GELU width here: fc1 is twice as large per block
    assert n == count_vit_params(32, 4, 64, 2, 4.0, 10) + 2 * (64 * 256 + 256)
    # H freed and 2H kept per row; the default is the GELU MLP's count
    assert n_open_mlp_blocks(32, 16, 64, 256, 512) == 16 * 256 // (128 + 512)
    assert n_open_mlp_blocks(32, 16, 64, 256) == 16 * 256 // (128 + 256)
    with pytest.raises(ValueError):
        Block(64, 4, mlp_type="relu")
    monkeypatch.setenv("VITFSDP_FUSED_GELU", "1")
    with pytest.raises(ValueError, match="FUSED_GELU"):
        Block(64, 4, mlp_type="swiglu")


def test_gelu_model_and_its_step_do_not_see_the_flag():
    a, b = _model(), _model(mlp_type="gelu")
    assert a.state_dict()["blocks.0.mlp.fc1.weight"].shape == (256, 64)
    x, y = torch.randn(2, 3, 32, 32), torch.tensor([1, 2])
    for m in (a, b):
        F.cross_entropy(m(x), y).backward()
        torch.optim.SGD(m.parameters(), lr=0.1).step()
    for (k, u), v in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(u, v), k


def test_cpu_route_is_the_formula_with_its_gradients():
    g = torch.Generator().manual_seed(0)
    h = (2 * torch.randn(3, 5, 32, generator=g, dtype=torch.float64)
         ).requires_grad_(True)
    da = torch.randn(3, 5, 16, generator=g, dtype=torch.float64)
    a = swiglu(h, 0.5, False)  # not training: no dropout
    gate, val = h.detach()[..., :16], h.detach()[..., 16:]
    torch.testing.assert_close(a, gate / (1 + torch.exp(-gate)) * val,
                               rtol=1e-13, atol=1e-13)
    (dh,) = torch.autograd.grad(a, h, da)
    dg, du = swiglu_bwd_reference(da, h.detach())
    torch.testing.assert_close(dh, torch.cat([dg, du], -1), rtol=1e-12,
                               atol=1e-12)
    torch.manual_seed(1)
    dropped = swiglu(h, 0.5, True)
    torch.manual_seed(1)
    assert torch.equal(dropped, F.dropout(a, 0.5, True))


# ---- vitfsdp::swiglu_bwd under TunedGemmMode ---------------------------------

B, T, D, H = 2, 4, 8, 16


class _Swiglu(torch.autograd.Function):
    """The backward issues the registered op, as ops.swiglu._SwigluFn does
    on the GPU."""

    @staticmethod
    def forward(ctx, h):
        ctx.save_for_backward(h)
        return F.silu(h[..., :H]) * h[..., H:]

    @staticmethod
    def backward(ctx, da):
        return torch.ops.vitfsdp.swiglu_bwd(
            da.contiguous(), ctx.saved_tensors[0], 0.0, 0)


def _run(monkeypatch, switch, min_elems=-1):
    monkeypatch.setenv("VITFSDP_FUSED_DGELU_DBIAS", switch)
    monkeypatch.delenv("VITFSDP_TN_WGRAD", raising=False)
    monkeypatch.delenv("VITFSDP_TN_DGELU_T", raising=False)
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", min_elems)
    monkeypatch.setitem(linmod._SWIGLU_CFG, "d", D)
    log = []

    def dswiglu(da, h, p, seed):
        log.append(("dswiglu", tuple(da.shape), tuple(h.shape), p, seed))
        dh = torch.cat(swiglu_bwd_reference(da, h), -1).to(h.dtype)
        return dh, dh.reshape(-1, 2 * H).sum(0)

    def gemm(a, b, idx, bias):
        log.append(("gemm", a))
        return torch.mm(a, b)

    def transpose(t, want_colsum):
        log.append(("transpose", tuple(t.shape), want_colsum))
        return t.t().contiguous(), (t.sum(0) if want_colsum else None)

    g = torch.Generator().manual_seed(0)
    x, w1, b1, w2, b2 = (
        torch.randn(*s, generator=g, requires_grad=True)
        for s in ((B, T, D), (2 * H, D), (2 * H,), (D, H), (D,)))
    kw = dict(handler=gemm, tn_handler=transpose) if min_elems >= 0 else {}
    with linmod.TunedGemmMode(table={}, native_wgrad=False,
                              dswiglu_handler=dswiglu, **kw) as m:
        y = F.linear(_Swiglu.apply(F.linear(x, w1, b1)), w2, b2)
        y.pow(2).sum().backward()
        assert m._dgelu_stash is None
    return m, log, [t.grad for t in (x, w1, b1, w2, b2)]


def test_mode_routes_the_op_and_answers_the_bias_sum(monkeypatch):
    m, log, on = _run(monkeypatch, "1")
    assert log == [("dswiglu", (B, T, H), (B, T, 2 * H), 0.0, 0)]
    assert m.dswiglu_hits == 1 and m.dbias_hits == 1  # fc1's sum, not fc2's
    m, log, off = _run(monkeypatch, "0")
    assert not m.fused_dswiglu and log == []
    assert m.dswiglu_hits == 0 and m.dbias_hits == 0
    for u, v in zip(on, off):
        torch.testing.assert_close(u, v, rtol=1e-5, atol=1e-5)
    # the TN route gets dh^T [2H, rows] from the stash: fc1's dy is not
    # transposed by a pass of its own
    m, log, tn = _run(monkeypatch, "1", min_elems=0)
    assert m.dswiglu_hits == 1 and m.dbias_hits == 1 and m.tn_hits == 2
    assert ("transpose", (B * T, 2 * H), False) not in log
    assert ("transpose", (B * T, 2 * H), True) not in log
    a = [e[1] for e in log if e[0] == "gemm" and e[1].shape == (2 * H, B * T)]
    assert len(a) == 1 and a[0].is_contiguous()
    torch.testing.assert_close(a[0].sum(1), off[2], rtol=1e-5, atol=1e-5)
    for u, v in zip(tn, off):
        torch.testing.assert_close(u, v, rtol=1e-5, atol=1e-5)
