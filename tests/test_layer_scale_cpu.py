"""--layer_scale_init away from the GPU: the flag, the parameters it adds
and only when it is on, timm's formula in both block interfaces, and the
op layer's composition route with its gradients."""

import pytest
import torch
import torch.nn.functional as F

from vit_10b_fsdp_example_amd.cli import parse_args
from vit_10b_fsdp_example_amd.models import (
    Block, FSDPViTModel, count_vit_params,
)
from vit_10b_fsdp_example_amd.ops import (
    drop_path, hidden_dropout, layer_scale, layer_scale_add,
)


def test_flag_and_param_count():
    assert parse_args([]).layer_scale_init == 0.0
    assert parse_args(["--layer_scale_init", "1e-5"]).layer_scale_init == 1e-5
    with pytest.raises(SystemExit):
        parse_args(["--layer_scale_init", "-0.1"])
    with pytest.raises(ValueError):
        Block(48, 3, layer_scale_init=-1.0)
    model = FSDPViTModel(
        image_size=32, patch_size=4, embed_dim=64, num_heads=4, num_blocks=3,
        mlp_ratio=4.0, pos_dropout=0.0, mlp_dropout=0.0, att_dropout=0.0,
        num_classes=10, grad_ckpt_wrap=lambda m: m, fsdp_wrap=lambda m: m,
        layer_scale_init=1e-2)
    sd = model.state_dict()
    for key in ("ls1.gamma", "ls2.gamma"):  # initialised to the value
        assert torch.equal(sd[f"blocks.2.{key}"], torch.full((64,), 1e-2))
    n = sum(p.numel() for p in model.parameters())
    assert n == count_vit_params(32, 4, 64, 3, 4.0, 10, layer_scale=True)
    assert n == count_vit_params(32, 4, 64, 3, 4.0, 10) + 3 * 2 * 64


@pytest.mark.parametrize("deferred", [False, True])
def test_block_off_is_todays_and_on_is_timms_formula(deferred):
    def build(**kw):
        torch.manual_seed(0)
        return Block(48, 3, deferred_residual=deferred, **kw)

    def run(blk, x):
        torch.manual_seed(1)
        out = blk(x)
        return out[0] + out[1] if deferred else out

    x = torch.randn(4, 7, 48)
    today = build(drop=0.1, drop_path=0.2)
    off = build(drop=0.1, drop_path=0.2, layer_scale_init=0.0)
    assert list(off.state_dict()) == list(today.state_dict())
    assert torch.equal(run(off, x), run(today, x))

    blk = build(layer_scale_init=0.1)
    with torch.no_grad():
        blk.ls1.gamma.mul_(1.0 + torch.rand(48))
        blk.ls2.gamma.mul_(1.0 + torch.rand(48))
    ln = lambda t, n: F.layer_norm(t, (48,), n.weight, n.bias, 1e-6)  # noqa: E731
    s1 = x + blk.ls1.gamma * blk.attn(ln(x, blk.norm1))
    h = F.gelu(blk.mlp.fc1(ln(s1, blk.norm2)))
    ref = s1 + blk.ls2.gamma * blk.mlp.fc2(h)
    torch.testing.assert_close(run(blk, x), ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("training", [False, True])
def test_cpu_route_is_the_composition(training):
    torch.manual_seed(0)
    x, res, gamma = torch.randn(4, 5, 16), torch.randn(4, 5, 16), torch.rand(16)

    def comp(t):
        return drop_path(hidden_dropout(t, 0.25, training) * gamma, 0.5,
                         training)

    torch.manual_seed(3)
    a = layer_scale(x, gamma, training, p_path=0.5, p_elem=0.25)
    b = layer_scale_add(x, res, gamma, training, p_path=0.5, p_elem=0.25)
    torch.manual_seed(3)
    assert torch.equal(a, comp(x)) and torch.equal(b, x + comp(res))
    with pytest.raises(ValueError):
        layer_scale(x, gamma, True, p_path=1.0)


def test_gradcheck():
    torch.manual_seed(0)
    x, res, gamma = (torch.rand(s, dtype=torch.float64, requires_grad=True)
                     for s in ((2, 3, 8), (2, 3, 8), (8,)))
    assert torch.autograd.gradcheck(
        lambda t, g: layer_scale(t, g, True), (x, gamma))
    assert torch.autograd.gradcheck(
        lambda t, r, g: layer_scale_add(t, r, g, True), (x, res, gamma))
