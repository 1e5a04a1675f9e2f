"""--norm_type rmsnorm away from the GPU: the composition against the
formula with its gradients, the modules and parameter counts the flag
gives, and 2-rank FSDP parity."""

import numpy as np
import pytest
import torch

from tests.test_fsdp_parity import _run_trajectory, _single_rank_reference
from tests.utils_mp import run_multiprocess
from vit_10b_fsdp_example_amd.cli import parse_args
from vit_10b_fsdp_example_amd.models import (
    Block, FSDPViTModel, count_vit_params,
)
from vit_10b_fsdp_example_amd.ops import (
    RMSNorm, fused_add_rms_norm, rms_norm,
)

EPS = 1e-6


def _model(**kw):
    torch.manual_seed(0)
    return FSDPViTModel(
        image_size=32, patch_size=4, embed_dim=64, num_heads=4, num_blocks=2,
        mlp_ratio=4.0, pos_dropout=0.0, mlp_dropout=0.0, att_dropout=0.0,
        num_classes=10, grad_ckpt_wrap=lambda m: m, fsdp_wrap=lambda m: m,
        **kw)


@pytest.mark.parametrize("add", [False, True])
def test_composition_is_the_formula_with_its_gradients(add):
    g = torch.Generator().manual_seed(0)
    x, res, dy, ds = (torch.randn(3, 5, 40, generator=g) for _ in range(4))
    w = 1 + 0.5 * torch.randn(40, generator=g)
    leaves = [t.clone().requires_grad_(True) for t in (x, res, w)]
    ref = [t.double().requires_grad_(True) for t in (x, res, w)]
    if add:
        s, y = fused_add_rms_norm(*leaves, EPS)
        s64 = ref[0] + ref[1]
    else:
        s, y, s64 = leaves[0], rms_norm(leaves[0], leaves[2], EPS), ref[0]
    y64 = s64 * torch.rsqrt(s64.pow(2).mean(-1, keepdim=True) + EPS) * ref[2]
    got = torch.autograd.grad([y, s], leaves, [dy, ds], allow_unused=True)
    want = torch.autograd.grad(
        [y64, s64], ref, [dy.double(), ds.double()], allow_unused=True)
    assert y.dtype == torch.float32
    pairs = [(y, y64), (s, s64)] + list(zip(got, want))
    for a, b in pairs:
        if b is not None:
            torch.testing.assert_close(a.double(), b, rtol=1e-5, atol=1e-6)


def test_flag_modules_and_param_count():
    assert parse_args([]).norm_type == "layernorm"
    assert parse_args(["--norm_type", "rmsnorm"]).norm_type == "rmsnorm"
    with pytest.raises(SystemExit):
        parse_args(["--norm_type", "batchnorm"])
    with pytest.raises(ValueError):
        Block(64, 4, norm_type="batchnorm")
    assert list(RMSNorm(16).state_dict()) == ["weight"]
    for qk_norm in (False, True):
        m = _model(norm_type="rmsnorm", qk_norm=qk_norm)
        keys = list(m.state_dict())
        assert "blocks.1.norm2.weight" in keys and "norm.weight" in keys
        assert not [k for k in keys if k == "norm.bias"
                    or k.endswith(("norm1.bias", "norm2.bias"))]
        assert ("blocks.0.attn.q_norm.bias" in keys) == qk_norm
        assert sum(p.numel() for p in m.parameters()) == count_vit_params(
            32, 4, 64, 2, 4.0, 10, num_heads=4, qk_norm=qk_norm,
            norm_type="rmsnorm")
    assert count_vit_params(32, 4, 64, 2, 4.0, 10) - count_vit_params(
        32, 4, 64, 2, 4.0, 10, norm_type="rmsnorm") == 5 * 64


def test_layernorm_model_keeps_its_state_dict_keys():
    per_block = [
        "norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias",
        "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias",
        "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias",
    ]
    want = (["pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"]
            + [f"blocks.{i}.{k}" for i in range(2) for k in per_block]
            + ["norm.weight", "norm.bias", "head.weight", "head.bias"])
    assert list(_model().state_dict()) == want
    assert list(_model(norm_type="layernorm").state_dict()) == want


def test_ws2_fsdp_rmsnorm_matches_single_rank():
    flag = ["--norm_type", "rmsnorm"]
    ref_l, ref_g = _single_rank_reference(flag + ["--run_without_fsdp"])
    for extra in (flag, flag + ["--fuse_residual"]):
        for l, g in run_multiprocess(_run_trajectory, world_size=2,
                                     args=(extra,)):
            np.testing.assert_allclose(l, ref_l, rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(g, ref_g, rtol=1e-4, atol=1e-5)
