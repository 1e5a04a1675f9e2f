"""--qk_norm away from the GPU: the flag, the parameters it adds and only
when it is on, the fp64 composition it stands for (with and without
gradient checkpointing), and FSDP parity of a --qk_norm trajectory."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_fsdp_parity import _run_trajectory, _single_rank_reference
from tests.utils_mp import run_multiprocess
from vit_10b_fsdp_example_amd.cli import parse_args
from vit_10b_fsdp_example_amd.models import (
    Block, FSDPViTModel, count_vit_params,
)
from vit_10b_fsdp_example_amd.parallel import checkpoint_module

def _model(**kw):
    return FSDPViTModel(
        image_size=32, patch_size=4, embed_dim=64, num_heads=4, num_blocks=3,
        mlp_ratio=4.0, pos_dropout=0.0, mlp_dropout=0.0, att_dropout=0.0,
        num_classes=10, grad_ckpt_wrap=lambda m: m, fsdp_wrap=lambda m: m,
        **kw)


def _count(model):
    return sum(p.numel() for p in model.parameters())


def test_flag_off_adds_nothing():
    assert parse_args([]).qk_norm is False
    assert parse_args(["--qk_norm"]).qk_norm is True
    today, off = _model(), _model(qk_norm=False)
    assert list(off.state_dict()) == list(today.state_dict())
    assert not any("q_norm" in k or "k_norm" in k for k in off.state_dict())
    assert _count(off) == count_vit_params(32, 4, 64, 3, 4.0, 10)


def test_flag_on_adds_four_vectors_per_block():
    on = _model(qk_norm=True)
    sd = on.state_dict()
    for i in range(3):
        for key in ("q_norm.weight", "q_norm.bias", "k_norm.weight",
                    "k_norm.bias"):
            assert sd[f"blocks.{i}.attn.{key}"].shape == (16,)
    assert len(sd) == len(_model().state_dict()) + 3 * 4
    for blk in on.blocks:
        for norm in (blk.attn.q_norm, blk.attn.k_norm):
            assert torch.equal(norm.weight, torch.ones(16))
            assert torch.equal(norm.bias, torch.zeros(16))
            assert norm.eps == 1e-6
    want = count_vit_params(32, 4, 64, 3, 4.0, 10, num_heads=4, qk_norm=True)
    assert _count(on) == want == _count(_model()) + 3 * 4 * 16


def _attention_composition(attn, x):
    """Per-head LayerNorm of q and k, then softmax attention, written out."""
    B, T, E = x.shape
    H, D = attn.num_heads, attn.head_dim
    qkv = F.linear(x, attn.qkv.weight, attn.qkv.bias).reshape(B, T, 3, H, D)
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))  # [B,H,T,D]

    def ln(t, norm):
        mu = t.mean(-1, keepdim=True)
        var = ((t - mu) ** 2).mean(-1, keepdim=True)
        return (t - mu) / torch.sqrt(var + 1e-6) * norm.weight + norm.bias

    q, k = ln(q, attn.q_norm), ln(k, attn.k_norm)
    # ops.math_attention takes the softmax in fp32 whatever the dtype; so
    # does this, and everything the flag adds is compared in full fp64
    s = q @ k.transpose(-2, -1) * D ** -0.5
    p = torch.softmax(s.float(), dim=-1).to(s.dtype)
    o = (p @ v).transpose(1, 2).reshape(B, T, E)
    return F.linear(o, attn.proj.weight, attn.proj.bias)


def _block_composition(blk, x):
    E = x.shape[-1]
    x = x + _attention_composition(
        blk.attn, F.layer_norm(x, (E,), blk.norm1.weight, blk.norm1.bias, 1e-6))
    h = F.layer_norm(x, (E,), blk.norm2.weight, blk.norm2.bias, 1e-6)
    h = F.gelu(F.linear(h, blk.mlp.fc1.weight, blk.mlp.fc1.bias))
    return x + F.linear(h, blk.mlp.fc2.weight, blk.mlp.fc2.bias)


@pytest.mark.parametrize("ckpt", [False, True])
def test_fp64_block_equals_composition(ckpt):
    torch.manual_seed(0)
    blk = Block(48, 3, qk_norm=True).double()
    with torch.no_grad():  # non-trivial gamma / beta, different for q and k
        for norm in (blk.attn.q_norm, blk.attn.k_norm):
            norm.weight.copy_(1.0 + 0.5 * torch.randn(16))
            norm.bias.copy_(torch.randn(16))
    x = torch.randn(2, 7, 48, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, 7, 48, dtype=torch.float64)
    params = list(blk.parameters())

    y = (checkpoint_module(blk) if ckpt else blk)(x)
    got = torch.autograd.grad(y, [x] + params, dy)
    ref_y = _block_composition(blk, x)
    ref = torch.autograd.grad(ref_y, [x] + params, dy)
    torch.testing.assert_close(y, ref_y, rtol=1e-11, atol=1e-12)
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-11)
    torch.testing.assert_close(blk.attn(x), _attention_composition(blk.attn, x),
                               rtol=1e-11, atol=1e-12)


def test_ws2_fsdp_matches_single_rank_with_qk_norm():
    ref_l, ref_g = _single_rank_reference(["--run_without_fsdp", "--qk_norm"])
    off_l, _ = _single_rank_reference(["--run_without_fsdp"])
    assert not np.allclose(ref_l, off_l, rtol=1e-4, atol=1e-5)
    results = run_multiprocess(_run_trajectory, world_size=2,
                               args=(["--qk_norm"],))
    for l, g in results:
        np.testing.assert_allclose(l, ref_l, rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(g, ref_g, rtol=1e-4, atol=1e-5)
