"""--qk_norm_type away from the GPU: the flag, the parameters of the RMS
form, and the composition it stands for against fp64."""

import pytest
import torch

from vit_10b_fsdp_example_amd.cli import parse_args
from vit_10b_fsdp_example_amd.models import FSDPViTModel, count_vit_params
from vit_10b_fsdp_example_amd.ops import LayerNorm, RMSNorm, attention_qkv


def _model(**kw):
    return FSDPViTModel(
        image_size=32, patch_size=4, embed_dim=64, num_heads=4, num_blocks=3,
        mlp_ratio=4.0, pos_dropout=0.0, mlp_dropout=0.0, att_dropout=0.0,
        num_classes=10, grad_ckpt_wrap=lambda m: m, fsdp_wrap=lambda m: m,
        **kw)


def test_flag():
    assert parse_args([]).qk_norm_type == "layernorm"
    assert parse_args(["--qk_norm"]).qk_norm_type == "layernorm"
    cfg = parse_args(["--qk_norm", "--qk_norm_type", "rmsnorm"])
    assert cfg.qk_norm is True and cfg.qk_norm_type == "rmsnorm"
    for argv in (["--qk_norm_type", "rmsnorm"],
                 ["--qk_norm", "--qk_norm_type", "batchnorm"]):
        with pytest.raises(SystemExit):
            parse_args(argv)


def test_rms_form_has_two_weights_per_block_and_no_bias():
    model = _model(qk_norm=True, qk_norm_type="rmsnorm")
    sd = model.state_dict()
    for i in range(3):
        for name in ("q_norm", "k_norm"):
            assert torch.equal(sd[f"blocks.{i}.attn.{name}.weight"],
                               torch.ones(16))
            assert f"blocks.{i}.attn.{name}.bias" not in sd
    for blk in model.blocks:
        for norm in (blk.attn.q_norm, blk.attn.k_norm):
            assert isinstance(norm, RMSNorm) and norm.eps == 1e-6
    count = sum(p.numel() for p in model.parameters())
    assert count == count_vit_params(32, 4, 64, 3, 4.0, 10, num_heads=4,
                                     qk_norm=True, qk_norm_type="rmsnorm")
    assert count == count_vit_params(32, 4, 64, 3, 4.0, 10) + 3 * 2 * 16


def test_norm_type_does_not_choose_the_qk_norm():
    cfg = parse_args(["--norm_type", "rmsnorm", "--qk_norm"])
    model = _model(qk_norm=cfg.qk_norm, norm_type=cfg.norm_type,
                   qk_norm_type=cfg.qk_norm_type)
    for blk in model.blocks:
        assert isinstance(blk.norm1, RMSNorm)
        assert isinstance(blk.attn.q_norm, LayerNorm)
        assert isinstance(blk.attn.k_norm, LayerNorm)


def test_composition_against_fp64():
    B, T, H, D = 2, 7, 3, 16
    torch.manual_seed(0)
    qkv = torch.randn(B, T, 3, H, D, requires_grad=True)
    wq = (1 + 0.5 * torch.randn(D)).requires_grad_(True)
    wk = (1 + 0.5 * torch.randn(D)).requires_grad_(True)
    do = torch.randn(B, T, H * D)
    leaves = [qkv, wq, wk]
    o = attention_qkv(qkv, H, qk_norm=(wq, None, wk, None, 1e-6))
    got = (o,) + torch.autograd.grad(o, leaves, do)

    leaves64 = [t.detach().double().requires_grad_(True) for t in leaves]
    q, k, v = (leaves64[0][:, :, i].transpose(1, 2) for i in range(3))

    def rms(t, w):
        return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-6) * w

    s = rms(q, leaves64[1]) @ rms(k, leaves64[2]).transpose(-2, -1) * D ** -0.5
    ref_o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, H * D)
    want = (ref_o,) + torch.autograd.grad(ref_o, leaves64, do.double())
    # fp32 (2^-24 per operation) through a few dozen operations and sums of
    # at most 16 terms, on values of order 1 to 10
    for a, b in zip(got, want):
        torch.testing.assert_close(a.double(), b, rtol=1e-4, atol=1e-5)
