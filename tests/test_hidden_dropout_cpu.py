"""ops/dropout.py on the CPU: off the native path the public functions
are exactly the nn.Dropout / F.gelu composition (values and RNG
consumption), the hash mask has the statistics of a Bernoulli mask, and
the model wiring changes neither state_dict keys nor CPU results."""

import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from vit_10b_fsdp_example_amd.models.vit import Block, FSDPViTModel
from vit_10b_fsdp_example_amd.ops import (
    HiddenDropout, dropout_add, fused_add_layer_norm, gelu_dropout,
    hidden_dropout, hidden_dropout_mask,
)

PS = [0.0, 0.1, 1.0]


def _run(fn, seed=99):
    torch.manual_seed(seed)
    out = fn()
    return out, torch.get_rng_state()


def _same(a, b):
    """bit-for-bit, NaN-safe (p = 1 gives 0 * inf nowhere, but keep the
    comparison exact rather than value-based)"""
    assert a.dtype == b.dtype and a.shape == b.shape
    if a.dtype == torch.bfloat16:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("p", PS)
def test_cpu_equals_stock_composition_and_rng(p, training, dtype):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, 7, 24, generator=g).to(dtype)
    res = torch.randn(6, 7, 24, generator=g).to(dtype)
    stock_drop = nn.Dropout(p).train(training)
    mod = HiddenDropout(p).train(training)

    pairs = [
        (lambda: hidden_dropout(x, p, training), lambda: stock_drop(x)),
        (lambda: mod(x), lambda: stock_drop(x)),
        (lambda: dropout_add(x, res, p, training),
         lambda: x + stock_drop(res)),
        (lambda: gelu_dropout(x, p, training),
         lambda: stock_drop(F.gelu(x))),
    ]
    for ours, stock in pairs:
        a, state_a = _run(ours)
        b, state_b = _run(stock)
        assert _same(a, b)
        assert torch.equal(state_a, state_b)


def test_hidden_dropout_module_is_a_dropin():
    m = HiddenDropout(0.25)
    assert repr(m).replace("HiddenDropout", "Dropout") == repr(nn.Dropout(0.25))
    assert len(m.state_dict()) == 0 and not list(m.parameters())
    with pytest.raises(ValueError):
        HiddenDropout(1.5)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_statistics(p):
    rows, cols = 257, 2048
    keep = hidden_dropout_mask(1234, rows, cols, p)
    assert keep.shape == (rows, cols) and keep.dtype == torch.bool
    k = keep.double()

    def sigmas(rate, n):
        return abs(rate - (1.0 - p)) / math.sqrt(p * (1.0 - p) / n)

    overall = sigmas(k.mean().item(), rows * cols)
    per_row = max(sigmas(v, cols) for v in k.mean(1).tolist())
    per_col = max(sigmas(v, rows) for v in k.mean(0).tolist())
    print(f"p={p}: overall {overall:.2f} sigma, rows {per_row:.2f}, "
          f"cols {per_col:.2f}")
    assert overall <= 4.0
    assert per_row <= 5.0
    assert per_col <= 5.0


def _model(drop):
    return FSDPViTModel(
        image_size=16, patch_size=4, embed_dim=32, num_heads=2, num_blocks=2,
        mlp_ratio=4.0, pos_dropout=drop, mlp_dropout=drop, att_dropout=0.0,
        num_classes=5, grad_ckpt_wrap=lambda m: m, fsdp_wrap=lambda m: m,
    )


def test_state_dict_keys_do_not_depend_on_dropout():
    assert list(_model(0.3).state_dict()) == list(_model(0.0).state_dict())


def _stock_block_forward(blk, x, drop):
    """The block as it was wired before ops/dropout.py: literal
    nn.Dropout modules at the three sites."""
    proj_drop, mlp_drop = nn.Dropout(drop), nn.Dropout(drop)
    a = blk.attn
    B, T, E = x.shape
    y = blk.norm1(x)
    qkv = a.qkv(y).reshape(B, T, 3, a.num_heads, a.head_dim)
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    probs = torch.softmax(
        (torch.matmul(q, k.transpose(-2, -1)) * a.scale).float(), dim=-1
    ).to(q.dtype)
    o = torch.matmul(probs, v).transpose(1, 2).reshape(B, T, E)
    attn_out = proj_drop(a.proj(o))
    x, normed = fused_add_layer_norm(
        x, attn_out, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps
    )
    h = mlp_drop(F.gelu(blk.mlp.fc1(normed)))
    return x + mlp_drop(blk.mlp.fc2(h))


@pytest.mark.parametrize("deferred", [False, True])
def test_block_cpu_equals_literal_nn_dropout(deferred):
    torch.manual_seed(0)
    blk = Block(32, 2, drop=0.2, deferred_residual=deferred).train()
    x = torch.randn(2, 9, 32)
    torch.manual_seed(11)
    out = blk(x)
    if deferred:  # (branch, stream): the pending add is the next norm's
        out = out[1] + out[0]
    state = torch.get_rng_state()
    torch.manual_seed(11)
    ref = _stock_block_forward(blk, x, 0.2)
    assert torch.equal(out, ref)
    assert torch.equal(state, torch.get_rng_state())
    # dropout really is active at these sites
    assert not torch.equal(out, blk.eval()(x) if not deferred
                           else sum(blk.eval()(x)))
