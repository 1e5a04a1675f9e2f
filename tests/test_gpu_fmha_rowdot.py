"""Attention-backward row dot Delta = rowsum(dO * O) (csrc/fmha.hip
fmha_rowdot_kernel: 16-byte loads, 8 lanes per row) directly, through
both backward entry points, and on the scalar path that operands with a
misaligned base address must take."""

import numpy as np
import pytest
import torch

from tests.fmha_reference import check_kernel_outputs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None


def _dev():
    return torch.device("cuda", 0)


def _check_rowdot(delta, dout, o):
    terms = dout.double() * o.double()
    ref = terms.sum(-1)
    # fp32 accumulation over at most 192 exactly-representable products
    tol = 1e-5 * terms.abs().sum(-1)
    assert delta.dtype == torch.float32 and delta.shape == ref.shape
    err = (delta.double() - ref).abs()
    print(f"rowdot: max err {err.max().item():.3e}, min slack "
          f"{(tol - err).min().item():.3e}")
    assert bool((err <= tol).all()), (err - tol).max().item()


@pytest.mark.parametrize(
    "B,H,T,D",
    [
        (1, 2, 80, 48),    # 6 vectors: lanes 6, 7 of a group idle
        (1, 1, 40, 176),   # 22 vectors: a ragged third load
        (2, 4, 256, 160),  # ViT-10B head shape, several blocks
        (1, 3, 7, 16),     # 21 rows: fewer than one block iteration
        (1, 1, 1, 192),    # one row, the widest head
    ],
)
def test_rowdot_vs_reference(B, H, T, D):
    torch.manual_seed(0)
    dout = torch.randn(B, H, T, D, device=_dev(), dtype=torch.bfloat16)
    o = torch.randn(B, H, T, D, device=_dev(), dtype=torch.bfloat16)
    _check_rowdot(EXT.fmha_rowdot(dout, o), dout, o)


def test_rowdot_misaligned_takes_scalar_path():
    """A contiguous view that starts 8 bytes into its buffer cannot use
    16-byte loads; the scalar kernel must give the same Delta, bit for
    bit (the vector kernel keeps the scalar kernel's summation order)."""
    torch.manual_seed(1)
    B, H, T, D = 2, 4, 256, 160
    n = B * H * T * D
    buf_a = torch.randn(n + 4, device=_dev(), dtype=torch.bfloat16)
    buf_b = torch.randn(n + 4, device=_dev(), dtype=torch.bfloat16)
    dout, o = buf_a[4:].view(B, H, T, D), buf_b[4:].view(B, H, T, D)
    assert dout.is_contiguous() and dout.data_ptr() % 16 == 8
    delta = EXT.fmha_rowdot(dout, o)
    _check_rowdot(delta, dout, o)
    aligned = EXT.fmha_rowdot(dout.clone(), o.clone())
    assert torch.equal(delta, aligned)


def _attention_ref(q, k, v, do, scale):
    qf = q.float().requires_grad_(True)
    kf = k.float().requires_grad_(True)
    vf = v.float().requires_grad_(True)
    s = (qf @ kf.transpose(-2, -1)) * scale
    (torch.softmax(s, dim=-1) @ vf).backward(do.float())
    return qf.grad, kf.grad, vf.grad


@pytest.mark.parametrize("B,H,T,D", [(1, 2, 80, 48), (2, 4, 256, 160)])
def test_fmha_bwd_with_new_rowdot(B, H, T, D):
    torch.manual_seed(2)
    q, k, v, do = (torch.randn(B, H, T, D, device=_dev(), dtype=torch.bfloat16)
                   for _ in range(4))
    scale = D ** -0.5
    o, lse = EXT.fmha_fwd(q, k, v, scale)
    dq, dk, dv = EXT.fmha_bwd(do, q, k, v, o, lse, scale)
    rq, rk, rv = _attention_ref(q, k, v, do, scale)
    for got, ref in ((dv, rv), (dq, rq), (dk, rk)):
        np.testing.assert_allclose(got.float().cpu().numpy(),
                                   ref.cpu().numpy(), rtol=0.1, atol=0.06)
    check_kernel_outputs(
        q, k, v, do, scale,
        {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv},
        f"rowdot-bwd/T{T}/D{D}")


@pytest.mark.parametrize("B,H,T,D", [(1, 2, 80, 48), (2, 4, 256, 160)])
def test_fmha_bwd_qkv_with_new_rowdot(B, H, T, D):
    """Fused-qkv layout: o/dO are [B, T, H*D], so the head stride is the
    smaller one and the kernel walks rows h-fastest."""
    torch.manual_seed(3)
    qkv = torch.randn(B, T, 3, H, D, device=_dev(), dtype=torch.bfloat16)
    do = torch.randn(B, T, H * D, device=_dev(), dtype=torch.bfloat16)
    scale = D ** -0.5
    o, lse = EXT.fmha_fwd_qkv(qkv, H, scale)
    dqkv = EXT.fmha_bwd_qkv(do, qkv, o, lse, H, scale)

    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)  # [B, H, T, D] views
    do_bhtd = do.view(B, T, H, D).transpose(1, 2)
    rq, rk, rv = _attention_ref(q, k, v, do_bhtd, scale)
    ref = torch.stack([rq, rk, rv], 0).permute(1, 3, 0, 2, 4)  # [B,T,3,H,D]
    np.testing.assert_allclose(dqkv.float().cpu().numpy(), ref.cpu().numpy(),
                               rtol=0.1, atol=0.06)
    dq, dk, dv = dqkv.permute(2, 0, 3, 1, 4).unbind(0)
    check_kernel_outputs(
        q, k, v, do_bhtd, scale,
        {"o": o.view(B, T, H, D).transpose(1, 2), "lse": lse, "dq": dq,
         "dk": dk, "dv": dv}, f"rowdot-bwd-qkv/T{T}/D{D}")
