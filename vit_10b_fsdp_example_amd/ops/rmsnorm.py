"""RMSNorm over the last dimension (--norm_type rmsnorm) on csrc/rmsnorm.hip.

    y = x * rsqrt(mean(x^2 over D) + eps) * weight

No mean subtraction and no bias (timm's RmsNorm; the parameter is
`weight`).  On GPU with bf16 x and weight, D % 8 == 0 and D <= 8192 the
forward and backward are the register-resident HIP kernels, which read
every input once and save x (or the sum), weight and one fp32 rstd per
row.  Everything else (CPU, fp32, an fp32 weight next to a bf16 x, wider
rows) takes the explicit composition below: statistic and product in
fp32, cast once to x.dtype.  VITFSDP_NATIVE_RMSNORM=0 forces the
composition on GPU for A/B runs and bisection.
"""

import os

import torch
import torch.nn as nn

from ._extension import ext, use_hip

MAX_KERNEL_DIM = 8192


def _native_rmsnorm_on():
    return os.environ.get("VITFSDP_NATIVE_RMSNORM", "1") != "0"


def _kernel_operands(x, weight):
    """What the HIP kernels serve; they refuse anything else, and must
    never reinterpret it."""
    return (
        x.dtype == torch.bfloat16
        and x.dim() >= 1
        and 0 < x.shape[-1] <= MAX_KERNEL_DIM
        and x.shape[-1] % 8 == 0
        and weight.dtype == torch.bfloat16
        and _native_rmsnorm_on()
    )


def _composition(x, weight, eps):
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * rstd * weight.float()).to(x.dtype)


class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        y, rstd = ext().rmsnorm_fwd(x, weight, eps)
        ctx.save_for_backward(x, weight, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, rstd = ctx.saved_tensors
        dx, dw = ext().rmsnorm_bwd(dy.contiguous(), x, weight, rstd)
        return dx, dw, None


def rms_norm(x, weight, eps=1e-6):
    if _kernel_operands(x, weight) and use_hip(x, weight):
        return _RMSNormFn.apply(x.contiguous(), weight.contiguous(), eps)
    return _composition(x, weight, eps)


class _FusedAddRMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, weight, eps):
        s, y, rstd = ext().rmsnorm_add_fwd(x, res, weight, eps)
        ctx.save_for_backward(s, weight, rstd)
        return s, y

    @staticmethod
    def backward(ctx, dsum, dy):
        s, weight, rstd = ctx.saved_tensors
        if dsum is None:
            dsum = torch.zeros_like(dy)
        dx1, dx2, dw = ext().rmsnorm_add_bwd(
            dy.contiguous(), dsum.contiguous(), s, weight, rstd
        )
        return dx1, dx2, dw, None


def fused_add_rms_norm(x, res, weight, eps=1e-6):
    """s = x + res and y = rms_norm(s) in one fused pass; returns (s, y).
    s is rounded to the input dtype exactly as torch's add rounds it, and
    the backward folds the gradient of s into the dx pass."""
    if (
        _kernel_operands(x, weight)
        and res.dtype == torch.bfloat16
        and res.shape == x.shape
        and use_hip(x, res, weight)
    ):
        return _FusedAddRMSNormFn.apply(
            x.contiguous(), res.contiguous(), weight.contiguous(), eps
        )
    s = x + res
    return s, _composition(s, weight, eps)


class RMSNorm(nn.Module):
    """RMSNorm module backed by the HIP kernels on GPU; `weight` only."""

    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.eps = eps
        self.dim = dim

    def forward(self, x):
        return rms_norm(x, self.weight, self.eps)

    def extra_repr(self):
        return f"{self.dim}, eps={self.eps}"
