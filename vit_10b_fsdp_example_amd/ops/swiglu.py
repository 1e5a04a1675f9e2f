"""SwiGLU for the gated MLP (--mlp_type swiglu) on csrc/swiglu.hip.

    h = fc1(x)                          [.., 2H], gate half first
    a = dropout(silu(h[..., :H]) * h[..., H:], p)

On GPU bf16 with H % 8 == 0 the forward is one kernel (_C.swiglu_fwd, the
dropout mask the (seed, row, col) hash of ops/dropout.py) inside an
autograd Function that keeps only h: neither silu(g), the product nor a
mask is saved.  Its backward is issued as the registered op
vitfsdp::swiglu_bwd (schema in ops/linear.py, implementations here:
_C.swiglu_bwd_colsum with the sums dropped on the GPU, plain torch
elsewhere), so that TunedGemmMode can answer it with the kernel call that
also parks fc1's bias gradient and, for the TN weight gradient, dh^T.
VITFSDP_NATIVE_SWIGLU=0 turns the native path off; that, the CPU and every
other dtype or layout run the stock composition.

swiglu_fc2_recompute is mlp_fc2_recompute_act for this MLP: fc2's saved
input becomes a handle on h and is rebuilt in the backward, as a^T by
_C.swiglu_fwd_t where fc2's weight gradient takes the TN route.
"""

import os

import torch
import torch.nn.functional as F

from ._extension import ext, use_hip
from . import linear as _linear
from .dropout import _mask_and_scale, _seed


def swiglu_hidden_dim(embed_dim, mlp_ratio):
    """H of the gated MLP: two thirds of the GELU MLP's hidden width, so
    that the parameter count stays near it, rounded up to a multiple of
    256, so that both GEMM dimensions stay tile-aligned."""
    return -(-(int(embed_dim * mlp_ratio) * 2) // (3 * 256)) * 256


def _native_swiglu_on():
    return os.environ.get("VITFSDP_NATIVE_SWIGLU", "1") != "0"


def _use_native(h, p):
    return (
        h.is_cuda
        and h.dtype == torch.bfloat16
        and h.dim() >= 1
        and h.shape[-1] > 0
        and h.shape[-1] % 16 == 0  # H % 8 == 0
        and 0.0 <= p < 1.0
        and h.is_contiguous()
        and h.data_ptr() % 16 == 0
        and _native_swiglu_on()
        and use_hip(h)
    )


def _composition(h, p, training):
    hid = h.shape[-1] // 2
    return F.dropout(F.silu(h[..., :hid]) * h[..., hid:], p, training)


class _SwigluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, p, seed):
        # only the pre-activation is kept
        ctx.save_for_backward(h)
        ctx.p, ctx.seed = p, seed
        return ext().swiglu_fwd(h, p, seed)

    @staticmethod
    def backward(ctx, da):
        (h,) = ctx.saved_tensors
        dh = torch.ops.vitfsdp.swiglu_bwd(da.contiguous(), h, ctx.p, ctx.seed)
        return dh, None, None


def swiglu(h, p, training, seed=None):
    """F.dropout(F.silu(h[..., :H]) * h[..., H:], p, training) for
    h [.., 2H]; one fused pass each way on GPU bf16, keeping only h."""
    p = float(p) if training else 0.0
    if _use_native(h, p):
        return _SwigluFn.apply(h, p, _seed(seed) if p > 0 else 0)
    return _composition(h, p, training)


def _swiglu_value(h):
    """swiglu(h, 0, False) outside autograd."""
    if _use_native(h, 0.0):
        return ext().swiglu_fwd(h, 0.0, 0)
    return _composition(h, 0.0, False)


def _rebuild_swiglu(h, shape, d_out):
    """silu(g) * u with that shape [rows, H] for fc2's weight gradient
    [d_out, H]."""
    with torch.no_grad():
        if (_linear._rebuild_transposed(h, shape, d_out)
                and shape[1] % 8 == 0 and _native_swiglu_on()):
            return ext().swiglu_fwd_t(h.view(shape[0], 2 * shape[1])).t()
        return _swiglu_value(h).view(shape)


def swiglu_fc2_recompute(fc2, h):
    """fc2(swiglu(h)) whose graph keeps h [.., 2H] alone: the Function
    above saves it, and fc2's saved input is a handle on it."""
    return _linear.mlp_fc2_recompute_act(
        fc2, h, act_fn=lambda t: swiglu(t, 0.0, False),
        rebuild=_rebuild_swiglu)


# ---- vitfsdp::swiglu_bwd -------------------------------------------------


def _swiglu_bwd_gpu(da, h, p, seed):
    return ext().swiglu_bwd_colsum(da, h, p, seed)[0]


def swiglu_bwd_reference(da, h, p=0.0, seed=0):
    """(dg, du) of the formula, in fp64 for the 16-bit and fp32 dtypes:
    dg = da u s (1 + g (1 - s)), du = da g s with s = sigmoid(g) and da
    scaled by 1 / (1 - p) where the hash mask keeps it, zero elsewhere."""
    hid = h.shape[-1] // 2
    g, u, d = h[..., :hid].double(), h[..., hid:].double(), da.double()
    if p > 0:
        mask, rscale = _mask_and_scale(da, p, seed)
        d = torch.where(mask, d * rscale, torch.zeros_like(d))
    s = torch.sigmoid(g)
    return d * u * s * (1.0 + g * (1.0 - s)), d * g * s


def _swiglu_bwd_torch(da, h, p, seed):
    """vitfsdp::swiglu_bwd away from the GPU, in plain torch (the native
    forward never runs there; this serves CPU tests of the routing)."""
    return torch.cat(swiglu_bwd_reference(da, h, p, seed), -1).to(h.dtype)


# the schema is in ops/linear.py, next to the dispatch mode that routes it
_linear._LIB.impl("swiglu_bwd", _swiglu_bwd_gpu, "CUDA")
_linear._LIB.impl("swiglu_bwd", _swiglu_bwd_torch, "CompositeExplicitAutograd")


def swiglu_reference(h, p=0.0, seed=0):
    """fp64 keep ? silu(g) * u / (1 - p) : 0."""
    hid = h.shape[-1] // 2
    g, u = h[..., :hid].double(), h[..., hid:].double()
    a = g * torch.sigmoid(g) * u
    if p > 0:
        mask, rscale = _mask_and_scale(a, p, seed)
        a = torch.where(mask, a * rscale, torch.zeros_like(a))
    return a
