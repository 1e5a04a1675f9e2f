"""Hidden dropout (--mlp_dropout, --pos_dropout) with the mask generated
in the kernel (csrc/dropout.hip).

The mask is the stateless (seed, row, col) hash the attention kernels
use: the backward regenerates it from one integer seed, so no mask is
stored (a bool mask is 671 MB at the ViT-10B GELU site) and the
checkpoint recompute reproduces it from the CPU generator alone.  Three
fused sites:

  hidden_dropout(x)        pos-embed, attention projection, deferred MLP
  dropout_add(x, res)      x + dropout(res): the MLP residual add
  gelu_dropout(x)          dropout(gelu(x)) after fc1; saves only x

Routing: the native path needs training, 0 < p < 1, bf16, a last dim
that is a multiple of 8 and GPU tensors; VITFSDP_NATIVE_DROPOUT=0 turns
it off.  In every other case the functions run exactly the stock
composition (F.dropout / F.gelu), so CPU results and RNG consumption are
those of nn.Dropout, and with p == 0 aten.gelu / aten.gelu_backward are
still issued for the TunedGemmMode intercepts in ops/linear.py.

The backward of gelu_dropout is issued as the registered op
vitfsdp::gelu_dropout_bwd (schema in ops/linear.py, implementations
here: _C.gelu_dropout_bwd on the GPU, plain torch elsewhere).  With no
dispatch mode active that is the kernel call it replaced; under
TunedGemmMode the op is answered by _C.gelu_dropout_bwd_colsum, which
writes the same dx together with fc1's bias gradient, as the p == 0
path does through aten.gelu_backward (the variant that also writes dx^T
for fc1's TN weight gradient is not routed: _DGELU_DROP_T in
ops/linear.py).
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._extension import ext, use_hip
from .attention import _draw_seed, dropout_mask_reference
from . import linear as _linear
from .linear import _gelu_fusion_on


def _native_dropout_on():
    return os.environ.get("VITFSDP_NATIVE_DROPOUT", "1") != "0"


def _use_native(p, training, *tensors):
    x = tensors[0]
    return (
        training
        and 0.0 < p < 1.0
        and all(
            t.dtype == torch.bfloat16 and t.shape == x.shape for t in tensors
        )
        and x.dim() >= 1
        and x.shape[-1] > 0
        and x.shape[-1] % 8 == 0
        and use_hip(*tensors)
        and all(t.is_cuda for t in tensors)
        and _native_dropout_on()
    )


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        ctx.p, ctx.seed = p, seed
        return ext().dropout_fwd(x.contiguous(), p, seed)

    @staticmethod
    def backward(ctx, dy):
        # dropout is its own adjoint: the same mask and scale on dy
        return ext().dropout_fwd(dy.contiguous(), ctx.p, ctx.seed), None, None


class _DropoutAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, p, seed):
        ctx.p, ctx.seed = p, seed
        return ext().dropout_add_fwd(x.contiguous(), res.contiguous(), p, seed)

    @staticmethod
    def backward(ctx, dout):
        dres = None
        if ctx.needs_input_grad[1]:
            dres = ext().dropout_fwd(dout.contiguous(), ctx.p, ctx.seed)
        return dout, dres, None, None


class _GeluDropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        x = x.contiguous()
        # only the pre-activation is kept: neither gelu(x) nor a mask
        ctx.save_for_backward(x)
        ctx.p, ctx.seed = p, seed
        return ext().gelu_dropout_fwd(x, p, seed)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        # as a registered op, so that TunedGemmMode can answer it with
        # the kernel that also makes fc1's bias gradient and dx^T
        dx = torch.ops.vitfsdp.gelu_dropout_bwd(
            dy.contiguous(), x, ctx.p, ctx.seed)
        return dx, None, None


def _seed(seed):
    # one CPU-generator integer per call (attention._draw_seed):
    # torch.manual_seed and the checkpoint wrapper's preserve_rng_state
    # reproduce it, no device RNG involved
    return _draw_seed() if seed is None else int(seed)


def hidden_dropout(x, p, training, seed=None):
    """F.dropout(x, p, training); in-kernel hash mask on GPU bf16."""
    if _use_native(p, training, x):
        return _DropoutFn.apply(x, float(p), _seed(seed))
    return F.dropout(x, p, training)


def dropout_add(x, res, p, training, seed=None):
    """x + F.dropout(res, p, training); one fused pass on GPU bf16."""
    if _use_native(p, training, x, res):
        return _DropoutAddFn.apply(x, res, float(p), _seed(seed))
    return x + F.dropout(res, p, training)


def gelu_dropout(x, p, training, seed=None):
    """F.dropout(F.gelu(x), p, training); one fused pass each way on GPU
    bf16, keeping only x for the backward."""
    # with the fused fc1 epilogue on, the dispatch mode has cached a
    # GELU output that only an aten.gelu consumes: issue it
    if not _gelu_fusion_on() and _use_native(p, training, x):
        return _GeluDropoutFn.apply(x, float(p), _seed(seed))
    return F.dropout(F.gelu(x), p, training)


class HiddenDropout(nn.Module):
    """Drop-in for nn.Dropout (no parameters, no state-dict entries)
    that routes through hidden_dropout."""

    def __init__(self, p=0.5):
        super().__init__()
        if p < 0 or p > 1:
            raise ValueError(
                f"dropout probability has to be between 0 and 1, but got {p}"
            )
        self.p = p

    def forward(self, x):
        return hidden_dropout(x, self.p, self.training)

    def extra_repr(self):
        return f"p={self.p}, inplace=False"


# ---- references for the tests --------------------------------------------


def hidden_dropout_mask(seed, rows, cols, p):
    """Keep mask [rows, cols] (bool, CPU) of the hidden-dropout kernels:
    element (r, c) is kept iff dropout_hash(seed, r, c) >= p * 2^32."""
    return dropout_mask_reference(
        seed, torch.arange(rows), torch.arange(cols), p
    )


def _mask_and_scale(x, p, seed):
    cols = x.shape[-1]
    mask = hidden_dropout_mask(seed, x.numel() // cols, cols, p)
    return mask.reshape(x.shape).to(x.device), 1.0 / (1.0 - p)


def _gelu_dropout_bwd_gpu(dy, x, p, seed):
    return ext().gelu_dropout_bwd(dy, x, p, seed)


def _gelu_dropout_bwd_torch(dy, x, p, seed):
    """vitfsdp::gelu_dropout_bwd away from the GPU, in plain torch (the
    native forward never runs there; this serves CPU tests of the
    routing)."""
    mask, rscale = _mask_and_scale(x, p, seed)
    dx = torch.ops.aten.gelu_backward(dy * rscale, x, approximate="none")
    return torch.where(mask, dx, torch.zeros_like(dx))


# the schema is in ops/linear.py, next to the dispatch mode that routes it
_linear._LIB.impl("gelu_dropout_bwd", _gelu_dropout_bwd_gpu, "CUDA")
_linear._LIB.impl("gelu_dropout_bwd", _gelu_dropout_bwd_torch,
                  "CompositeExplicitAutograd")


def hidden_dropout_reference(x, p, seed):
    """fp64 keep ? x / (1 - p) : 0 under the hash mask."""
    mask, rscale = _mask_and_scale(x, p, seed)
    x64 = x.double()
    return torch.where(mask, x64 * rscale, torch.zeros_like(x64))


def dropout_add_reference(x, res, p, seed):
    """fp64 x + (keep ? res / (1 - p) : 0)."""
    return x.double() + hidden_dropout_reference(res, p, seed)


def gelu_dropout_reference(x, p, seed):
    """fp64 keep ? gelu_erf(x) / (1 - p) : 0."""
    mask, rscale = _mask_and_scale(x, p, seed)
    x64 = x.double()
    g = 0.5 * x64 * (1.0 + torch.erf(x64 * 0.7071067811865476))
    return torch.where(mask, g * rscale, torch.zeros_like(g))
