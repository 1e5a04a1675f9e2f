"""Stochastic depth (--drop_path_rate) with the per-sample mask
generated in the kernel (csrc/drop_path.hip).

A residual branch is kept per sample b of the leading batch dimension
with probability 1 - p_path and scaled by 1 / (1 - p_path) (timm's
drop_path, scale_by_keep).  Sample b is kept iff
dropout_hash(seed_path, b, 0) >= p_path * 2^32: the hidden-dropout hash
(ops/dropout.py) at column 0, so the backward and the checkpoint
recompute regenerate the mask from one CPU-generator integer and no mask
is stored.  The branch's own element dropout (p_elem) is folded into the
same pass, with exactly the mask hidden_dropout would have drawn.  Two
fused sites:

  drop_path(x)            attention branch, deferred MLP branch
  drop_path_add(x, res)   x + drop_path(res): the MLP residual add

Rows of a dropped sample are never read by the kernels.

Routing: not training, or p_path == 0, is today's call
(hidden_dropout / dropout_add) and draws no path seed.  The native path
needs ops/dropout.py's conditions (training, bf16, a last dim that is a
multiple of 8, GPU tensors, VITFSDP_NATIVE_DROPOUT unset or not "0"),
at least two dims and 0 <= p_elem < 1.  Every other case runs the stock
composition: F.dropout on the branch, then a Bernoulli keep tensor of
shape [B, 1, ..., 1] from the device generator.

Seeds: one CPU-generator integer per mask per call, the element seed
first and the path seed second; a mask that is off draws none.
"""

import torch
import torch.nn.functional as F

from ._extension import ext
from .attention import dropout_mask_reference
from .dropout import (
    _seed, _use_native, dropout_add, hidden_dropout, hidden_dropout_mask,
)


def _check_p_path(p_path):
    if p_path < 0.0 or p_path >= 1.0:
        raise ValueError(
            f"drop_path probability has to be in [0, 1), but got {p_path}"
        )


def _use_native_path(p_path, p_elem, training, *tensors):
    x = tensors[0]
    return (
        _use_native(p_path, training, *tensors)
        and x.dim() >= 2
        and x.shape[0] >= 1
        and 0.0 <= p_elem < 1.0
    )


def _seeds(p_elem, seed, elem_seed):
    # element seed first, path seed second; no draw for a mask that is off
    elem_seed = _seed(elem_seed) if p_elem > 0.0 else 0
    return _seed(seed), elem_seed


class _DropPathFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n_samples, p_path, seed, p_elem, elem_seed):
        ctx.args = (n_samples, p_path, seed, p_elem, elem_seed)
        return ext().drop_path_fwd(x.contiguous(), *ctx.args)

    @staticmethod
    def backward(ctx, dy):
        # its own adjoint: the same masks and scale on dy
        dx = ext().drop_path_fwd(dy.contiguous(), *ctx.args)
        return dx, None, None, None, None, None


class _DropPathAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, n_samples, p_path, seed, p_elem, elem_seed):
        ctx.args = (n_samples, p_path, seed, p_elem, elem_seed)
        return ext().drop_path_add_fwd(
            x.contiguous(), res.contiguous(), *ctx.args)

    @staticmethod
    def backward(ctx, dout):
        dres = None
        if ctx.needs_input_grad[1]:
            dres = ext().drop_path_fwd(dout.contiguous(), *ctx.args)
        return dout, dres, None, None, None, None, None


def _stock_drop_path(branch, p_path, p_elem):
    branch = F.dropout(branch, p_elem, True)
    keep = branch.new_empty(
        tuple(branch.shape[:1]) + (1,) * (branch.dim() - 1)
    ).bernoulli_(1.0 - p_path)
    return branch * keep / (1.0 - p_path)


def drop_path(x, p_path, training, p_elem=0.0, seed=None, elem_seed=None):
    """drop_path(F.dropout(x, p_elem, training), p_path, training); one
    fused pass with in-kernel hash masks on GPU bf16."""
    _check_p_path(p_path)
    if not training or p_path == 0.0:
        return hidden_dropout(x, p_elem, training, seed=elem_seed)
    if _use_native_path(p_path, p_elem, training, x):
        seed, elem_seed = _seeds(p_elem, seed, elem_seed)
        return _DropPathFn.apply(
            x, x.shape[0], float(p_path), seed, float(p_elem), elem_seed)
    return _stock_drop_path(x, p_path, p_elem)


def drop_path_add(x, res, p_path, training, p_elem=0.0, seed=None,
                  elem_seed=None):
    """x + drop_path(F.dropout(res, p_elem, training), p_path, training);
    one fused pass on GPU bf16."""
    _check_p_path(p_path)
    if not training or p_path == 0.0:
        return dropout_add(x, res, p_elem, training, seed=elem_seed)
    if _use_native_path(p_path, p_elem, training, x, res):
        seed, elem_seed = _seeds(p_elem, seed, elem_seed)
        return _DropPathAddFn.apply(
            x, res, x.shape[0], float(p_path), seed, float(p_elem), elem_seed)
    return x + _stock_drop_path(res, p_path, p_elem)


# ---- references for the tests --------------------------------------------


def drop_path_mask(seed, n_samples, p):
    """Keep mask [n_samples] (bool, CPU) of the drop-path kernels: sample
    b is kept iff dropout_hash(seed, b, 0) >= p * 2^32."""
    return dropout_mask_reference(
        seed, torch.arange(n_samples), torch.tensor([0]), p
    ).reshape(n_samples)


def drop_path_reference(x, n_samples, p_path, seed, p_elem=0.0, elem_seed=0):
    """fp64 keep_sample && keep_elem ? x / ((1 - p_path)(1 - p_elem)) : 0,
    rows of x flattened and split evenly over n_samples."""
    cols = x.shape[-1]
    rows = x.numel() // cols
    keep = drop_path_mask(seed, n_samples, p_path).repeat_interleave(
        rows // n_samples).reshape(rows, 1).expand(rows, cols)
    if p_elem > 0.0:
        keep = keep & hidden_dropout_mask(elem_seed, rows, cols, p_elem)
    keep = keep.reshape(x.shape).to(x.device)
    x64 = x.double()
    rscale = 1.0 / ((1.0 - p_path) * (1.0 - p_elem))
    return torch.where(keep, x64 * rscale, torch.zeros_like(x64))


def drop_path_add_reference(x, res, n_samples, p_path, seed, p_elem=0.0,
                            elem_seed=0):
    """fp64 x + drop_path_reference(res, ...)."""
    return x.double() + drop_path_reference(
        res, n_samples, p_path, seed, p_elem, elem_seed)
