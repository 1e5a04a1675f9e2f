"""Patch dropout (--patch_drop_rate): a random K of the T patch tokens
per sample in training, with the plan, the pos-embed gather and its
gradient on csrc/patch_drop.hip.

This is timm's PatchDropout with ordered=True (the FLIP / MAE recipe):
the kept tokens stay in their original order, which carries no
information under a learned absolute position embedding and mean pooling,
and keeps every gather monotone.  Two calls make the front of the model:

  patch_drop_plan(B, T, K, device)      -> idx [B, K], inv [B, T]  (int32)
  patch_drop_embed(proj, pos, idx, inv) -> dropout(proj + pos[idx])

idx lists each sample's kept tokens ascending; inv is its inverse, -1 at
a dropped token.  The plan comes first, so that only the kept patch rows
are projected.  On the native path the subset is a pure function of one
integer: token t of sample b gets the key dropout_hash(seed, b, t) and the
K smallest (key, t) pairs are kept, so the checkpoint machinery and
torch.manual_seed reproduce it from the CPU generator alone.
patch_drop_embed is one autograd.Function that saves inv and nothing
else; its backward is one kernel that writes the gradient of proj and
sums the gradient of pos over the batch in a fixed order, with no
scatter-add and no atomics.

Routing follows ops/dropout.py: the native path needs training, GPU
bf16 tensors, E % 8 == 0, T <= 1024 and VITFSDP_NATIVE_DROPOUT unset or
not "0".  Every other case runs the stock composition: timm's
rand / argsort / sort for the subset (device generator), indexing for the
gather and hidden_dropout for the dropout.

Seeds: one CPU-generator integer per mask per call, the plan seed (in
patch_drop_plan) first and the dropout seed (in patch_drop_embed) second;
a mask that is off draws none.
"""

import torch

from ._extension import ext, use_hip
from .attention import _dropout_hash
from .dropout import (
    _native_dropout_on, _seed, hidden_dropout, hidden_dropout_mask,
)

_MAX_TOKENS = 1024  # csrc/patch_drop.hip kMaxTokens


def _inverse_plan(idx, T):
    B, K = idx.shape
    inv = torch.full((B, T), -1, dtype=torch.int32, device=idx.device)
    slots = torch.arange(K, dtype=torch.int32, device=idx.device)
    return inv.scatter_(1, idx.long(), slots.expand(B, K))


def patch_drop_plan(B, T, K, device, seed=None):
    """(idx int32 [B, K] ascending, inv int32 [B, T]): a uniformly random
    K-subset of range(T) per sample and its inverse."""
    if not 1 <= K <= T:
        raise ValueError(f"K has to be in [1, T = {T}], but got {K}")
    device = torch.device(device)
    if (device.type == "cuda" and T <= _MAX_TOKENS and _native_dropout_on()
            and use_hip(torch.empty(0, device=device))):
        with torch.cuda.device(device):
            return tuple(ext().patch_drop_plan(_seed(seed), B, T, K))
    idx = torch.rand(B, T, device=device).argsort(-1)[:, :K].sort(-1).values
    idx = idx.to(torch.int32)
    return idx, _inverse_plan(idx, T)


class _PatchDropEmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, proj, pos, idx, inv, p, seed):
        T, E = pos.shape[-2:]
        ctx.save_for_backward(inv)
        ctx.p, ctx.seed, ctx.pos_shape = p, seed, pos.shape
        return ext().patch_drop_embed_fwd(
            proj.contiguous(), pos.reshape(T, E).contiguous(), idx, p, seed)

    @staticmethod
    def backward(ctx, dy):
        (inv,) = ctx.saved_tensors
        dproj, dpos = ext().patch_drop_embed_bwd(
            dy.contiguous(), inv, ctx.pos_shape[-2], ctx.p, ctx.seed)
        return dproj, dpos.reshape(ctx.pos_shape), None, None, None, None


def _use_native(proj, pos, idx, inv, p, training):
    return (
        training
        and 0.0 <= p < 1.0
        and proj.dtype == torch.bfloat16 and pos.dtype == torch.bfloat16
        and idx.dtype == torch.int32 and inv.dtype == torch.int32
        and proj.dim() == 3
        and proj.shape[-1] > 0 and proj.shape[-1] % 8 == 0
        and pos.shape[-2] <= _MAX_TOKENS
        and use_hip(proj, pos)
        and all(t.is_cuda for t in (proj, pos, idx, inv))
        and _native_dropout_on()
    )


def patch_drop_embed(proj, pos, idx, inv, p, training, seed=None):
    """hidden_dropout(proj + pos[idx], p, training) for proj [B, K, E],
    pos [T, E] or [1, T, E] and a plan (idx, inv); one fused pass each way
    on GPU bf16."""
    if _use_native(proj, pos, idx, inv, p, training):
        seed = _seed(seed) if p > 0.0 else 0
        return _PatchDropEmbedFn.apply(proj, pos, idx, inv, float(p), seed)
    T, E = pos.shape[-2:]
    return hidden_dropout(
        proj + pos.reshape(T, E)[idx.long()], p, training, seed=seed)


# ---- references for the tests --------------------------------------------


def patch_drop_plan_reference(seed, B, T, K):
    """_C.patch_drop_plan bit for bit on the CPU: (idx, inv) int32."""
    keys = _dropout_hash(seed, torch.arange(B), torch.arange(T))
    # stable: equal keys rank by token, as the kernel's (key, t) pairs
    kept = keys.argsort(dim=1, stable=True)[:, :K]
    idx = kept.sort(dim=1).values.to(torch.int32)
    return idx, _inverse_plan(idx, T)


def patch_drop_embed_reference(proj, pos, idx, p, seed):
    """fp64 keep ? (proj + pos[idx]) / (1 - p) : 0 under the hash mask of
    the flattened [B * K, E] output; p == 0 is no mask."""
    B, K, E = proj.shape
    out = proj.double() + pos.double().reshape(-1, E)[idx.long()]
    if p > 0.0:
        mask = hidden_dropout_mask(seed, B * K, E, p).reshape(B, K, E)
        out = torch.where(mask.to(out.device), out / (1.0 - p),
                          torch.zeros_like(out))
    return out
