"""Gradient (activation) checkpointing wrapper.

Capability parity with torch_xla's checkpoint_module as the reference
composes it (run_vit_training.py:13,143-145,194): activations inside the
wrapped module are discarded in forward and recomputed in backward, and
the wrapper sits INSIDE the FSDP wrapper so the recompute reuses the
FSDP-gathered full parameters.

Interplay with our FSDP engine: the FSDP unit's pre-backward hook (on
the unit output) fires before this wrapper's recompute, refilling the
flat parameter storage that the module's leaf views point into — so the
recompute transparently reads correct weights.  Non-reentrant torch
checkpointing is used (recompute happens lazily at saved-tensor unpack,
inside the same backward engine invocation, which keeps FSDP's
end-of-backward callback semantics intact).  RNG state is saved and
restored so dropout masks match between forward and recompute.
"""

import threading

import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

_region = threading.local()


def in_checkpoint_region():
    """Whether the caller runs inside a region checkpointed by
    CheckpointWrapper, in the forward or in the backward's recompute
    (which runs on the autograd engine's thread)."""
    return getattr(_region, "depth", 0) > 0


def _as_region(fn):
    def run(*args, **kwargs):
        _region.depth = getattr(_region, "depth", 0) + 1
        try:
            return fn(*args, **kwargs)
        finally:
            _region.depth -= 1

    return run


def n_open_mlp_blocks(n_blocks, n_ckpt, embed_dim, hidden_dim, kept_dim=None):
    """How many of the n_ckpt checkpointed blocks run their MLP half
    outside the checkpoint region, so that fc1 and the activation are not
    recomputed, without more saved activation memory than checkpointing
    them whole.

    Per token row, in elements: every block whose MLP runs outside a
    region stops keeping the activation (ops/linear.py
    mlp_fc2_recompute_act), hidden_dim less for each of the
    n_blocks - n_ckpt blocks that are not checkpointed; an opened block
    keeps the stream and the LN2 output (embed_dim each) and h (kept_dim)
    that a block checkpointed whole does not.  kept_dim is hidden_dim for
    the GELU MLP, the default, and twice that for the gated one, whose h
    holds the gate and the value half.  So what the former free pays for
    floor((n_blocks - n_ckpt) * hidden_dim / (2 * embed_dim + kept_dim))
    of the latter.  Model shape and checkpoint depth only: the same on
    every rank."""
    if kept_dim is None:
        kept_dim = hidden_dim
    n_ckpt = max(0, min(n_ckpt, n_blocks))
    freed = (n_blocks - n_ckpt) * hidden_dim
    return min(n_ckpt, freed // (2 * embed_dim + kept_dim))


class CheckpointWrapper(nn.Module):
    """open_mlp: checkpoint only the module's attention half
    (``attn_half``: everything up to and including the second LayerNorm)
    and run its ``mlp_half`` on what that returns outside the region, its
    activations kept as in a block that is not checkpointed."""

    WRAPPER_ATTR = "_checkpoint_wrapped_module"

    def __init__(self, module, open_mlp=False):
        super().__init__()
        setattr(self, self.WRAPPER_ATTR, module)
        self.open_mlp = open_mlp

    def forward(self, *args, **kwargs):
        module = getattr(self, self.WRAPPER_ATTR)
        if not torch.is_grad_enabled():
            return module(*args, **kwargs)
        region = module.attn_half if self.open_mlp else module
        out = checkpoint(
            _as_region(region),
            *args,
            use_reentrant=False,
            preserve_rng_state=True,
            **kwargs,
        )
        return module.mlp_half(*out) if self.open_mlp else out


def checkpoint_module(module, open_mlp=False):
    """Wrap `module` so its forward activations are recomputed in
    backward (reference: torch_xla checkpoint_module)."""
    return CheckpointWrapper(module, open_mlp=open_mlp)
