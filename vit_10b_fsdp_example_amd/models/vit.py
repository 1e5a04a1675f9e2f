"""Vision Transformer built from our own modules over MI355X-native ops.

Capability parity with the reference's FSDPViTModel
(run_vit_training.py:99-162) and the timm 0.4.12 modules it pulls in
(PatchEmbed / Block, run_vit_training.py:14-19), re-designed for the
hardware:

  * PatchEmbed is a pure GEMM, not a convolution: patches do not overlap
    (kernel == stride), so the im2col is a free reshape/permute and the
    projection is a [B*T, 3*p*p] x [3*p*p, E] hipBLASLt GEMM — no MIOpen
    conv path.
  * LayerNorm / attention core / loss run in hand-written CDNA4 HIP
    kernels on GPU (see ops/), eager torch on CPU.
  * The FSDP and gradient-checkpoint wrappers are injected callables
    (grad_ckpt_wrap, fsdp_wrap), preserving the reference's one real
    architectural seam (run_vit_training.py:118-119,145,194-199): the
    same model class runs with or without sharding.

Weight init matches the reference *behavior*: timm 0.4.12's
_init_vit_weights is a single-module (non-recursive) function, and the
reference calls it on container modules where it matches no isinstance
branch — a documented no-op.  So blocks keep framework
default init and only pos_embed gets trunc_normal(std=0.02).  Pass
recursive=True to init_vit_weights for the "intended" behavior.
"""

import os

import torch
import torch.nn as nn

from .. import dist as xdist
from ..ops import (  # noqa: F401
    HiddenDropout, LayerNorm, NativeLinear, attention_qkv, cross_entropy,
    RMSNorm, drop_path, drop_path_add, dropout_add, fused_add_layer_norm,
    fused_add_rms_norm, gelu_dropout, hidden_dropout, layer_scale,
    layer_scale_add, patch_drop_embed, patch_drop_plan, swiglu,
    swiglu_fc2_recompute, swiglu_hidden_dim,
)
from ..ops.linear import mlp_fc2_recompute_act, mlp_recompute_act_on
from ..parallel.checkpoint import in_checkpoint_region, n_open_mlp_blocks


def init_vit_weights(module, recursive=False):
    """timm-0.4.12-compatible init (see module docstring).

    Single-module semantics by default: only has an effect when `module`
    itself is Linear or LayerNorm.  The reference calls this on
    PatchEmbed / Block containers, where it is a no-op —
    we replicate that exactly so loss curves correspond.
    """
    def _apply(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, (nn.LayerNorm, LayerNorm)):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)
        elif isinstance(m, RMSNorm):
            nn.init.ones_(m.weight)

    if recursive:
        module.apply(_apply)
    else:
        _apply(module)


class PatchEmbed(nn.Module):
    """Non-overlapping patch projection as a single GEMM.

    Equivalent to timm's Conv2d(kernel=patch, stride=patch) + flatten +
    transpose (reference run_vit_training.py:124): the conv weight
    [E, 3, p, p] flattened over (c, ph, pw) equals our Linear weight
    [E, 3*p*p], and the input patch extraction is a reshape/permute.
    """

    def __init__(self, img_size=224, patch_size=14, in_chans=3, embed_dim=768):
        super().__init__()
        assert img_size % patch_size == 0, "image size must divide by patch size"
        self.img_size = img_size
        self.patch_size = patch_size
        self.in_chans = in_chans
        self.grid_size = img_size // patch_size
        self.num_patches = self.grid_size * self.grid_size
        self.proj = nn.Linear(in_chans * patch_size * patch_size, embed_dim)

    def forward(self, x, idx=None):
        """idx [B, K] (patch dropout): project only patch rows idx[b] of
        sample b, giving [B, K, E]."""
        B, C, H, W = x.shape
        p, g = self.patch_size, self.grid_size
        # [B, C, g, p, g, p] -> [B, g, g, C, p, p] -> [B, T, C*p*p]
        x = x.reshape(B, C, g, p, g, p).permute(0, 2, 4, 1, 3, 5)
        x = x.reshape(B, g * g, C * p * p)
        if idx is not None:
            x = x[torch.arange(B, device=x.device)[:, None], idx.long()]
        return self.proj(x)


class Attention(nn.Module):
    """Pre-projection multi-head attention matching timm 0.4.12's module
    (fused qkv Linear with bias, per-head scaled dot product, attention
    dropout, output projection + dropout).

    qk_norm (timm's flag of that name, ViT-22B's remedy for attention-
    logit growth): a LayerNorm over head_dim on q and on k before the dot
    product, its parameters shared by all heads.  q_norm and k_norm exist
    only when it is on.  qk_norm_type "rmsnorm" makes them ops.RMSNorm
    (weight only; timm's qk_norm with norm_layer=RmsNorm), on
    csrc/qk_rmsnorm.hip."""

    def __init__(self, dim, num_heads, qkv_bias=True, attn_drop=0.0,
                 proj_drop=0.0, qk_norm=False, qk_norm_type="layernorm"):
        super().__init__()
        if qk_norm_type not in NORM_TYPES:
            raise ValueError(
                f"qk_norm_type has to be one of {NORM_TYPES}, but got "
                f"{qk_norm_type!r}"
            )
        assert dim % num_heads == 0
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        # NativeLinear: weight gradients route through the csrc wgrad
        # kernel where the shape qualifies (ops/linear.py)
        self.qkv = NativeLinear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop_p = attn_drop
        self.proj = NativeLinear(dim, dim)
        self.proj_drop = HiddenDropout(proj_drop)
        self.qk_norm = qk_norm
        if qk_norm:
            self.q_norm = make_norm(qk_norm_type, self.head_dim)
            self.k_norm = make_norm(qk_norm_type, self.head_dim)

    def forward(self, x, skip_proj_drop=False):
        """skip_proj_drop: return the projection output BEFORE proj_drop;
        the block then folds that dropout into its drop_path pass."""
        B, T, E = x.shape
        # [B, T, 3, H, d] is a free view of the fused projection; the
        # attention core reads q/k/v through strides and returns [B, T, E]
        # directly (no permute/contiguous copies around the kernel)
        qkv = self.qkv(x).reshape(B, T, 3, self.num_heads, self.head_dim)
        qk_norm = None
        if self.qk_norm:
            # an RMSNorm has no bias: (wq, None, wk, None, eps)
            qk_norm = (self.q_norm.weight, getattr(self.q_norm, "bias", None),
                       self.k_norm.weight, getattr(self.k_norm, "bias", None),
                       self.q_norm.eps)
        o = attention_qkv(
            qkv,
            self.num_heads,
            scale=self.scale,
            dropout_p=self.attn_drop_p,
            training=self.training,
            qk_norm=qk_norm,
        )
        o = self.proj(o)
        return o if skip_proj_drop else self.proj_drop(o)


MLP_TYPES = ("gelu", "swiglu")


class Mlp(nn.Module):
    """fc1 -> GELU -> dropout -> fc2 -> dropout (timm Mlp).

    forward returns fc2's output BEFORE its dropout, together with the
    dropout probability: the block applies that dropout itself, fused
    into the residual add (ops.dropout_add) or, with the deferred
    residual, as ops.hidden_dropout on the branch.

    mlp_type "swiglu" is the gated MLP: fc1 is Linear(dim, 2 * hidden_dim),
    and the activation silu(h[..., :hidden_dim]) * h[..., hidden_dim:],
    gate half first (ops.swiglu, csrc/swiglu.hip).  The parameter names
    are those of "gelu"; fc1's shapes differ."""

    def __init__(self, dim, hidden_dim, drop=0.0, mlp_type="gelu"):
        super().__init__()
        if mlp_type not in MLP_TYPES:
            raise ValueError(
                f"mlp_type has to be one of {MLP_TYPES}, but got {mlp_type!r}"
            )
        self.mlp_type = mlp_type
        gated = mlp_type == "swiglu"
        if gated and os.environ.get("VITFSDP_FUSED_GELU", "0") == "1":
            raise ValueError(
                "VITFSDP_FUSED_GELU=1 fuses a GELU into fc1's epilogue and "
                "cannot be combined with mlp_type 'swiglu'"
            )
        self.fc1 = NativeLinear(dim, 2 * hidden_dim if gated else hidden_dim)
        self.fc2 = NativeLinear(hidden_dim, dim)
        self.drop = HiddenDropout(drop)
        from ..ops.linear import configure_gelu_fusion, configure_swiglu

        if gated:
            # fc1's input width, for the dh^T gate of the SwiGLU backward
            configure_swiglu(dim)
        else:
            # register the MLP dims so the GEMM dispatch router can fuse
            # the GELU into the fc1/fc2 hipBLASLt epilogues
            # (VITFSDP_FUSED_GELU)
            configure_gelu_fusion(dim, hidden_dim)

    def forward(self, x):
        p = self.drop.p
        h = self.fc1(x)
        # outside a checkpoint region the activation is not kept for the
        # backward but rebuilt from h there (ops/linear.py
        # mlp_fc2_recompute_act)
        recompute = (torch.is_grad_enabled() and mlp_recompute_act_on(p)
                     and not in_checkpoint_region())
        if self.mlp_type == "swiglu":
            if recompute:
                return swiglu_fc2_recompute(self.fc2, h), p
            return self.fc2(swiglu(h, p, self.training)), p
        if recompute:
            return mlp_fc2_recompute_act(self.fc2, h), p
        return self.fc2(gelu_dropout(h, p, self.training)), p


class LayerScale(nn.Module):
    """Learnable per-channel scale of a residual branch (CaiT; timm's
    module and parameter name, so blocks.N.ls1.gamma / ls2.gamma match
    timm checkpoints).  Block does not call it: it hands gamma to
    ops.layer_scale / ops.layer_scale_add, which fold the scale into the
    branch's dropout, drop-path and residual-add pass."""

    def __init__(self, dim, init):
        super().__init__()
        self.gamma = nn.Parameter(torch.full((dim,), float(init)))

    def forward(self, x):
        return layer_scale(x, self.gamma, self.training)


NORM_TYPES = ("layernorm", "rmsnorm")


def make_norm(norm_type, dim):
    """The norm module of blocks.N.norm1 / norm2, the final norm and
    attn.q_norm / k_norm."""
    if norm_type not in NORM_TYPES:
        raise ValueError(
            f"norm_type has to be one of {NORM_TYPES}, but got {norm_type!r}"
        )
    if norm_type == "rmsnorm":
        return RMSNorm(dim, eps=1e-6)
    return LayerNorm(dim, eps=1e-6)


def apply_norm(norm, x, res=None):
    """The one seam to a norm module of either type: norm(x), or with res
    the fused pair (x + res, norm(x + res))."""
    if res is None:
        return norm(x)
    if isinstance(norm, RMSNorm):
        return fused_add_rms_norm(x, res, norm.weight, norm.eps)
    return fused_add_layer_norm(x, res, norm.weight, norm.bias, norm.eps)


class Block(nn.Module):
    """Pre-LN transformer block: x + Attn(LN1(x)); x + MLP(LN2(x))
    (timm Block as configured at reference run_vit_training.py:134-141).

    drop_path (unused by the reference, default 0) is timm's stochastic
    depth: in training each of the two branches is dropped per sample
    with that probability and scaled by 1 / (1 - drop_path) otherwise,
    after the branch's own dropout and with an independent mask each
    (ops.drop_path / ops.drop_path_add, one fused pass per branch).  At 0
    the block runs exactly the statements it ran without it.

    layer_scale_init (timm's init_values, default 0 = off): with a value
    > 0 each branch is multiplied by a learnable per-channel vector
    (ls1.gamma, ls2.gamma) initialised to it, between the branch's
    dropout and its drop-path mask: x + drop_path(gamma * dropout(branch)).
    The scale, both masks and the MLP residual add are one pass
    (ops.layer_scale / ops.layer_scale_add).  At 0 neither module exists
    and the block runs exactly the statements it ran without it.

    Two interfaces, identical math:
      * default: tensor -> tensor, with the attention residual add fused
        into norm2 (one ln_add kernel) and the MLP residual as a plain
        add;
      * deferred residual (Megatron-style, --fuse_residual): input and
        output are (hidden, stream) pairs and the MLP residual add is
        fused into the NEXT block's norm1 — no standalone elementwise
        add kernels remain anywhere in the block stack.  The bf16
        rounding of every sum matches the plain add exactly (ln_add
        rounds the fp32 sum to bf16 the same way torch's add does).

    norm_type "rmsnorm" makes norm1 and norm2 ops.RMSNorm (weight only,
    csrc/rmsnorm.hip), with the same fused residual adds; the norm of
    qk_norm is chosen by qk_norm_type alone.
    """

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=True,
                 drop=0.0, attn_drop=0.0, deferred_residual=False,
                 drop_path=0.0, qk_norm=False, layer_scale_init=0.0,
                 mlp_type="gelu", norm_type="layernorm",
                 qk_norm_type="layernorm"):
        super().__init__()
        if layer_scale_init < 0:
            raise ValueError(
                f"layer_scale_init has to be >= 0, but got {layer_scale_init}"
            )
        if drop_path < 0 or drop_path >= 1:
            raise ValueError(
                f"drop_path probability has to be in [0, 1), but got "
                f"{drop_path}"
            )
        self.deferred_residual = deferred_residual
        self.drop_path = drop_path
        self.norm1 = make_norm(norm_type, dim)
        self.attn = Attention(
            dim, num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop,
            proj_drop=drop, qk_norm=qk_norm, qk_norm_type=qk_norm_type,
        )
        self.norm2 = make_norm(norm_type, dim)
        hidden_dim = (swiglu_hidden_dim(dim, mlp_ratio)
                      if mlp_type == "swiglu" else int(dim * mlp_ratio))
        self.mlp = Mlp(dim, hidden_dim, drop=drop, mlp_type=mlp_type)
        self.layer_scale_init = layer_scale_init
        if layer_scale_init > 0:
            self.ls1 = LayerScale(dim, layer_scale_init)
            self.ls2 = LayerScale(dim, layer_scale_init)

    def extra_repr(self):
        return f"drop_path={self.drop_path}"

    def _attn_branch(self, normed):
        if self.layer_scale_init > 0:
            # gamma, proj_drop and the per-sample mask in one pass
            return layer_scale(
                self.attn(normed, skip_proj_drop=True), self.ls1.gamma,
                self.training, p_path=self.drop_path,
                p_elem=self.attn.proj_drop.p,
            )
        if self.drop_path == 0.0:
            return self.attn(normed)
        # proj_drop and the per-sample mask in one pass
        return drop_path(
            self.attn(normed, skip_proj_drop=True), self.drop_path,
            self.training, p_elem=self.attn.proj_drop.p,
        )

    def forward(self, x):
        return self.mlp_half(*self.attn_half(x))

    def attn_half(self, x):
        """Everything up to and including norm2: (stream, norm2 output).
        The checkpoint wrapper's open-MLP form checkpoints this alone."""
        if self.deferred_residual and isinstance(x, (tuple, list)):
            hidden, stream = x
            # previous block's MLP residual add, fused into our norm1
            s0, y0 = apply_norm(self.norm1, stream, hidden)
        else:  # plain interface, or first block: nothing pending
            s0, y0 = x, self.norm1(x)
        attn_out = self._attn_branch(y0)
        # fused residual add + norm2 (one kernel for x+attn_out and its LN)
        return apply_norm(self.norm2, s0, attn_out)

    def mlp_half(self, x, normed):
        """The MLP branch on attn_half's pair; returns what forward does."""
        mlp_out, p = self.mlp(normed)
        if self.deferred_residual:
            if self.layer_scale_init > 0:
                return layer_scale(
                    mlp_out, self.ls2.gamma, self.training,
                    p_path=self.drop_path, p_elem=p), x
            if self.drop_path == 0.0:
                return hidden_dropout(mlp_out, p, self.training), x
            return drop_path(
                mlp_out, self.drop_path, self.training, p_elem=p), x
        # MLP residual add with fc2's dropout folded in
        if self.layer_scale_init > 0:
            return layer_scale_add(
                x, mlp_out, self.ls2.gamma, self.training,
                p_path=self.drop_path, p_elem=p)
        if self.drop_path == 0.0:
            return dropout_add(x, mlp_out, p, self.training)
        return drop_path_add(
            x, mlp_out, self.drop_path, self.training, p_elem=p)


class FSDPViTModel(nn.Module):
    """ViT with nested FSDP + gradient checkpointing injected per block
    (reference run_vit_training.py:99-162): PatchEmbed + learned
    pos-embed (no CLS token) + N blocks + final LN + mean-pool + linear
    head (mean pooling per arXiv 2106.04560).

    patch_drop_rate (timm's, default 0 = off): in training each sample
    keeps a random K = max(1, int(T * (1 - rate))) of its T patch tokens,
    in their original order, chosen BEFORE the patch projection, so every
    layer from the projection on sees K rows per sample
    (ops.patch_drop_plan / ops.patch_drop_embed).  It adds no parameters;
    in eval, or at 0, forward runs exactly the statements it ran without
    it."""

    def __init__(
        self,
        image_size,
        patch_size,
        embed_dim,
        num_heads,
        num_blocks,
        mlp_ratio,
        pos_dropout,
        mlp_dropout,
        att_dropout,
        num_classes,
        grad_ckpt_wrap,
        fsdp_wrap,
        fuse_residual=False,
        drop_path_rate=0.0,
        qk_norm=False,
        layer_scale_init=0.0,
        mlp_type="gelu",
        norm_type="layernorm",
        qk_norm_type="layernorm",
        patch_drop_rate=0.0,
    ):
        super().__init__()
        if patch_drop_rate < 0 or patch_drop_rate >= 1:
            raise ValueError(
                f"patch_drop_rate has to be in [0, 1), but got "
                f"{patch_drop_rate}"
            )
        self.fuse_residual = fuse_residual
        self.patch_drop_rate = patch_drop_rate

        self.patch_embed = PatchEmbed(
            img_size=image_size, patch_size=patch_size, in_chans=3,
            embed_dim=embed_dim,
        )
        init_vit_weights(self.patch_embed)
        num_patches = self.patch_embed.num_patches
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches, embed_dim))
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        self.pos_drop = HiddenDropout(pos_dropout)

        blocks = []
        for idx in range(num_blocks):
            block = Block(
                dim=embed_dim,
                num_heads=num_heads,
                mlp_ratio=mlp_ratio,
                qkv_bias=True,
                drop=mlp_dropout,
                attn_drop=att_dropout,
                deferred_residual=fuse_residual,
                # timm's linspace(0, rate, num_blocks): block 0 never
                # drops, the last block drops at the full rate
                drop_path=drop_path_rate * idx / max(num_blocks - 1, 1),
                qk_norm=qk_norm,
                layer_scale_init=layer_scale_init,
                mlp_type=mlp_type,
                norm_type=norm_type,
                qk_norm_type=qk_norm_type,
            )
            # init BEFORE wrapping: FSDP shards the weights at wrap time
            init_vit_weights(block)
            # grad-ckpt wrapper goes INSIDE the FSDP wrapper so the
            # backward recompute reuses the gathered full params
            # (reference run_vit_training.py:143-145)
            block = fsdp_wrap(grad_ckpt_wrap(block))
            blocks.append(block)
            xdist.master_print(f"built ViT block {idx}")
        self.blocks = nn.Sequential(*blocks)

        self.norm = make_norm(norm_type, embed_dim)
        init_vit_weights(self.norm)
        self.head = nn.Linear(embed_dim, num_classes)

    def _embed_kept(self, image):
        """Patch dropout: pos_drop(proj(kept patches) + their pos_embed
        rows), [B, K, E]."""
        T = self.patch_embed.num_patches
        K = max(1, int(T * (1.0 - self.patch_drop_rate)))
        idx, inv = patch_drop_plan(image.shape[0], T, K, image.device)
        return patch_drop_embed(
            self.patch_embed(image, idx), self.pos_embed, idx, inv,
            self.pos_drop.p, self.training)

    def forward(self, image):
        if self.training and self.patch_drop_rate > 0:
            x = self._embed_kept(image)
        else:
            x = self.patch_embed(image) + self.pos_embed
            x = self.pos_drop(x)
        x = self.blocks(x)
        if self.fuse_residual:
            # last block's pending MLP residual add fuses into the
            # final norm
            hidden, stream = x
            _, normed = apply_norm(self.norm, stream, hidden)
        else:
            normed = self.norm(x)
        # mean pooling over the patch sequence instead of a [CLS] token
        logits = self.head(torch.mean(normed, dim=1))
        return logits


def count_vit_params(image_size, patch_size, embed_dim, num_blocks, mlp_ratio,
                     num_classes, in_chans=3, num_heads=None, qk_norm=False,
                     layer_scale=False, mlp_type="gelu",
                     norm_type="layernorm", qk_norm_type="layernorm"):
    """Exact parameter count for the architecture (used by tests; the
    10B default config gives 10,077,917,160 — SURVEY.md §2D).  qk_norm
    adds q_norm and k_norm, 4 * head_dim per block (2 * head_dim with
    qk_norm_type "rmsnorm", which has no biases), and needs num_heads;
    layer_scale adds ls1.gamma and ls2.gamma, 2 * embed_dim per block;
    mlp_type "swiglu" has fc1 [2H, e] and fc2 [e, H] with
    H = swiglu_hidden_dim(e, mlp_ratio); norm_type "rmsnorm" has no bias
    in norm1, norm2 and the final norm, embed_dim less per site."""
    e = embed_dim
    hid = int(e * mlp_ratio)
    fc1_out = hid
    if mlp_type == "swiglu":
        hid = swiglu_hidden_dim(e, mlp_ratio)
        fc1_out = 2 * hid
    t = (image_size // patch_size) ** 2
    per_block = (
        e * 3 * e + 3 * e
        + e * e + e
        + e * fc1_out + fc1_out
        + hid * e + e
        + (2 * e if norm_type == "rmsnorm" else 4 * e)
    )
    if qk_norm:
        per_block += (2 if qk_norm_type == "rmsnorm" else 4) * (e // num_heads)
    if layer_scale:
        per_block += 2 * e
    patch_embed = (in_chans * patch_size * patch_size) * e + e
    pos_embed = t * e
    final_norm = e if norm_type == "rmsnorm" else 2 * e
    head = e * num_classes + num_classes
    return num_blocks * per_block + patch_embed + pos_embed + final_norm + head


def build_fsdp_vit_model(cfg, device, compute_dtype=torch.float32):
    """Create the ViT with nested FSDP and gradient checkpointing
    (reference run_vit_training.py:165-200).

    Wrap policy mirrors the reference: per-block
    fsdp_wrap(grad_ckpt_wrap(block)), then a root fsdp_wrap over the
    whole model (no grad-ckpt at the root).  --run_without_fsdp swaps
    both wrappers for identity/to(device) — the plain-DDP baseline.
    """
    from ..parallel import FullyShardedDataParallel as FSDP
    from ..parallel import checkpoint_module

    def fsdp_wrap(module):
        if cfg.run_without_fsdp:
            return module.to(device)
        return FSDP(
            module if cfg.shard_on_cpu else module.to(device),
            reshard_after_forward=cfg.reshard_after_forward,
            flatten_parameters=cfg.flatten_parameters,
            compute_dtype=compute_dtype,
            device=device,
            shard_on_cpu=cfg.shard_on_cpu,
        )

    # --grad_ckpt_blocks N: checkpoint only the first N blocks (identical
    # gradients; recompute is pure overhead wherever activations fit in
    # the 288 GB of HBM3E).  -1 = every block, the reference behavior.
    ckpt_limit = getattr(cfg, "grad_ckpt_blocks", -1)
    ckpt_count = {"i": 0}
    # the first n_open of the checkpointed blocks checkpoint only their
    # attention half: what the others save by not keeping gelu(h) pays
    # for their MLP activations (parallel/checkpoint.py)
    n_open = 0
    mlp_type = getattr(cfg, "mlp_type", "gelu")
    if cfg.grad_ckpt and mlp_recompute_act_on(cfg.mlp_dropout):
        hidden_dim = int(cfg.embed_dim * cfg.mlp_ratio)
        kept_dim = hidden_dim
        if mlp_type == "swiglu":
            # H is freed, h [.., 2H] is kept
            hidden_dim = swiglu_hidden_dim(cfg.embed_dim, cfg.mlp_ratio)
            kept_dim = 2 * hidden_dim
        n_open = n_open_mlp_blocks(
            cfg.num_blocks,
            cfg.num_blocks if ckpt_limit < 0 else ckpt_limit,
            cfg.embed_dim, hidden_dim, kept_dim)

    def grad_ckpt_wrap(module):
        if not cfg.grad_ckpt:
            return module
        idx = ckpt_count["i"]
        ckpt_count["i"] += 1
        if 0 <= ckpt_limit <= idx:
            return module
        return checkpoint_module(module, open_mlp=idx < n_open)

    model = FSDPViTModel(
        image_size=cfg.image_size,
        patch_size=cfg.patch_size,
        embed_dim=cfg.embed_dim,
        num_heads=cfg.num_heads,
        num_blocks=cfg.num_blocks,
        mlp_ratio=cfg.mlp_ratio,
        pos_dropout=cfg.pos_dropout,
        mlp_dropout=cfg.mlp_dropout,
        att_dropout=cfg.att_dropout,
        num_classes=cfg.num_classes,
        grad_ckpt_wrap=grad_ckpt_wrap,
        fsdp_wrap=fsdp_wrap,
        fuse_residual=getattr(cfg, "fuse_residual", False),
        drop_path_rate=getattr(cfg, "drop_path_rate", 0.0),
        qk_norm=getattr(cfg, "qk_norm", False),
        layer_scale_init=getattr(cfg, "layer_scale_init", 0.0),
        mlp_type=mlp_type,
        norm_type=getattr(cfg, "norm_type", "layernorm"),
        qk_norm_type=getattr(cfg, "qk_norm_type", "layernorm"),
        patch_drop_rate=getattr(cfg, "patch_drop_rate", 0.0),
    )
    # root wrap without grad-ckpt (reference run_vit_training.py:197-199)
    model = fsdp_wrap(model)
    return model
