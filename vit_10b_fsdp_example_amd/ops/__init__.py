from ._extension import ext, has_ext, use_hip
from .layernorm import LayerNorm, layer_norm, fused_add_layer_norm
from .attention import attention, attention_qkv, math_attention
from .cross_entropy import CrossEntropyLoss, cross_entropy
from .adamw import FusedAdamW
from .multi_tensor import local_sqnorm, scale_
from .linear import (
    NativeLinear, NativeWgradMode, TunedGemmMode, gemm_dispatch_context,
)
from .dropout import (
    HiddenDropout, dropout_add, dropout_add_reference, gelu_dropout,
    gelu_dropout_reference, hidden_dropout, hidden_dropout_mask,
    hidden_dropout_reference,
)
from .drop_path import (
    drop_path, drop_path_add, drop_path_add_reference, drop_path_mask,
    drop_path_reference,
)

__all__ = [
    "ext",
    "has_ext",
    "use_hip",
    "LayerNorm",
    "layer_norm",
    "fused_add_layer_norm",
    "attention",
    "attention_qkv",
    "math_attention",
    "CrossEntropyLoss",
    "cross_entropy",
    "FusedAdamW",
    "local_sqnorm",
    "scale_",
    "NativeLinear",
    "NativeWgradMode",
    "TunedGemmMode",
    "gemm_dispatch_context",
    "HiddenDropout",
    "hidden_dropout",
    "dropout_add",
    "gelu_dropout",
    "hidden_dropout_mask",
    "hidden_dropout_reference",
    "dropout_add_reference",
    "gelu_dropout_reference",
    "drop_path",
    "drop_path_add",
    "drop_path_mask",
    "drop_path_reference",
    "drop_path_add_reference",
]
