"""Linear layer with a native weight-gradient kernel.

Forward and the input-gradient GEMM go through hipBLASLt (the sanctioned
library path for plain GEMMs; the input gradient as its TN kernel on a
weight transposed by csrc/transpose.hip, see "Input gradients as library
TN GEMMs" below); the weight gradient dW = dY^T X routes
through csrc/wgemm.hip (gfx950 ds_read_b64_tr_b16 hardware transpose
reads on direct-to-LDS staged tiles) for the shapes where that kernel
beats the library INSIDE the training step.

The kernel beats the library in the step on the qkv and proj shapes and
loses on fc1 and fc2, which run the library's TN kernel on operands
transposed by csrc/transpose.hip instead (the "TN weight gradients"
section below, VITFSDP_TN_WGRAD); measurements per shape, isolated and
in the step, in profiles/PROFILES.md "wgemm NT ladder".  The default
route, VITFSDP_NATIVE_WGRAD=2, is the dispatcher-level interception
below (NativeWgradMode, or the wgemm route of TunedGemmMode); the shape
gate _wgrad_mm_shapes_ok keeps fc1/fc2 away from the kernel.
VITFSDP_NATIVE_WGRAD=0 switches the route off.

How the integration got here (all measured on MI355X):
  * the dbias column sums are NOT fused into the GEMM: the per-fragment
    unpack+accumulate VALU work cost 945 -> 535 TF/s on the qkv shape;
    dbias stays a separate memory-bound reduction (the WITH_BIAS kernel
    instantiation remains for the benchmark and its test);
  * kernel timings use a cold-cache rotation (4 operand sets past the
    256 MB L3): a single reused set flattered the kernel ~1.8x;
  * wrapping the linears in a custom autograd.Function (mode "1") lost
    ~164 ms/step: torch's codegen'd addmm packs its input SavedVariables
    BEFORE dispatching the kernel, so checkpoint(use_reentrant=False)
    early-stops the recompute before the region's LAST GEMM (fc2 forward
    is never recomputed); a Function packs only after forward returns
    and forces that GEMM back into every block recompute (+128 forward
    GEMMs per 4 profiled steps; benchmarks/ktrace_diff.py on the ON/OFF
    traces, CPU repro in tests/test_checkpoint_earlystop.py).  Mode "2"
    keeps the stock addmm node and swaps only the kernel at dispatch
    time, so the early-stop survives; the routed traces show no extra
    forward GEMMs;
  * the kernel has no split-K: ungated at ViT-Large (16-64 workgroup dW
    grids) mode 2 ran 1040 -> 702 img/s, hence the _MIN_TILES >= 256
    gate.  The TorchDispatchMode python overhead itself is not
    measurable: backward is GPU-bound and dispatch overlaps with queued
    kernels;
  * with the first version of the kernel the route was neutral at 10B
    (64.5 vs 65.0 img/s) and stayed opt-in; the ladder pass (clustered
    2-D tile mapping, direct-to-LDS staging) made qkv and proj win
    in-step by ~9%, which is what flipped the default.
"""

import contextlib
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode

from ._extension import ext, use_hip
from ..tuning import lt_algo_table


# "1": custom autograd.Function (kept for A/B history; defeats checkpoint
#      early-stop, see tests/test_checkpoint_earlystop.py)
# "2": dispatcher interception below autograd (NativeWgradMode) — the
#      stock addmm node stays, early-stop is preserved.  The default.
# "0": every dW GEMM stays on the library
_WGRAD_MODE = os.environ.get("VITFSDP_NATIVE_WGRAD", "2")
_NATIVE_WGRAD = _WGRAD_MODE == "1"
_NATIVE_WGRAD_DISPATCH = _WGRAD_MODE == "2"


def _use_native_wgrad(dy2, x2, w):
    if not _NATIVE_WGRAD:
        return False
    if not (dy2.is_cuda and dy2.dtype == torch.bfloat16):
        return False
    m, n = w.shape[0], w.shape[1]
    k = dy2.shape[0]
    if not (k % 64 == 0 and m % 256 == 0 and n % 256 == 0):
        return False
    # measured crossover: hipBLASLt wins on the very wide/tall shapes
    if m > 16384 or n > 8192:
        return False
    return use_hip(dy2) and hasattr(ext(), "wgrad_gemm")


class _NativeLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        dx = torch.matmul(dy, weight)  # hipBLASLt dgrad

        if _use_native_wgrad(dy2, x2, weight):
            # dbias via the fused in-kernel column sums measured ~1.7x
            # slower end-to-end (per-fragment unpack+accumulate VALU);
            # the plain reduction is one cheap memory-bound pass
            (dw,) = ext().wgrad_gemm(dy2.contiguous(), x2.contiguous(), False)
            db = dy2.sum(0) if ctx.has_bias else None
        else:
            dw = torch.matmul(dy2.t(), x2)
            db = dy2.sum(0) if ctx.has_bias else None
        return dx, dw, db


# The kernel has no split-K: its grid is (m/256)*(n/256) workgroups, so
# small dW matrices cannot fill 256 CUs (ViT-Large proj dW is 16
# workgroups and measured 1040 -> 702 img/s when routed native).  10B
# qkv/proj are 1200/400 workgroups.  Env override for experiments.
_MIN_TILES = int(os.environ.get("VITFSDP_WGRAD_MIN_TILES", "256"))


def _wgrad_mm_shapes_ok(m, n, k):
    """Shape gate for the native wgrad kernel: the 256x256x64 tile must
    divide evenly (the same condition wgrad_gemm checks), the grid must
    be large enough to fill the chip (_MIN_TILES), and only shapes that
    beat the library in the ViT-10B step are routed: qkv (-0.45 ms per
    call) and proj (-0.17 ms) go native, the 20480-wide MLP shapes stay
    on hipBLASLt (fc1 +0.12 ms, fc2 +0.22 ms per call when routed).
    Symmetric bound because the dispatcher sees dW in whichever
    orientation AddmmBackward chose."""
    return (k % 64 == 0 and m % 256 == 0 and n % 256 == 0
            and m <= 16384 and n <= 16384
            and (m // 256) * (n // 256) >= _MIN_TILES)


def _wgrad_mm_dims(at, b):
    """(m, n, k) if mm(at, b) has the layout of the weight-gradient GEMM
    AddmmBackward emits — first operand a transposed view of a
    contiguous [K, M] base, second operand contiguous [K, N] — else
    None."""
    if at.dim() != 2 or b.dim() != 2 or at.shape[1] != b.shape[0]:
        return None
    m, k = at.shape
    if m < 2 or k < 2:
        return None  # degenerate strides are ambiguous
    if not (at.stride(0) == 1 and at.stride(1) == m):
        return None
    if not (b.stride(1) == 1 and b.stride(0) == b.shape[1]):
        return None
    return m, b.shape[1], k


def _is_wgrad_mm(at, b):
    """The weight-gradient GEMM, at a shape the native kernel takes."""
    dims = _wgrad_mm_dims(at, b)
    return dims is not None and _wgrad_mm_shapes_ok(*dims)


# --------------------------------------------------------------------------
# Weight gradients as library TN GEMMs on transposed operands
# (csrc/transpose.hip).  In dW[out, in] = dY^T X both operands have the
# token index as the slow dimension, the NT form, which the library runs
# 30-40 % slower than its TN form at these sizes.  Transposing both
# operands is memory traffic at ~5 TB/s against a compute-bound GEMM,
# and the pass over dY also yields dY's column sums, the bias gradient,
# so the separate reduction goes too.  AddmmBackward on this torch emits
#     mm(dy, W) ; mm(dy.t(), x) -> [out, in] ; sum.dim_IntList(dy, [0], True)
# and the route answers the second and third; either may come first.
# fc1's dy^T is a third output of the GELU backward
# (_C.gelu_bwd_colsum_t, VITFSDP_TN_DGELU_T; behind hidden dropout see
# _DGELU_DROP_T below).
#
# Gate: the shapes that won both isolated and in the step, fc1 and fc2
# (_TN_WGRAD_SHAPES); proj loses and qkv leads the wgemm.hip path by less
# than the spread of its own samples, so both stay there.
# VITFSDP_TN_WGRAD=0 turns the route off.  Measurements:
# benchmarks/bench_tn_wgrad.py, profiles/PROFILES.md "TN wgrad".
# --------------------------------------------------------------------------

# (out, in) of the dW shapes that won both isolated and in the step
_TN_WGRAD_SHAPES = frozenset({(20480, 5120), (5120, 20480)})

# The measurements are at K = 32768.  Transpose bytes and GEMM FLOPs both
# scale with K, so their ratio holds at other batch sizes; the floor only
# keeps the route away from GEMMs too short to be compute-bound.
_TN_WGRAD_MIN_K = 4096

# Experiments and tests: when >= 0, every dW with out * in >= this many
# elements is routed whatever the table and the K floor say.
_TN_MIN_ELEMS = int(os.environ.get("VITFSDP_TN_WGRAD_MIN_ELEMS", "-1"))


def _tn_wgrad_on():
    return os.environ.get("VITFSDP_TN_WGRAD", "1") != "0"


def _tn_dgelu_t_on():
    """fc1's dy^T as a third output of the GELU backward
    (_C.gelu_bwd_colsum_t) instead of a transpose2d of its result."""
    return os.environ.get("VITFSDP_TN_DGELU_T", "1") != "0"


def _tn_wgrad_shapes_ok(m, n, k):
    """Shape gate of the TN route for dW [m = out, n = in] over k rows.
    Both transposes need a multiple of 8 columns."""
    if m % 8 or n % 8:
        return False
    if _TN_MIN_ELEMS >= 0:
        return m * n >= _TN_MIN_ELEMS
    return (m, n) in _TN_WGRAD_SHAPES and k >= _TN_WGRAD_MIN_K


def _tn_wgrad_out_ok(m, k):
    """The gate as far as it can be told from dy [k, m] alone, for a
    bias sum that arrives before its GEMM."""
    if m % 8 or k < 2:
        return False
    if _TN_MIN_ELEMS >= 0:
        return True
    return k >= _TN_WGRAD_MIN_K and any(m == s[0] for s in _TN_WGRAD_SHAPES)


def _is_tn_wgrad_mm(at, b):
    """The weight-gradient GEMM, at a shape the TN route takes."""
    dims = _wgrad_mm_dims(at, b)
    return dims is not None and _tn_wgrad_shapes_ok(*dims)


# --------------------------------------------------------------------------
# Input gradients as library TN GEMMs on a transposed weight
# (_C.dgrad_tn, csrc/ltgemm.cpp + csrc/transpose.hip).  dX[tok, in] =
# dY[tok, out] W[out, in] is the library's NN form; with W^T [in, out]
# as a contiguous tensor it is the TN form of a forward, which the step
# trace shows 13-15 % faster per FLOP.  Only the weight is transposed:
# 52-210 MB read and written once per call against a 5-7 TFLOP GEMM.
# The route answers AddmmBackward's mm(dy, W), both operands
# row-contiguous; W^T lives in a scratch buffer of the extension and is
# rebuilt on every call (weights change every step).
#
# The TN index is the tabled one of the forward with the same sizes (fc2,
# fc1 and proj forwards); qkv's key ("T","N", 5120, tok, 15360) has no
# entry and takes the library heuristic, which no searched index beats on
# cold caches.  Gate: all four weights of the block won isolated and in
# the step (_TN_DGRAD_SHAPES).  VITFSDP_TN_DGRAD=0 turns the route off.
# Measurements: benchmarks/bench_tn_dgrad.py, profiles/PROFILES.md
# "TN dgrad".
# --------------------------------------------------------------------------

# (out, in) of the weights whose dgrad won both isolated and in the step
_TN_DGRAD_SHAPES = frozenset(
    {(15360, 5120), (5120, 5120), (20480, 5120), (5120, 20480)})

# Measured at 32768 token rows.  The weight transpose does not shrink
# with the batch while the GEMM does, so the route keeps away from short
# GEMMs (the same floor as _TN_WGRAD_MIN_K).
_TN_DGRAD_MIN_TOK = 4096

# Experiments and tests: when >= 0, every dgrad whose weight has at least
# this many elements is routed whatever the table and the floor say.
_TN_DGRAD_MIN_ELEMS = int(os.environ.get("VITFSDP_TN_DGRAD_MIN_ELEMS", "-1"))


def _tn_dgrad_on():
    return os.environ.get("VITFSDP_TN_DGRAD", "1") != "0"


def _tn_dgrad_shapes_ok(out, inn, tok):
    """Shape gate of the TN dgrad route for dy [tok, out] @ W [out, in].
    _C.dgrad_tn needs both weight dimensions to be multiples of 8."""
    if out % 8 or inn % 8:
        return False
    if _TN_DGRAD_MIN_ELEMS >= 0:
        return out * inn >= _TN_DGRAD_MIN_ELEMS
    return (out, inn) in _TN_DGRAD_SHAPES and tok >= _TN_DGRAD_MIN_TOK


def _same_buffer(t, ref):
    """t is the tensor ref or a same-sized contiguous view of it whose
    rows have ref's length (the identity test of the parked sums)."""
    return (
        t.dtype == ref.dtype
        and t.device == ref.device
        and t.untyped_storage().data_ptr() == ref.untyped_storage().data_ptr()
        and t.storage_offset() == ref.storage_offset()
        and t.numel() == ref.numel()
        and t.dim() >= 2
        and t.shape[-1] == ref.shape[-1]
        and t.is_contiguous()
    )


def _row_sum_args(args, kwargs):
    """(t, keepdim) if this sum.dim_IntList reduces every dim but the
    last of a contiguous tensor with no dtype change, else None."""
    if kwargs.get("dtype") is not None:
        return None
    t = args[0]
    dims = args[1] if len(args) > 1 else None
    keepdim = args[2] if len(args) > 2 else kwargs.get("keepdim", False)
    if not (
        isinstance(t, torch.Tensor)
        and dims is not None
        and t.dim() >= 2
        and t.is_contiguous()
        and sorted(d % t.dim() for d in dims) == list(range(t.dim() - 1))
    ):
        return None
    return t, keepdim


def _hip_bf16(*tensors):
    """The GPU gate of both modes and every route below: all of these
    are bf16 tensors on one GPU and the extension serves them (use_hip
    raises when it is not built, so that a GPU step cannot quietly run
    without it).

    It asks more than any of the four hand-written checks it replaces and
    decides as each did on every call aten would accept: the operands of
    an mm, addmm or gelu_backward share dtype and device, so it made no
    difference that the mode-level check looked at the first operand
    only, NativeWgradMode at both dtypes but one device, and the dgrad
    route at dy.device == w.device without use_hip (the mode-level check
    ahead of it had called it).  What one kernel asks beyond the gate
    stays at its route: a 16-byte aligned W for _C.dgrad_tn, hid % 8 for
    the GELU backward."""
    dev = tensors[0].device
    return all(
        t.is_cuda and t.dtype == torch.bfloat16 and t.device == dev
        for t in tensors
    ) and use_hip(*tensors)


def _wgemm_takes(at, b):
    """mm(at, b) is a weight gradient that csrc/wgemm.hip takes."""
    return (_is_wgrad_mm(at, b) and _hip_bf16(at, b)
            and hasattr(ext(), "wgrad_gemm"))


def _wgemm(at, b):
    """dW [M, N] = at @ b by csrc/wgemm.hip, from the contiguous [K, M]
    base of at and b [K, N]."""
    (dw,) = ext().wgrad_gemm(at.t().contiguous(), b.contiguous(), False)
    return dw


class NativeWgradMode(TorchDispatchMode):
    """Reroute ONLY the dW GEMMs to csrc/wgemm.hip, below autograd.

    This is the corrected integration after the Function-path root cause
    (see module docstring): pushing a mode around ``loss.backward()``
    leaves every forward an ordinary codegen'd addmm — non-reentrant
    checkpoint early-stop keeps skipping the last recompute GEMM — and
    the mode swaps the kernel at dispatch time when AddmmBackward runs
    its mm(x^T, dy).  The engine propagates the mode into its worker
    threads via ThreadLocalState, which
    tests/test_native_wgrad_dispatch.py verifies on CPU.

    ``handler(a, b)`` (a: contiguous [K, M] base, b: contiguous [K, N],
    returns [M, N]) is a test seam; the default requires the HIP
    extension and bf16 CUDA tensors.
    """

    def __init__(self, handler=None):
        super().__init__()
        self.hits = 0
        if handler is None:
            self._takes, self._kernel = _wgemm_takes, _wgemm
        else:
            self._takes = _is_wgrad_mm
            self._kernel = lambda at, b: handler(at.t(), b)

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func is torch.ops.aten.mm.default and self._takes(*args):
            self.hits += 1
            return self._kernel(*args)
        return func(*args, **(kwargs or {}))


def _op_layout(t):
    """'N' for a row-contiguous 2-D tensor, 'T' for a transposed view of
    one, None otherwise (mirrors csrc/ltgemm.cpp classify())."""
    if t.dim() != 2:
        return None
    r, c = t.shape
    s0, s1 = t.stride()
    if s1 == 1 and (s0 == c or r == 1):
        return "N"
    if s0 == 1 and (s1 == r or c == 1):
        return "T"
    return None


def _dual_key(a, b):
    """Column-major-dual shape key for row-major a @ b, matching the
    offline search rows (csrc/tools/hipblaslt_search.cpp): the A-slot
    takes b's memory, the B-slot a's."""
    la, lb = _op_layout(a), _op_layout(b)
    if la is None or lb is None:
        return None
    return (lb, la, b.shape[1], a.shape[0], a.shape[1])


# --------------------------------------------------------------------------
# Fused MLP GELU (ROADMAP item 6 / VERDICT 3).
#
# Enabled by configure_gelu_fusion(embed_dim, hidden_dim) + the
# VITFSDP_FUSED_GELU env knob.  Mechanism (below autograd, so the stock
# addmm/gelu graph nodes — and checkpoint early-stop — are untouched):
# fc1's forward addmm runs as _C.fwd_gemm_gelu (csrc/fgemm.hip, the
# hand-written CDNA4 GEMM with an EXACT-erf GELU+bias epilogue); the
# dispatch returns the PRE-activation as the addmm result (so
# GeluBackward saves exactly what the stock graph expects) and answers
# the immediately following aten.gelu with the cached gelu output.  The
# backward is entirely stock — erf forward + erf gelu_backward, i.e.
# reference numerics up to GEMM rounding.
#
# (hipblaslt-ext's GELU_AUX/DGELU epilogues ship no algorithms for bf16
# on this ROCm 7.2 / gfx950 stack — probed on-box, r2 GPU call 2 — and
# are tanh-approx anyway; the lt_gemm_gelu / lt_gemm_dgelu_bgrad
# entries remain in csrc/ltgemm.cpp as dormant alternatives.)
# --------------------------------------------------------------------------

_GELU_CFG = {"d": 0, "hid": 0}

# minimum (M/256)*(N/256) workgroups before fc1 routes to fgemm (grid
# fill, same rationale as the wgrad gate)
_FGEMM_MIN_TILES = int(os.environ.get("VITFSDP_FGEMM_MIN_TILES", "256"))


def configure_gelu_fusion(embed_dim, hidden_dim):
    """Register the MLP dims so the dispatch mode can recognize fc1's
    forward addmm by shape.  No-op when embed == hidden (the shape key
    would be ambiguous)."""
    if embed_dim != hidden_dim:
        _GELU_CFG["d"] = int(embed_dim)
        _GELU_CFG["hid"] = int(hidden_dim)


def _gelu_fusion_on():
    return (
        os.environ.get("VITFSDP_FUSED_GELU", "0") == "1"
        and _GELU_CFG["hid"] > 0
    )


# --------------------------------------------------------------------------
# GELU backward with the fc1 bias gradient in the same pass
# (csrc/gelu.hip).  In the stock backward of linear -> gelu, GeluBackward
# writes dgelu [.., hid] and AddmmBackward then reads all of it again
# for the bias gradient:
#     gelu_backward(grad [B, T, hid], pre [B, T, hid]) -> dx
#     view(dx, [B*T, hid])
#     mm(dx2d, W) ; mm(dx2d.t(), x2d)
#     sum.dim_IntList(dx2d, [0], keepdim=True) -> [1, hid] -> view [hid]
# (sequence confirmed with a logging dispatch mode).  The hook answers
# the gelu_backward with _C.gelu_bwd_colsum, parks the column sums, and
# answers that sum from them.  On by default once the MLP dims are
# configured; VITFSDP_FUSED_DGELU_DBIAS=0 turns it off.
# --------------------------------------------------------------------------


def _dgelu_dbias_on():
    return (
        os.environ.get("VITFSDP_FUSED_DGELU_DBIAS", "1") != "0"
        and _GELU_CFG["hid"] > 0
    )


# --------------------------------------------------------------------------
# The same with hidden dropout behind the GELU (--mlp_dropout > 0).  There
# the backward of dropout(gelu(x)) is one kernel of ours
# (_C.gelu_dropout_bwd, issued by ops/dropout.py), not an aten op, and a
# dispatch mode sees aten and registered ops only.  So that backward is a
# registered op, defined here because the _OPS table of TunedGemmMode
# needs the op object; ops/dropout.py registers its implementations and
# issues it.  The route answers it with _C.gelu_dropout_bwd_colsum(_t),
# whose dx is bit-identical, and parks (dx, colsum, dx^T) in the stash of
# the p = 0 route, so that the bias sum and the TN GEMM find it as they
# find gelu_bwd_colsum's.  The same switch turns both off.
# --------------------------------------------------------------------------

# Whether the route uses _C.gelu_dropout_bwd_colsum_t where fc1's weight
# gradient takes the TN route.  Off: at (32768, 20480), p = 0.1 that
# kernel took 1.37-1.43 ms against 1.42-1.49 ms for gelu_dropout_bwd +
# transpose_colsum, a lead smaller than the spread of either between
# series (profiles/PROFILES.md "Hidden dropout"), and the plain kernel
# followed by transpose2d would read dx once more than those two.  So at
# such a shape the route declines and the two-pass sequence runs;
# everywhere else (and with VITFSDP_TN_DGELU_T=0) it is the plain kernel,
# which won by 13 %.
_DGELU_DROP_T = False

_LIB = torch.library.Library("vitfsdp", "DEF")
_LIB.define(
    "gelu_dropout_bwd(Tensor dy, Tensor x, float p, int seed) -> Tensor")


# --------------------------------------------------------------------------
# The extension kernels behind the routes of TunedGemmMode, under the
# names of its test seams.  A missing kernel is an error here, not a
# fallback.
# --------------------------------------------------------------------------


def _lt_gemm(a, b, idx, bias):
    """a @ b (+ bias) by hipBLASLt algorithm idx, -1 for its heuristic."""
    return ext().lt_gemm(a, b, idx, bias)


def _gelu_bwd_colsum(dy, x, want_t):
    """(dx, bf16 column sums of dx, dx^T contiguous or None)."""
    if want_t:
        return ext().gelu_bwd_colsum_t(dy, x)
    dx, colsum = ext().gelu_bwd_colsum(dy, x)
    return dx, colsum, None


def _gelu_dropout_bwd_colsum(dy, x, p, seed, want_t):
    """_gelu_bwd_colsum for the backward of dropout(gelu(x)) under the
    hash mask of (seed, p)."""
    if want_t:
        return ext().gelu_dropout_bwd_colsum_t(dy, x, p, seed)
    dx, colsum = ext().gelu_dropout_bwd_colsum(dy, x, p, seed)
    return dx, colsum, None


def _transposed(t, want_colsum):
    """(t^T contiguous, bf16 column sums of t or None)."""
    if want_colsum:
        tt, colsum = ext().transpose_colsum(t)
        return tt, colsum
    return ext().transpose2d(t), None


def _dgrad_tn(dy, w, idx):
    """dy @ w as the TN GEMM idx on w^T."""
    return ext().dgrad_tn(dy, w, idx)


_KERNELS = {"gemm": _lt_gemm, "dgelu": _gelu_bwd_colsum,
            "dgelu_drop": _gelu_dropout_bwd_colsum,
            "transpose": _transposed, "dgrad": _dgrad_tn}

# what an op method of TunedGemmMode returns for "not mine: run the stock op"
_STOCK = object()


class TunedGemmMode(TorchDispatchMode):
    """Reroute training GEMMs whose shape has an offline-searched
    hipBLASLt algorithm (tuned/lt_algos_gfx950.json) through
    _C.lt_gemm with the explicit index — same library, better kernel
    pick than the heuristic (ROADMAP item 5).  Dispatcher-level like
    NativeWgradMode, so the autograd graph keeps its stock addmm/mm
    nodes and non-reentrant checkpoint early-stop is preserved.

    Also hosts the native-wgrad reroute when VITFSDP_NATIVE_WGRAD=2, the
    TN weight-gradient route (which takes precedence at the shapes in
    its gate), the TN input-gradient route (_C.dgrad_tn, ahead of the
    tuned N,N index at the shapes in its gate) and the fused MLP GELU
    epilogues when configured, so one mode covers the whole step (push
    around forward AND backward).

    __torch_dispatch__ looks the op up in _OPS; the method found there
    tries its routes in the order written and answers the op, or returns
    _STOCK and the stock op runs.  Every kernel is called through _call
    and every route asks _takes whether the tensors are its kernel's, so
    the constructor's handlers (fakes of the kernels in _KERNELS) are
    consulted in those two places.
    """

    def __init__(self, table=None, native_wgrad=None, handler=None,
                 dgelu_handler=None, tn_handler=None, dgrad_handler=None,
                 *, dgelu_drop_handler=None):
        super().__init__()
        self.table = lt_algo_table() if table is None else table
        self.native_wgrad = (
            _NATIVE_WGRAD_DISPATCH if native_wgrad is None else native_wgrad
        )
        # test seams: a fake under a name of _KERNELS replaces that kernel
        # and lifts the GPU gate for it, so that the routing logic runs
        # on the CPU.  Signatures as in _KERNELS, except that the dgelu
        # fake is dgelu_handler(dy, x) -> (dx, colsum) and the dgelu_drop
        # fake dgelu_drop_handler(dy, x, p, seed) -> (dx, colsum), and
        # that the gemm fake also stands in for _C.fwd_gemm_gelu when
        # called with idx == "gelu" (-> (gelu output, pre-activation)).
        fakes = {"gemm": handler, "dgelu": dgelu_handler,
                 "dgelu_drop": dgelu_drop_handler,
                 "transpose": tn_handler, "dgrad": dgrad_handler}
        self._fakes = {k: f for k, f in fakes.items() if f is not None}

        def on(switch, name=None):
            # a route whose own kernel is not faked is off when the GEMM
            # is: the real kernel could not take the fake GEMM's tensors
            return switch and (name in self._fakes
                               or "gemm" not in self._fakes)

        self.hits = 0
        self._wgemm_on = on(self.native_wgrad)  # no seam of its own
        self.wgrad_hits = 0
        # fused-GELU state (see module comment above):
        self.fused_gelu = _gelu_fusion_on()
        # pre-act data_ptr -> (pre-act, gelu_out), transient.  The entry
        # holds the pre-activation itself so its address cannot be freed
        # and handed to another tensor while the key is live.
        self._pending_gelu = {}
        self.gelu_hits = 0
        # fused dgelu + fc1 bias gradient (see module comment above)
        self.fused_dgelu = on(_dgelu_dbias_on(), "dgelu")
        # the same behind hidden dropout (vitfsdp::gelu_dropout_bwd)
        self.fused_dgelu_drop = on(_dgelu_dbias_on(), "dgelu_drop")
        # (dx, colsum, dx^T or None) of either route: at most one entry
        self._dgelu_stash = None
        self.dgelu_hits = 0
        self.dgelu_drop_hits = 0
        self.dbias_hits = 0
        # TN weight gradients (see module comment above); the GEMM goes
        # through the gemm seam
        self.tn_wgrad = on(_tn_wgrad_on(), "transpose")
        # (dy, colsum, dyT), at most one entry, holding dy so that its
        # address cannot be recycled.  After the GEMM: colsum waits for
        # the bias sum, dyT is None.  After a bias sum that came first:
        # dyT waits for the GEMM, colsum is None.
        self._tn_stash = None
        self.tn_dgelu_t = self.tn_wgrad and _tn_dgelu_t_on()
        # set by the first routed GEMM that found no dy^T parked: the
        # sums follow their GEMMs here and none needs a pass of its own
        self._tn_mm_first = False
        self.tn_hits = 0
        self.tn_dbias_hits = 0
        # TN input gradients (see module comment above)
        self.tn_dgrad = on(_tn_dgrad_on(), "dgrad")
        self.tn_dgrad_hits = 0

    def __exit__(self, exc_type, exc_val, exc_tb):
        self._dgelu_stash = None
        self._tn_stash = None
        return super().__exit__(exc_type, exc_val, exc_tb)

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        op = self._OPS.get(func)
        if op is not None:
            out = op(self, args, kwargs)
            if out is not _STOCK:
                return out
        return func(*args, **kwargs)

    def _call(self, name, *args):
        """The fake under this seam name if there is one, else the
        extension's kernel."""
        return self._fakes.get(name, _KERNELS[name])(*args)

    def _takes(self, name, *tensors, kernel_ok=True):
        """Whether the route that ends in this seam may take these
        tensors: it is faked, or they pass the GPU gate and what the real
        kernel asks beyond it (``kernel_ok``), which a fake does not."""
        return name in self._fakes or (kernel_ok and _hip_bf16(*tensors))

    def _tuned_index(self, key):
        return self.table.get(key) if self.table and key is not None else None

    # -- the ops, each with its routes in order of precedence ---------------

    def _mm(self, args, kwargs):
        a, b = args
        # asked once for every route below: TN wgrad and the tuned index
        # end in the GEMM seam, and wgemm and TN dgrad ask the same of
        # the same two tensors
        if not self._takes("gemm", a, b):
            return _STOCK
        if self.tn_wgrad and _is_tn_wgrad_mm(a, b):
            return self._tn_wgrad(a, b)
        if self._wgemm_on and _wgemm_takes(a, b):
            self.wgrad_hits += 1
            return _wgemm(a, b)
        if self.tn_dgrad and self._is_tn_dgrad_mm(a, b):
            return self._tn_dgrad(a, b)
        idx = self._tuned_index(_dual_key(a, b))
        if idx is None:
            return _STOCK
        self.hits += 1
        return self._call("gemm", a, b, idx, None)

    def _addmm(self, args, kwargs):
        if not (
            len(args) == 3
            and kwargs.get("beta", 1) == 1
            and kwargs.get("alpha", 1) == 1
            and args[0].dim() == 1
            and self._takes("gemm", *args)
        ):
            return _STOCK
        bias, a, b = args
        key = _dual_key(a, b)
        if (
            self.fused_gelu
            and self._is_fc1_fwd(key)
            and ("gemm" in self._fakes or hasattr(ext(), "fwd_gemm_gelu"))
        ):
            return self._fused_fc1_fwd(a, b, bias)
        idx = self._tuned_index(key)
        if idx is None:
            return _STOCK
        self.hits += 1
        return self._call("gemm", a, b, idx, bias)

    def _gelu(self, args, kwargs):
        if self.fused_gelu:
            _, out = self._pending_gelu.pop(args[0].data_ptr(), (None, None))
            if out is not None and out.shape == args[0].shape:
                return out
        return _STOCK

    def _gelu_backward(self, args, kwargs):
        if self.fused_dgelu and self._is_mlp_dgelu(args, kwargs):
            return self._fused_dgelu(*args)
        return _STOCK

    def _gelu_dropout_bwd(self, args, kwargs):
        if (self.fused_dgelu_drop and len(args) == 4 and not kwargs
                and self._is_mlp_dgelu_pair("dgelu_drop", *args[:2])
                # see _DGELU_DROP_T: dx^T is wanted, and that kernel is
                # not routed
                and (_DGELU_DROP_T or not self._wants_dgelu_t(args[0]))):
            return self._fused_dgelu_drop(*args)
        return _STOCK  # the implementation ops/dropout.py registered

    def _take_parked(self, stash, t):
        """The column sums parked in that stash if t is the tensor they
        were taken from (which empties the stash), else None."""
        st = getattr(self, stash)
        if st is None or st[1] is None or not _same_buffer(t, st[0]):
            return None
        setattr(self, stash, None)
        return st[1]

    def _sum(self, args, kwargs):
        """A bias gradient whose column sums a kernel of ours has made
        already, or, when the sum comes before its TN GEMM, makes here."""
        if self._dgelu_stash is None and not self.tn_wgrad:
            return _STOCK
        rs = _row_sum_args(args, kwargs)
        if rs is None:
            return _STOCK
        t, keepdim = rs
        colsum = self._take_parked("_dgelu_stash", t)
        if colsum is not None:
            self.dbias_hits += 1
        else:
            colsum = self._take_parked("_tn_stash", t)
            if (
                colsum is None
                and self.tn_wgrad
                and not self._tn_mm_first
                and t.dim() == 2
                and self._takes("gemm", t)
                and _tn_wgrad_out_ok(t.shape[1], t.shape[0])
            ):
                # the GEMM's other operand is not known yet, so this goes by
                # dy's shape alone; a GEMM outside the gate leaves dy^T unused
                dyT, colsum = self._call("transpose", t, True)
                self._tn_stash = (t, None, dyT)
            if colsum is None:
                return _STOCK
            self.tn_dbias_hits += 1
        if keepdim:
            return colsum.view([1] * (t.dim() - 1) + [t.shape[-1]])
        return colsum

    # what __torch_dispatch__ looks an op up in (a class-level table of
    # plain functions: a per-mode table of bound methods would tie every
    # mode into a reference cycle)
    _OPS = {
        torch.ops.aten.mm.default: _mm,
        torch.ops.aten.addmm.default: _addmm,
        torch.ops.aten.gelu.default: _gelu,
        torch.ops.aten.gelu_backward.default: _gelu_backward,
        torch.ops.vitfsdp.gelu_dropout_bwd.default: _gelu_dropout_bwd,
        torch.ops.aten.sum.dim_IntList: _sum,
    }

    # -- fused-GELU helpers -------------------------------------------------

    def _is_fc1_fwd(self, key):
        if not (
            key is not None
            and key[0] == "T" and key[1] == "N"
            and key[2] == _GELU_CFG["hid"] and key[4] == _GELU_CFG["d"]
        ):
            return False
        if "gemm" in self._fakes:
            return True  # the fake has no kernel shape limits
        hid, tok = key[2], key[3]
        return (
            tok % 256 == 0 and hid % 256 == 0 and key[4] % 64 == 0
            and (tok // 256) * (hid // 256) >= _FGEMM_MIN_TILES
        )

    def _fused_fc1_fwd(self, a, b, bias):
        if "gemm" in self._fakes:  # stands in for fwd_gemm_gelu
            out, pre = self._fakes["gemm"](a, b, "gelu", bias)
        else:
            # b is the transposed view of fc1's weight [hid, d]: b.t()
            # IS the weight, row-major contiguous — fgemm reads it
            # directly (W [N, K], K contiguous)
            out, pre = ext().fwd_gemm_gelu(
                a.contiguous(), b.t().contiguous(), bias
            )
        self.gelu_hits += 1
        if len(self._pending_gelu) > 4:  # unconsumed strays (shouldn't happen)
            self._pending_gelu.clear()
        self._pending_gelu[pre.data_ptr()] = (pre, out)
        return pre

    # -- fused dgelu + bias-gradient helpers --------------------------------

    def _is_mlp_dgelu(self, args, kwargs):
        if len(args) != 2 or kwargs.get("approximate", "none") != "none":
            return False
        return self._is_mlp_dgelu_pair("dgelu", *args)

    def _is_mlp_dgelu_pair(self, name, dy, x):
        """dy and x are those of the MLP's GELU backward, and the kernel
        behind this seam name takes them."""
        if not (
            dy.dim() >= 2
            and dy.shape[-1] == _GELU_CFG["hid"]
            and dy.shape == x.shape
            and dy.is_contiguous() and x.is_contiguous()
        ):
            return False
        # the kernel's rows are 16-byte vectors
        return self._takes(name, dy, x, kernel_ok=dy.shape[-1] % 8 == 0)

    def _wants_dgelu_t(self, dy):
        """fc1's weight gradient will take the TN route and expects dx^T
        from the GELU backward."""
        hid = dy.shape[-1]
        return self.tn_dgelu_t and _tn_wgrad_shapes_ok(
            hid, _GELU_CFG["d"], dy.numel() // hid)

    def _dgelu_kernel(self, name, dy, x, *mask):
        """The kernel or the fake under this seam name, with dx^T if fc1's
        weight gradient will take the TN route; parks what it returns."""
        hid = dy.shape[-1]
        want_t = self._wants_dgelu_t(dy)
        if name in self._fakes:  # (dx, colsum) only: dx^T in torch
            dx, colsum = self._fakes[name](dy, x, *mask)
            dxt = dx.reshape(-1, hid).t().contiguous() if want_t else None
        else:
            dx, colsum, dxt = _KERNELS[name](dy, x, *mask, want_t)
        # holding dx keeps its address from being recycled while the
        # entry lives; the next GELU backward overwrites it
        self._dgelu_stash = (dx, colsum, dxt)
        return dx

    def _fused_dgelu(self, dy, x):
        dx = self._dgelu_kernel("dgelu", dy, x)
        self.dgelu_hits += 1
        return dx

    def _fused_dgelu_drop(self, dy, x, p, seed):
        dx = self._dgelu_kernel("dgelu_drop", dy, x, float(p), int(seed))
        self.dgelu_drop_hits += 1
        return dx

    # -- TN weight-gradient helpers ------------------------------------------

    def _tn_wgrad(self, at, x):
        """dW [out, in] contiguous = lt_gemm(dy^T, (x^T).t()).  The two
        transposes live only until the GEMM is queued."""
        dy = at.t()  # the contiguous [K, out] base
        st, self._tn_stash = self._tn_stash, None
        if st is not None and st[2] is not None and _same_buffer(dy, st[0]):
            dyT = st[2]  # its bias sum came first and did the pass
        else:
            # on this torch the GEMM comes first: stop guessing at sums
            self._tn_mm_first = True
            if self._dgelu_stash is not None and _same_buffer(
                    dy, self._dgelu_stash[0]):
                # fc1: dy is the GELU backward's result, whose column
                # sums that kernel has parked already, with dy^T if it
                # was told to write it
                dx, colsum, dyT = self._dgelu_stash
                if dyT is None:
                    dyT, _ = self._call("transpose", dy, False)
                else:
                    self._dgelu_stash = (dx, colsum, None)
            else:
                dyT, colsum = self._call("transpose", dy, True)
                self._tn_stash = (dy, colsum, None)
        xT, _ = self._call("transpose", x, False)
        b = xT.t()
        idx = self._tuned_index(_dual_key(dyT, b))
        self.tn_hits += 1
        return self._call("gemm", dyT, b, -1 if idx is None else idx, None)

    # -- TN input-gradient helpers -------------------------------------------

    def _is_tn_dgrad_mm(self, dy, w):
        """mm(dy [tok, out], W [out, in]) with both operands row-contiguous
        (a weight gradient's first operand is a transposed view, a
        forward's second one is), at a gated shape, and nothing that
        _C.dgrad_tn would refuse."""
        if _op_layout(dy) != "N" or _op_layout(w) != "N":
            return False
        if dy.shape[1] != w.shape[0] or w.data_ptr() % 16:
            return False
        if not _tn_dgrad_shapes_ok(w.shape[0], w.shape[1], dy.shape[0]):
            return False
        return self._takes("dgrad", dy, w)

    def _tn_dgrad(self, dy, w):
        """dx = dy @ W as the TN GEMM on W^T, which _C.dgrad_tn writes
        and drops.  That GEMM is lt_gemm(dy, wT.t()), so its tuned index
        is the one under the dual key of a forward with these sizes."""
        out, inn = w.shape
        idx = self._tuned_index(("T", "N", inn, dy.shape[0], out))
        self.tn_dgrad_hits += 1
        return self._call("dgrad", dy, w, -1 if idx is None else idx)


def gemm_dispatch_context():
    """Context manager for the training step (forward and backward):
    activates the dispatcher-level GEMM rerouting when the tuned
    algorithm table is present, fused MLP GELU or the fused
    dgelu + bias-gradient pass is configured, or VITFSDP_NATIVE_WGRAD=2;
    otherwise a no-op.  The TN weight-gradient route (VITFSDP_TN_WGRAD)
    lives in TunedGemmMode and is active whenever that mode is; it does
    not bring the mode up on its own: with the tuned table disabled and
    the fused dgelu off, the step is the plain NativeWgradMode one."""
    if lt_algo_table() or _gelu_fusion_on() or _dgelu_dbias_on():
        return TunedGemmMode()
    if _NATIVE_WGRAD_DISPATCH:
        return NativeWgradMode()  # backward-compatible, wgrad only
    return contextlib.nullcontext()


class NativeLinear(nn.Linear):
    """Drop-in nn.Linear that routes the weight gradient through the
    native wgrad kernel when VITFSDP_NATIVE_WGRAD=1 and the shape
    qualifies (identical state_dict keys and initialization).

    When the native path is disabled it falls back to stock autograd
    entirely: a within-box A/B showed the custom Function with the
    LIBRARY wgrad formulation costs ~126 ms/step at ViT-10B — torch's
    own matmul backward picks a faster dW GEMM layout than the explicit
    dy^T @ x call — so there is no reason to take the Function without
    the native kernel."""

    def forward(self, x):
        if _NATIVE_WGRAD:
            return _NativeLinearFn.apply(x, self.weight, self.bias)
        return F.linear(x, self.weight, self.bias)
