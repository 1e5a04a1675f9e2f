"""One whole training step under the dispatch modes of ops/linear.py on
the CPU, pinned to literals: two checkpointed blocks (attention-shaped
and MLP-shaped residual halves of plain F.linear / F.gelu), forward and
backward under ONE mode, with every kernel seam of TunedGemmMode faked
by a logging stand-in.  What is compared is the sequence of kernel calls
the routes make, the aten ops that reach the backend, and every hit
counter, so any change of route precedence, gate or stash handling
shows as a diff against the lists at the end of this file.  The lists
were recorded from the code as it stood before the dispatch half of
ops/linear.py was restructured into an op table.

The per-route tests (test_tn_wgrad_dispatch.py, test_tn_dgrad_dispatch.py,
test_dgelu_dbias_dispatch.py, test_fused_gelu_dispatch.py,
test_tuned_gemm.py, test_native_wgrad_dispatch.py) cover each route
alone; this one covers them together, in the order a step runs them."""

import functools

import pytest
import torch
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils.checkpoint import checkpoint

from vit_10b_fsdp_example_amd.ops import linear as linmod

# pairwise distinct widths, so that no shape key is ambiguous (with
# HID == QKV the qkv forward would be taken for fc1)
ROWS, D, QKV, HID = (2, 8), 8, 24, 32
TOK = ROWS[0] * ROWS[1]

COUNTERS = ("hits", "wgrad_hits", "gelu_hits", "dgelu_hits", "dbias_hits",
            "tn_hits", "tn_dbias_hits", "tn_dgrad_hits")

# the qkv forward, the fc2 forward (which is also the key the TN dgrad of
# fc1 looks up), and the N,N key of qkv's input gradient, which belongs
# to the tuned-index path and must not be used while the dgrad route
# takes that mm
TABLE = {
    ("T", "N", QKV, TOK, D): 101,
    ("T", "N", D, TOK, HID): 202,
    ("N", "N", D, TOK, QKV): 303,
}


class _Fakes:
    """Fake kernels for the four seams that log what is asked of them."""

    def __init__(self):
        self.log = []

    def gemm(self, a, b, idx, bias):
        self.log.append(("gemm", linmod._op_layout(a), linmod._op_layout(b),
                         tuple(a.shape), tuple(b.shape), idx,
                         bias is not None))
        out = torch.mm(a, b)
        out = out + bias if bias is not None else out
        return (F.gelu(out), out) if idx == "gelu" else out

    def transpose(self, t, want_colsum):
        self.log.append(("transpose", tuple(t.shape), want_colsum))
        return t.t().contiguous(), (t.sum(0) if want_colsum else None)

    def dgelu(self, dy, x):
        self.log.append(("dgelu", tuple(dy.shape)))
        dx = torch.ops.aten.gelu_backward(dy, x, approximate="none")
        return dx, dx.reshape(-1, dx.shape[-1]).sum(0)

    def dgrad(self, dy, w, idx):
        self.log.append(("dgrad", tuple(dy.shape), tuple(w.shape), idx))
        return torch.mm(dy, w)


class _OpLog(TorchDispatchMode):
    """Outer mode: the aten ops that reach the backend, as names without
    the "aten." prefix and the ".default" suffix."""

    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.ops.append(
            str(func).removeprefix("aten.").removesuffix(".default"))
        return func(*args, **(kwargs or {}))


def _model(rows, d, qkv, hid):
    """(input, parameters of two blocks), weights scaled to keep the
    activations of order one."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(*rows, d, generator=g, requires_grad=True)
    blocks = []
    for _ in range(2):
        p = []
        for out, inn in ((qkv, d), (d, qkv), (hid, d), (d, hid)):
            w = torch.randn(out, inn, generator=g) * inn ** -0.5
            p += [w.requires_grad_(True),
                  torch.randn(out, generator=g, requires_grad=True)]
        blocks.append(p)
    return x, blocks


def _block(t, p):
    t = t + F.linear(F.linear(t, p[0], p[1]), p[2], p[3])
    return t + F.linear(F.gelu(F.linear(t, p[4], p[5])), p[6], p[7])


def _step(x, blocks, mode):
    """Forward and backward of both checkpointed blocks under ``mode``;
    returns the backend op names and the gradients."""
    leaves = [x] + [t for p in blocks for t in p]
    for t in leaves:
        t.grad = None
    log = _OpLog()
    with log, mode:
        t = x
        for p in blocks:
            t = checkpoint(functools.partial(_block, p=p), t,
                           use_reentrant=False)
        t.pow(2).sum().backward()
    return log.ops, [t.grad.clone() for t in leaves]


class _NoMode:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _assert_same_grads(got, ref):
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5), a.shape


@pytest.mark.parametrize("fused_gelu", [0, 1])
def test_tuned_mode_step_trace(monkeypatch, fused_gelu):
    for knob in ("VITFSDP_TN_WGRAD", "VITFSDP_TN_DGRAD",
                 "VITFSDP_TN_DGELU_T", "VITFSDP_FUSED_DGELU_DBIAS"):
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setenv("VITFSDP_FUSED_GELU", str(fused_gelu))
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", 0)
    monkeypatch.setattr(linmod, "_TN_DGRAD_MIN_ELEMS", 0)
    monkeypatch.setitem(linmod._GELU_CFG, "d", D)
    monkeypatch.setitem(linmod._GELU_CFG, "hid", HID)

    x, blocks = _model(ROWS, D, QKV, HID)
    _, ref = _step(x, blocks, _NoMode())
    fakes = _Fakes()
    mode = linmod.TunedGemmMode(
        table=dict(TABLE), native_wgrad=False, handler=fakes.gemm,
        dgelu_handler=fakes.dgelu, tn_handler=fakes.transpose,
        dgrad_handler=fakes.dgrad)
    ops, grads = _step(x, blocks, mode)

    assert fakes.log == KERNEL_CALLS[fused_gelu]
    assert ops == BACKEND_OPS[fused_gelu].split()
    assert {c: getattr(mode, c) for c in COUNTERS} == {
        "hits": 6, "wgrad_hits": 0, "gelu_hits": 4 * fused_gelu,
        "dgelu_hits": 2, "dbias_hits": 2, "tn_hits": 8,
        "tn_dbias_hits": 6, "tn_dgrad_hits": 8,
    }
    assert mode._tn_stash is None and mode._dgelu_stash is None
    _assert_same_grads(grads, ref)


def test_native_wgrad_mode_step_trace(monkeypatch):
    """The same model under NativeWgradMode, at widths its shape gate
    takes (multiples of 256, 64 token rows)."""
    monkeypatch.setattr(linmod, "_MIN_TILES", 0)
    x, blocks = _model((2, 32), 256, 768, 512)
    _, ref = _step(x, blocks, _NoMode())
    calls = []

    def handler(a, b):
        calls.append((tuple(a.shape), tuple(b.shape)))
        return a.t() @ b

    mode = linmod.NativeWgradMode(handler=handler)
    ops, grads = _step(x, blocks, mode)
    assert mode.hits == 8  # four weight gradients per block
    # backward runs the second block first, each block's MLP half first;
    # a: the [K, M] base of dy, b: x [K, N]
    assert calls == 2 * [((64, 256), (64, 512)), ((64, 512), (64, 256)),
                         ((64, 256), (64, 768)), ((64, 768), (64, 256))]
    assert ops == NATIVE_WGRAD_BACKEND_OPS.split()
    _assert_same_grads(grads, ref)


# ---- recorded literals ----------------------------------------------------

KERNEL_CALLS = {
    0: [
        ("gemm", "N", "T", (16, 8), (8, 24), 101, True),
        ("gemm", "N", "T", (16, 32), (32, 8), 202, True),
        ("gemm", "N", "T", (16, 8), (8, 24), 101, True),
        ("gemm", "N", "T", (16, 32), (32, 8), 202, True),
        ("gemm", "N", "T", (16, 8), (8, 24), 101, True),
        ("dgrad", (16, 8), (8, 32), -1),
        ("transpose", (16, 8), True),
        ("transpose", (16, 32), False),
        ("gemm", "N", "T", (8, 16), (16, 32), -1, False),
        ("dgelu", (2, 8, 32)),
        ("dgrad", (16, 32), (32, 8), 202),
        ("transpose", (16, 8), False),
        ("gemm", "N", "T", (32, 16), (16, 8), -1, False),
        ("dgrad", (16, 8), (8, 24), 101),
        ("transpose", (16, 8), True),
        ("transpose", (16, 24), False),
        ("gemm", "N", "T", (8, 16), (16, 24), -1, False),
        ("dgrad", (16, 24), (24, 8), -1),
        ("transpose", (16, 24), True),
        ("transpose", (16, 8), False),
        ("gemm", "N", "T", (24, 16), (16, 8), -1, False),
        ("gemm", "N", "T", (16, 8), (8, 24), 101, True),
        ("dgrad", (16, 8), (8, 32), -1),
        ("transpose", (16, 8), True),
        ("transpose", (16, 32), False),
        ("gemm", "N", "T", (8, 16), (16, 32), -1, False),
        ("dgelu", (2, 8, 32)),
        ("dgrad", (16, 32), (32, 8), 202),
        ("transpose", (16, 8), False),
        ("gemm", "N", "T", (32, 16), (16, 8), -1, False),
        ("dgrad", (16, 8), (8, 24), 101),
        ("transpose", (16, 8), True),
        ("transpose", (16, 24), False),
        ("gemm", "N", "T", (8, 16), (16, 24), -1, False),
        ("dgrad", (16, 24), (24, 8), -1),
        ("transpose", (16, 24), True),
        ("transpose", (16, 8), False),
        ("gemm", "N", "T", (24, 16), (16, 8), -1, False),
    ],
    1: [
        ("gemm", "N", "T", (16, 8), (8, 24), 101, True),
        ("gemm", "N", "T", (16, 8), (8, 32), "gelu", True),
        ("gemm", "N", "T", (16, 32), (32, 8), 202, True),
        ("gemm", "N", "T", (16, 8), (8, 24), 101, True),
        ("gemm", "N", "T", (16, 8), (8, 32), "gelu", True),
        ("gemm", "N", "T", (16, 32), (32, 8), 202, True),
        ("gemm", "N", "T", (16, 8), (8, 24), 101, True),
        ("gemm", "N", "T", (16, 8), (8, 32), "gelu", True),
        ("dgrad", (16, 8), (8, 32), -1),
        ("transpose", (16, 8), True),
        ("transpose", (16, 32), False),
        ("gemm", "N", "T", (8, 16), (16, 32), -1, False),
        ("dgelu", (2, 8, 32)),
        ("dgrad", (16, 32), (32, 8), 202),
        ("transpose", (16, 8), False),
        ("gemm", "N", "T", (32, 16), (16, 8), -1, False),
        ("dgrad", (16, 8), (8, 24), 101),
        ("transpose", (16, 8), True),
        ("transpose", (16, 24), False),
        ("gemm", "N", "T", (8, 16), (16, 24), -1, False),
        ("dgrad", (16, 24), (24, 8), -1),
        ("transpose", (16, 24), True),
        ("transpose", (16, 8), False),
        ("gemm", "N", "T", (24, 16), (16, 8), -1, False),
        ("gemm", "N", "T", (16, 8), (8, 24), 101, True),
        ("gemm", "N", "T", (16, 8), (8, 32), "gelu", True),
        ("dgrad", (16, 8), (8, 32), -1),
        ("transpose", (16, 8), True),
        ("transpose", (16, 32), False),
        ("gemm", "N", "T", (8, 16), (16, 32), -1, False),
        ("dgelu", (2, 8, 32)),
        ("dgrad", (16, 32), (32, 8), 202),
        ("transpose", (16, 8), False),
        ("gemm", "N", "T", (32, 16), (16, 8), -1, False),
        ("dgrad", (16, 8), (8, 24), 101),
        ("transpose", (16, 8), True),
        ("transpose", (16, 24), False),
        ("gemm", "N", "T", (8, 16), (16, 24), -1, False),
        ("dgrad", (16, 24), (24, 8), -1),
        ("transpose", (16, 24), True),
        ("transpose", (16, 8), False),
        ("gemm", "N", "T", (24, 16), (16, 8), -1, False),
    ],
}

BACKEND_OPS = {
    0: """
empty.memory_format empty.memory_format view t mm add.Tensor view view t
addmm view add.Tensor view t addmm view gelu view t mm add.Tensor view
add.Tensor empty.memory_format empty.memory_format view t mm add.Tensor view
view t addmm view add.Tensor view t addmm view gelu view t mm add.Tensor
view add.Tensor pow.Tensor_Scalar sum ones_like expand pow.Tensor_Scalar
mul.Scalar mul.Tensor view view t detach detach mm add.Tensor view view t
detach detach addmm view add.Tensor view t detach detach addmm view detach
gelu view t detach detach detach detach t mm t t t contiguous
sum.dim_IntList t contiguous t mm t view view detach t detach view detach
gelu_backward reshape sum.dim_IntList reshape t contiguous view detach
detach t mm t t t contiguous t mm t view view detach t detach view
add.Tensor view detach detach t mm t t t contiguous sum.dim_IntList t
contiguous t mm t view view detach t detach view view detach detach t mm t t
t contiguous sum.dim_IntList t contiguous t mm t view view detach t detach
view add.Tensor view view t detach detach mm add.Tensor view view t detach
detach addmm view add.Tensor view t detach detach addmm view detach gelu
view t detach detach detach detach t mm t t t contiguous sum.dim_IntList t
contiguous t mm t view view detach t detach view detach gelu_backward
reshape sum.dim_IntList reshape t contiguous view detach detach t mm t t t
contiguous t mm t view view detach t detach view add.Tensor view detach
detach t mm t t t contiguous sum.dim_IntList t contiguous t mm t view view
detach t detach view view detach detach t mm t t t contiguous
sum.dim_IntList t contiguous t mm t view view detach t detach view
add.Tensor detach
""",
    1: """
empty.memory_format empty.memory_format view t mm add.Tensor view view t
addmm view add.Tensor view t mm add.Tensor gelu view gelu view t mm
add.Tensor view add.Tensor empty.memory_format empty.memory_format view t mm
add.Tensor view view t addmm view add.Tensor view t mm add.Tensor gelu view
gelu view t mm add.Tensor view add.Tensor pow.Tensor_Scalar sum ones_like
expand pow.Tensor_Scalar mul.Scalar mul.Tensor view view t detach detach mm
add.Tensor view view t detach detach addmm view add.Tensor view t detach
detach mm add.Tensor gelu view detach gelu view t detach detach detach
detach t mm t t t contiguous sum.dim_IntList t contiguous t mm t view view
detach t detach view detach gelu_backward reshape sum.dim_IntList reshape t
contiguous view detach detach t mm t t t contiguous t mm t view view detach
t detach view add.Tensor view detach detach t mm t t t contiguous
sum.dim_IntList t contiguous t mm t view view detach t detach view view
detach detach t mm t t t contiguous sum.dim_IntList t contiguous t mm t view
view detach t detach view add.Tensor view view t detach detach mm add.Tensor
view view t detach detach addmm view add.Tensor view t detach detach mm
add.Tensor gelu view detach gelu view t detach detach detach detach t mm t t
t contiguous sum.dim_IntList t contiguous t mm t view view detach t detach
view detach gelu_backward reshape sum.dim_IntList reshape t contiguous view
detach detach t mm t t t contiguous t mm t view view detach t detach view
add.Tensor view detach detach t mm t t t contiguous sum.dim_IntList t
contiguous t mm t view view detach t detach view view detach detach t mm t t
t contiguous sum.dim_IntList t contiguous t mm t view view detach t detach
view add.Tensor detach
""",
}

NATIVE_WGRAD_BACKEND_OPS = """
empty.memory_format empty.memory_format view t addmm view view t addmm view
add.Tensor view t addmm view gelu view t addmm view add.Tensor
empty.memory_format empty.memory_format view t addmm view view t addmm view
add.Tensor view t addmm view gelu view t addmm view add.Tensor
pow.Tensor_Scalar sum ones_like expand pow.Tensor_Scalar mul.Scalar
mul.Tensor view view t detach detach addmm view view t detach detach addmm
view add.Tensor view t detach detach addmm view detach gelu view t detach
detach detach detach t mm t t t matmul t sum.dim_IntList view detach t
detach view detach gelu_backward view detach detach t mm t t t matmul t
sum.dim_IntList view detach t detach view add.Tensor view detach detach t mm
t t t matmul t sum.dim_IntList view detach t detach view view detach detach
t mm t t t matmul t sum.dim_IntList view detach t detach view add.Tensor
view view t detach detach addmm view view t detach detach addmm view
add.Tensor view t detach detach addmm view detach gelu view t detach detach
detach detach t mm t t t matmul t sum.dim_IntList view detach t detach view
detach gelu_backward view detach detach t mm t t t matmul t sum.dim_IntList
view detach t detach view add.Tensor view detach detach t mm t t t matmul t
sum.dim_IntList view detach t detach view view detach detach t mm t t t
matmul t sum.dim_IntList view detach t detach view add.Tensor detach
"""
