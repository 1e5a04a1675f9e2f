"""Flash attention (csrc/fmha.hip: forward, bwd_dq, bwd_dkv, row dot)
against an fp64 reference, with bounds from a rounding model instead of
fixed tolerances (tests/fmha_reference.py explains the scheme).

Every case runs the forward and then the backward on the kernel's own o
and lse, and checks o, lse, dq, dk and dv.  B = 2, H = 3: a head count
that is no power of two, so bh / H, bh % H and both stride sets matter.
All twelve dispatched head dims appear, with and without dropout, in both
layouts."""

import importlib

import pytest
import torch

from tests.fmha_reference import (
    HEAD_DIMS, _U, assert_family_stress, check_kernel_outputs, keep_mask,
    make_inputs,
)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None

B, H = 2, 3
DROP_SEED = 98765


def _dev():
    return torch.device("cuda", 0)


def _to_qkv(q, k, v, do):
    """[B,H,T,D] q, k, v, do -> contiguous qkv [B,T,3,H,D], do [B,T,H*D]."""
    b, h, t, d = q.shape
    qkv = torch.stack([x.transpose(1, 2) for x in (q, k, v)], dim=2)
    return qkv.contiguous(), do.transpose(1, 2).reshape(b, t, h * d)


def _from_qkv(o, dqkv, h):
    """o [B,T,H*D], dqkv [B,T,3,H,D] -> [B,H,T,D] views."""
    b, t, e = o.shape
    dq, dk, dv = dqkv.permute(2, 0, 3, 1, 4).unbind(0)
    return o.view(b, t, h, e // h).transpose(1, 2), dq, dk, dv


def _kernel_bhtd(q, k, v, do, scale, p_drop=0.0, seed=0):
    o, lse = EXT.fmha_fwd(q, k, v, scale, p_drop, seed)
    dq, dk, dv = EXT.fmha_bwd(do, q, k, v, o, lse, scale, p_drop, seed)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def _kernel_qkv(q, k, v, do, scale, p_drop=0.0, seed=0):
    h = q.shape[1]
    qkv, do_flat = _to_qkv(q, k, v, do)
    o, lse = EXT.fmha_fwd_qkv(qkv, h, scale, p_drop, seed)
    dqkv = EXT.fmha_bwd_qkv(do_flat, qkv, o, lse, h, scale, p_drop, seed)
    o4, dq, dk, dv = _from_qkv(o, dqkv, h)
    return {"o": o4, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def _floors(q, k, v, do, scale):
    """T = 1 only: P = 1 and dS = scale * (dP - Delta) = 0 exactly, so the
    fp64 dq and dk are zero and the relative metrics have nothing to
    divide by.  dP and Delta are fp32 sums of the same DP products in
    different orders, each within DP * 2^-24 * sum|dO_d v_d| of the exact
    value; what is left is bounded by scale * 2 * DP * 2^-24 * sum|dO v|
    times the largest |k| (dq) or |q| (dk), plus the bf16 store."""
    if q.shape[-2] != 1:
        return None
    dp = ((q.shape[-1] + 31) // 32) * 32
    ds = scale * 2 * dp * _U * (do.double().abs() * v.double().abs()).sum(-1)
    ds = ds.max().item() * (1 + 2.0 ** -8)
    return {"dq": ds * k.double().abs().max().item(),
            "dk": ds * q.double().abs().max().item()}


def _run(family, t, d, layout="bhtd", p_drop=0.0, seed=0):
    name = f"{layout}/{family}/T{t}/D{d}" + (f"/p{p_drop}" if p_drop else "")
    q, k, v, do = make_inputs(family, B, H, t, d, seed, device=_dev())
    scale = d ** -0.5
    keep = keep_mask(DROP_SEED, p_drop, B, H, t, _dev()) if p_drop else None
    run = _kernel_bhtd if layout == "bhtd" else _kernel_qkv
    got = run(q, k, v, do, scale, p_drop, DROP_SEED if p_drop else 0)
    for x in got.values():
        assert bool(torch.isfinite(x.float()).all()), name
    ref64, _, _ = check_kernel_outputs(q, k, v, do, scale, got, name, keep,
                                       p_drop, _floors(q, k, v, do, scale))
    if family != "randn":
        assert_family_stress(family, ref64, d, t)
    return (q, k, v, do, scale), got


@pytest.mark.parametrize("family", ["randn", "rising"])
@pytest.mark.parametrize("t", [33, 129])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_head_dim_sweep(d, t, family):
    """All twelve dispatched head dims: both QSub settings (D <= 96 ->
    128-row q tiles) and all five DP > D zero-padded cases."""
    _run(family, t, d)


@pytest.mark.parametrize(
    "t", [1, 7, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257])
@pytest.mark.parametrize("d", [48, 96, 112, 160, 192])
def test_seq_len_sweep(d, t):
    """T = 1, T < 16 and +-1 around the 32 / 64 / 128 tile edges, at
    QSub=2 with DP>D (48), both sides of the QSub switch (96, 112), the
    workload head (160) and the widest (192)."""
    _run("randn", t, d)


@pytest.mark.parametrize("family", ["randn", "peaked", "rising", "offset"])
@pytest.mark.parametrize("t", [80, 256])
@pytest.mark.parametrize("d", [64, 160])
def test_input_families(d, t, family):
    _run(family, t, d)


@pytest.mark.parametrize("family", ["randn", "rising"])
@pytest.mark.parametrize("t", [33, 129])
@pytest.mark.parametrize("d", [48, 96, 112, 160, 192])
def test_fused_qkv_layout(d, t, family):
    """[B,T,3,H,D] entry points against the same reference through the
    permuted views, and bit-equal to the contiguous entry points: the
    arithmetic is identical, only the strides differ."""
    inp, got = _run(family, t, d, layout="qkv")
    want = _kernel_bhtd(*inp)
    for key in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(got[key], want[key]), key


@pytest.mark.parametrize("layout", ["bhtd", "qkv"])
@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("t", [33, 200])
@pytest.mark.parametrize("d", [48, 112, 160])
def test_dropout(d, t, family, layout):
    """p = 0.3 with the exact mask folded into both the fp64 reference
    and the rounding model."""
    _run(family, t, d, layout=layout, p_drop=0.3)


@pytest.mark.parametrize("p_drop", [0.0, 0.3])
@pytest.mark.parametrize("layout", ["bhtd", "qkv"])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_dispatch_table_coverage(d, layout, p_drop):
    """Every instantiation of the dispatch table -- twelve head dims,
    with and without dropout -- through both layouts, at a T one past the
    64-row tiles (two q tiles at D > 96, three key tiles, two dkv
    blocks)."""
    _run("peaked", 65, d, layout=layout, p_drop=p_drop)


def test_dropout_p09():
    """Most entries dropped; the 1/(1-p) = 10x scale is applied before
    the bf16 pack of P."""
    _run("randn", 200, 112, p_drop=0.9)


def test_attention_autograd_wrapper():
    from vit_10b_fsdp_example_amd.ops import attention

    t, d = 129, 160
    q, k, v, do = make_inputs("randn", B, H, t, d, 5, device=_dev())
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
    o = attention(*leaves)
    o.backward(do)
    got = {"o": o.detach(), "dq": leaves[0].grad, "dk": leaves[1].grad,
           "dv": leaves[2].grad}
    check_kernel_outputs(q, k, v, do, d ** -0.5, got, "ops.attention")


def test_attention_qkv_autograd_wrapper():
    from vit_10b_fsdp_example_amd.ops import attention_qkv

    t, d = 129, 96
    q, k, v, do = make_inputs("randn", B, H, t, d, 6, device=_dev())
    qkv, do_flat = _to_qkv(q, k, v, do)
    qkv.requires_grad_(True)
    o = attention_qkv(qkv, H)
    assert o.shape == (B, t, H * d)
    o.backward(do_flat)
    o4, dq, dk, dv = _from_qkv(o.detach(), qkv.grad, H)
    got = {"o": o4, "dq": dq, "dk": dk, "dv": dv}
    check_kernel_outputs(q, k, v, do, d ** -0.5, got, "ops.attention_qkv")


def test_attention_fp16_takes_math_path():
    """fp16 must not reach the bf16-only kernel: attention() returns the
    math composition's result, and its autograd works."""
    attn = importlib.import_module("vit_10b_fsdp_example_amd.ops.attention")

    q, k, v, do = (x.to(torch.float16) for x in
                   make_inputs("randn", B, H, 33, 64, 7, device=_dev()))
    want = attn.math_attention(q, k, v)
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
    out = attn.attention(*leaves)
    assert out.dtype == torch.float16 and torch.equal(out, want)
    out.backward(do)
    assert all(bool(torch.isfinite(x.grad.float()).all()) for x in leaves)


# ---- refusals: the backward entry points validate what they read.  Every
# bad argument's storage is at least as large as the good one's, so
# nothing can read out of bounds whatever the entry point does with it.


def _good_bwd_args():
    t, d = 33, 64
    q, k, v, do = make_inputs("randn", B, H, t, d, 8, device=_dev())
    scale = d ** -0.5
    o, lse = EXT.fmha_fwd(q, k, v, scale)
    return {"dout": do, "q": q, "k": k, "v": v, "o": o, "lse": lse}, scale


def _non_contiguous(x):
    """Same shape and values, transposed view of a full-size tensor."""
    return x.transpose(-2, -1).contiguous().transpose(-2, -1)


def _bad(kind, args, name):
    x = args[name]
    if kind == "noncontig":
        bad = _non_contiguous(x)
        assert bad.shape == x.shape and not bad.is_contiguous()
    elif kind == "fp32":
        bad = x.float()
    elif kind == "lse_long":
        bad = torch.zeros(x.shape[0], x.shape[1], x.shape[2] + 1,
                          device=x.device, dtype=x.dtype)
    assert bad.untyped_storage().nbytes() >= x.untyped_storage().nbytes()
    return bad


@pytest.mark.parametrize("kind,name", [
    ("noncontig", "o"), ("noncontig", "k"), ("noncontig", "dout"),
    ("fp32", "o"), ("fp32", "q"), ("fp32", "v"), ("fp32", "dout"),
    ("lse_long", "lse"),
])
def test_fmha_bwd_refuses(kind, name):
    args, scale = _good_bwd_args()
    args[name] = _bad(kind, args, name)
    with pytest.raises(RuntimeError, match=r"fmha_bwd: "):
        EXT.fmha_bwd(args["dout"], args["q"], args["k"], args["v"],
                     args["o"], args["lse"], scale)


@pytest.mark.parametrize("kind,name", [
    ("noncontig", "o"), ("noncontig", "dout"), ("fp32", "o"),
    ("fp32", "dout"), ("fp32", "qkv"), ("lse_long", "lse"),
])
def test_fmha_bwd_qkv_refuses(kind, name):
    t, d = 33, 64
    q, k, v, do = make_inputs("randn", B, H, t, d, 9, device=_dev())
    qkv, do_flat = _to_qkv(q, k, v, do)
    scale = d ** -0.5
    o, lse = EXT.fmha_fwd_qkv(qkv, H, scale)
    args = {"dout": do_flat, "qkv": qkv, "o": o, "lse": lse}
    args[name] = _bad(kind, args, name)
    with pytest.raises(RuntimeError, match=r"fmha_bwd_qkv: "):
        EXT.fmha_bwd_qkv(args["dout"], args["qkv"], args["o"], args["lse"],
                         H, scale)


def test_backward_accepts_what_the_forward_returns():
    """The checks refuse nothing that is right: o as [B,T,H,D] too."""
    t, d = 33, 64
    q, k, v, do = make_inputs("randn", B, H, t, d, 9, device=_dev())
    qkv, do_flat = _to_qkv(q, k, v, do)
    scale = d ** -0.5
    o, lse = EXT.fmha_fwd_qkv(qkv, H, scale)
    a = EXT.fmha_bwd_qkv(do_flat, qkv, o, lse, H, scale)
    b = EXT.fmha_bwd_qkv(do_flat.view(B, t, H, d), qkv, o.view(B, t, H, d),
                         lse, H, scale)
    assert torch.equal(a, b)
