"""csrc/qk_rmsnorm.hip and --qk_norm_type rmsnorm on the GPU: the kernels
against fp64 from the same bf16 inputs under the per-element bounds of
tests/test_gpu_rmsnorm.py (one bf16 rounding plus short fp32 chains), the
ops path bit-identical to the kernels chained by hand with and without the
recompute, what the node saves, the refusals, one Block."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None

from vit_10b_fsdp_example_amd.ops.attention import (  # noqa: E402
    QK_RMSNORM_HEAD_DIMS, _draw_seed, attention_qkv,
)
from vit_10b_fsdp_example_amd.ops.rmsnorm import _composition  # noqa: E402

EPS = 1e-6
# csrc/qk_rmsnorm.hip Geometry<L>: kBlocks, and kRowsPerIter by L
QK_BLOCKS, ROWS_PER_ITER = 512, {4: 32, 2: 64}
# one row more than a full first walk, so that workgroup 0 alone walks
# twice: 16385 = 5 * 3277 rows at L = 4, 32769 = 3 * 10923 at L = 2
WALKS = [(5, 3277, 1, 160), (3, 10923, 1, 80)]
assert [b * t for b, t, _, _ in WALKS] == [
    QK_BLOCKS * ROWS_PER_ITER[L] + 1 for L in (4, 2)]
# 3 rows per slice with idle groups at every head dim; H = 5: 15 rows,
# groups straddle tokens and the second wave of each slice is empty
SHAPES = [(1, 3, 1, d) for d in QK_RMSNORM_HEAD_DIMS] + [
    (3, 1, 5, d) for d in (48, 80, 160)] + WALKS


def _bits(t):
    return t.contiguous().view(torch.int16)


def _rn(g, *shape):
    return torch.randn(*shape, generator=g).to("cuda", torch.bfloat16)


@pytest.mark.parametrize("family", ["randn", "zero_and_constant_rows"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_vs_fp64(shape, family):
    B, T, H, D = shape
    rows = B * T * H
    g = torch.Generator().manual_seed(0)
    qkv, dout = _rn(g, B, T, 3, H, D), _rn(g, B, T, 3, H, D)
    if family != "randn":  # rows 0 and 1 of q and of k
        for r, value in ((0, 0.0), (1, 0.30078125)):
            qkv[r // (T * H), r // H % T, :2, r % H] = value
    ws = [1 + 0.5 * _rn(g, D), 1 + 0.5 * _rn(g, D)]

    out, rstd = EXT.qk_rmsnorm_fwd(qkv, *ws, EPS)
    dqkv = dout.clone()
    grads = EXT.qk_rmsnorm_bwd(dqkv, qkv, *ws, rstd)
    again = EXT.qk_rmsnorm_bwd(dout.clone(), qkv, *ws, rstd)
    assert out.shape == qkv.shape and out.dtype == torch.bfloat16
    assert rstd.shape == (B, T, 2, H) and rstd.dtype == torch.float32
    # v: copied by the forward, not touched by the backward
    assert torch.equal(_bits(out[:, :, 2]), _bits(qkv[:, :, 2]))
    assert torch.equal(_bits(dqkv[:, :, 2]), _bits(dout[:, :, 2]))
    for a, b in zip(grads, again):
        assert a.shape == (D,) and a.dtype == torch.bfloat16
        assert torch.equal(_bits(a), _bits(b))

    for s in range(2):
        x = qkv[:, :, s].reshape(rows, D).double()
        dy, w = dout[:, :, s].reshape(rows, D).double(), ws[s].double()
        r64 = torch.rsqrt(x.pow(2).mean(1, keepdim=True) + EPS)
        xhat, gw = x * r64, dy * w
        y64 = xhat * w
        dx64 = r64 * (gw - xhat * (gw * xhat).mean(1, keepdim=True))
        dw64 = (dy * xhat).sum(0)
        m = r64 * (gw.abs() + xhat.abs() * (gw * xhat).abs().mean(1, keepdim=True))
        for name, got, want, tol in (
                ("y", out[:, :, s], y64, 2.0 ** -7 * y64.abs()),
                ("dx", dqkv[:, :, s], dx64,
                 2.0 ** -7 * dx64.abs() + 2.0 ** -17 * m),
                ("dw", grads[s], dw64,
                 2.0 ** -7 * dw64.abs() + (rows + 4 * D) * 2.0 ** -24 * (
                     dy.abs() * (xhat.abs() + 1)).sum(0))):
            err = (got.reshape(want.shape).double() - want).abs()
            print(f"{'qk'[s]} {name}: max err / bound "
                  f"{(err / tol.clamp_min(1e-300)).max():.3f}")
            assert bool((err <= tol).all()), (s, name, (err - tol).max().item())
        if family != "randn":  # row 0 is all zeros
            assert not bool(out[:, :, s].reshape(rows, D)[0].any())


def _operands(B, T, H, D):
    g = torch.Generator().manual_seed(7)
    return (_rn(g, B, T, 3, H, D), 1 + 0.5 * _rn(g, D), 1 + 0.5 * _rn(g, D),
            _rn(g, B, T, H * D))


def _through_ops(qkv, wq, wk, do, p_drop):
    leaves = [t.clone().requires_grad_(True) for t in (qkv, wq, wk)]
    torch.manual_seed(11)
    o = attention_qkv(leaves[0], qkv.shape[3], dropout_p=p_drop,
                      training=True, qk_norm=(leaves[1], None, leaves[2],
                                              None, EPS))
    return (o.detach(),) + torch.autograd.grad(o, leaves, do)


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_ops_path_is_the_chain_bit_for_bit(p_drop, monkeypatch):
    B, T, H, D = 2, 256, 4, 80
    qkv, wq, wk, do = _operands(B, T, H, D)
    do_before = do.clone()
    torch.manual_seed(11)
    seed = _draw_seed() if p_drop > 0.0 else 0
    qkv_n, rstd = EXT.qk_rmsnorm_fwd(qkv, wq, wk, EPS)
    o, lse = EXT.fmha_fwd_qkv(qkv_n, H, D ** -0.5, p_drop, seed)
    dqkv = EXT.fmha_bwd_qkv(do, qkv_n, o, lse, H, D ** -0.5, p_drop, seed)
    want = (o, dqkv) + tuple(EXT.qk_rmsnorm_bwd(dqkv, qkv, wq, wk, rstd))
    for recompute in ("1", "0"):
        monkeypatch.setenv("VITFSDP_QK_NORM_RECOMPUTE", recompute)
        for a, b in zip(_through_ops(qkv, wq, wk, do, p_drop), want):
            assert a.shape == b.shape and torch.equal(_bits(a), _bits(b))
    # the in-place step worked on the function's own buffer
    assert torch.equal(_bits(do), _bits(do_before))


def test_recompute_saves_one_qkv_less(monkeypatch):
    qkv, wq, wk, do = _operands(2, 256, 4, 160)
    saved = {}
    for recompute in ("1", "0"):
        monkeypatch.setenv("VITFSDP_QK_NORM_RECOMPUTE", recompute)
        sizes = []
        with torch.autograd.graph.saved_tensors_hooks(
                lambda t: sizes.append(t.numel() * t.element_size()) or t,
                lambda t: t):
            _through_ops(qkv, wq, wk, do, 0.0)
        saved[recompute] = sum(sizes)
    assert saved["0"] - saved["1"] == qkv.numel() * 2


@pytest.mark.parametrize("case", ["D=24", "D=208", "strided", "fp32 weight"])
def test_kernel_refuses_and_op_takes_the_composition(case):
    D = {"D=24": 24, "D=208": 208}.get(case, 64)
    g = torch.Generator().manual_seed(5)
    qkv, w = _rn(g, 2, 128, 3, 2, D), 1 + 0.5 * _rn(g, D)
    rstd = torch.ones(2, 128, 2, 2, device="cuda")
    if case == "strided":
        qkv = torch.stack([qkv, qkv], -1)[..., 0]
    if case == "fp32 weight":
        w = w.float()
    with pytest.raises(RuntimeError, match="qk_rmsnorm_fwd: "):
        EXT.qk_rmsnorm_fwd(qkv, w, w, EPS)
    with pytest.raises(RuntimeError, match="qk_rmsnorm_bwd: "):
        EXT.qk_rmsnorm_bwd(qkv.clone(), qkv, w, w, rstd)
    if case == "fp32 weight":
        q, k, v = qkv.unbind(2)
        ref = attention_qkv(torch.stack(
            (_composition(q, w, EPS), _composition(k, w, EPS), v), dim=2), 2)
        got = attention_qkv(qkv, 2, qk_norm=(w, None, w, None, EPS))
        assert torch.equal(_bits(got), _bits(ref))
    torch.cuda.synchronize()


def test_block_checkpointing_is_bit_identical():
    from vit_10b_fsdp_example_amd.models.vit import Block
    from vit_10b_fsdp_example_amd.ops import RMSNorm
    from vit_10b_fsdp_example_amd.parallel import checkpoint_module

    torch.manual_seed(0)
    blk = Block(640, 8, qk_norm=True, qk_norm_type="rmsnorm").to(
        "cuda", torch.bfloat16).train()
    assert isinstance(blk.attn.q_norm, RMSNorm) and blk.attn.head_dim == 80
    x = torch.randn(2, 256, 640, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    dy = torch.randn_like(x)
    leaves = [x] + list(blk.parameters())
    plain = torch.autograd.grad(blk(x), leaves, dy)
    ckpt = torch.autograd.grad(checkpoint_module(blk)(x), leaves, dy)
    for a, b in zip(plain, ckpt):
        assert torch.equal(_bits(a), _bits(b))
