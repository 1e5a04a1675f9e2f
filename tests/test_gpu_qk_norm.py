"""csrc/qk_norm.hip and --qk_norm on the GPU: the kernels against fp64
under kernel_reference's LayerNorm bounds, the ops path bit-identical to
the kernels chained by hand, the operand refusals, one training step."""

import math

import pytest
import torch
import torch.nn.functional as F

from tests import kernel_reference as kr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None

from vit_10b_fsdp_example_amd.ops.attention import (  # noqa: E402
    QK_NORM_HEAD_DIMS, _draw_seed, attention_qkv,
)

EPS = kr.LN_EPS
ROWS_PER_ITER, QK_BLOCKS = 32, 512  # csrc/qk_norm.hip kRowsPerIter, kQkBlocks
# one row more than a full first walk (16385 = 5 * 3277 tokens of one
# head, 47 MB per tensor at D = 160): workgroup 0 alone walks twice
WALK = (5, (QK_BLOCKS * ROWS_PER_ITER + 1) // 5, 1)
assert WALK[0] * WALK[1] == QK_BLOCKS * ROWS_PER_ITER + 1
# H = 5: 15 rows per slice, a wave's 16 groups straddle tokens and the
# second wave of each slice is empty
SHAPES = [(1, 3, 1, d) for d in QK_NORM_HEAD_DIMS] + [
    (3, 1, 5, d) for d in QK_NORM_HEAD_DIMS] + [
    WALK + (d,) for d in (64, 160)]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _case(shape, family):
    """Inputs and the kernels' outputs of one case."""
    B, T, H, D = shape
    rows = B * T * H
    inq = kr.ln_make_inputs(family, rows, D, 1, "cuda")
    ink = kr.ln_make_inputs(family, rows, D, 2, "cuda")
    g = torch.Generator().manual_seed(3)
    qkv = torch.empty(B, T, 3, H, D, device="cuda", dtype=torch.bfloat16)
    dout = torch.empty_like(qkv)
    for s, inp in enumerate((inq, ink)):
        qkv[:, :, s] = inp[0].view(B, T, H, D)
        dout[:, :, s] = inp[4].view(B, T, H, D)
    qkv[:, :, 2] = torch.randn(B, T, H, D, generator=g).to(qkv)
    dout[:, :, 2] = torch.randn(B, T, H, D, generator=g).to(qkv)
    wq, bq, wk, bk = inq[2], inq[3], ink[2], ink[3]
    out, mean, rstd = EXT.qk_norm_fwd(qkv, wq, bq, wk, bk, EPS)
    dqkv = dout.clone()
    grads = EXT.qk_norm_bwd(dqkv, qkv, wq, wk, mean, rstd)
    again = EXT.qk_norm_bwd(dout.clone(), qkv, wq, wk, mean, rstd)
    return (inq, ink), qkv, dout, out, mean, rstd, dqkv, grads, again


@pytest.mark.parametrize("family", kr.LN_FAMILIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_vs_fp64(shape, family):
    B, T, H, D = shape
    rows = B * T * H
    inputs, qkv, dout, out, mean, rstd, dqkv, grads, again = _case(
        shape, family)
    assert out.shape == qkv.shape and out.dtype == torch.bfloat16
    assert mean.shape == rstd.shape == (B, T, 2, H)
    # v: copied by the forward, not touched by the backward
    assert torch.equal(_bits(out[:, :, 2]), _bits(qkv[:, :, 2]))
    assert torch.equal(_bits(dqkv[:, :, 2]), _bits(dout[:, :, 2]))
    for a, b in zip(grads, again):
        assert a.shape == (D,) and a.dtype == torch.bfloat16
        assert torch.equal(_bits(a), _bits(b))

    for s, inp in enumerate(inputs):
        name = f"qk_norm/{'qk'[s]}/{family}/{B}x{T}x{H}x{D}"
        got = {"y": out[:, :, s].reshape(rows, D),
               "mean": mean[:, :, s].reshape(rows),
               "rstd": rstd[:, :, s].reshape(rows),
               "dx": dqkv[:, :, s].reshape(rows, D)}
        _, ref, _ = kr.ln_check(got, inp, "plain", name)
        kr.ln_assert_family(family, ref["sum"], rows)

        # dgamma, dbeta: bf16 store + worst-case fp32 sum in any order +
        # (dgamma only) what the statistics' intervals leave of xhat
        dy = inp[4].double()
        st = kr.ln_stat_bounds(ref["sum"], EPS)
        xhat = ref["xhat"]
        dxhat = (st["dmean"] * st["rstd_hi"]).unsqueeze(1) + xhat.abs() * (
            st["drstd"] / st["rstd"]).unsqueeze(1)
        for what, terms, extra, got_g in (
                ("dgamma", dy * xhat, (dy.abs() * dxhat).sum(0), grads[2 * s]),
                ("dbeta", dy, 0.0, grads[2 * s + 1])):
            col = terms.sum(0)
            bound = (2.0 ** -8 * col.abs()
                     + (rows + 16) * 2.0 ** -24 * terms.abs().sum(0) + extra)
            err = (got_g.double() - col).abs()
            print(f"{name} {what}: worst err/bound "
                  f"{(err / bound).max().item():.3f}")
            assert bool((err <= bound).all()), (name, what)


def _chain(qkv, H, params, do, p_drop, seed):
    wq, bq, wk, bk = params
    scale = qkv.shape[-1] ** -0.5
    qkv_n, mean, rstd = EXT.qk_norm_fwd(qkv, wq, bq, wk, bk, EPS)
    o, lse = EXT.fmha_fwd_qkv(qkv_n, H, scale, p_drop, seed)
    dqkv = EXT.fmha_bwd_qkv(do, qkv_n, o, lse, H, scale, p_drop, seed)
    return (o, dqkv) + tuple(EXT.qk_norm_bwd(dqkv, qkv, wq, wk, mean, rstd))


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_ops_path_is_the_chain_bit_for_bit(p_drop):
    B, T, H, D = 2, 256, 4, 160
    g = torch.Generator().manual_seed(7)

    def rn(*shape):
        return torch.randn(*shape, generator=g).to("cuda", torch.bfloat16)

    qkv, do = rn(B, T, 3, H, D), rn(B, T, H * D)
    params = [1.0 + 0.5 * rn(D), rn(D), 1.0 + 0.5 * rn(D), rn(D)]
    do_before = do.clone()

    leaves = [t.clone().requires_grad_(True) for t in [qkv] + params]
    torch.manual_seed(11)
    o = attention_qkv(leaves[0], H, dropout_p=p_drop, training=True,
                      qk_norm=(*leaves[1:], EPS))
    got = (o.detach(),) + torch.autograd.grad(o, leaves, do)
    torch.manual_seed(11)
    seed = _draw_seed() if p_drop > 0.0 else 0
    want = _chain(qkv, H, params, do, p_drop, seed)
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b))
    # the in-place step worked on the function's own buffer
    assert torch.equal(_bits(do), _bits(do_before))


def test_block_checkpointing_is_bit_identical():
    from vit_10b_fsdp_example_amd.models.vit import Block
    from vit_10b_fsdp_example_amd.parallel import checkpoint_module

    torch.manual_seed(0)
    blk = Block(640, 4, qk_norm=True).to("cuda", torch.bfloat16).train()
    x = torch.randn(2, 256, 640, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    dy = torch.randn_like(x)
    leaves = [x] + list(blk.parameters())
    plain = torch.autograd.grad(blk(x), leaves, dy)
    ckpt = torch.autograd.grad(checkpoint_module(blk)(x), leaves, dy)
    for a, b in zip(plain, ckpt):
        assert torch.equal(_bits(a), _bits(b))


def _bad_variants(t):
    """wrong dtype, not contiguous, wrong shape (one dim more: nothing
    else about it is wrong), wrong device"""
    yield t.to(torch.float16 if t.dtype == torch.float32 else torch.float32)
    yield torch.stack([t, t], -1)[..., 0]
    yield t.unsqueeze(0)
    yield t.cpu()


@pytest.mark.parametrize("fn", ["qk_norm_fwd", "qk_norm_bwd"])
def test_refuses_bad_operands(fn):
    inputs, qkv, dout, _, mean, rstd, _, _, _ = _case((2, 3, 2, 64), "randn")
    wq, bq, wk, bk = inputs[0][2], inputs[0][3], inputs[1][2], inputs[1][3]
    names, args = {
        "qk_norm_fwd": ("qkv wq bq wk bk", [qkv, wq, bq, wk, bk, EPS]),
        "qk_norm_bwd": ("dqkv qkv wq wk mean rstd",
                        [dout.clone(), qkv, wq, wk, mean, rstd])}[fn]
    getattr(EXT, fn)(*args)
    for i, what in enumerate(names.split()):
        for bad in _bad_variants(args[i]):
            call = list(args)
            call[i] = bad
            with pytest.raises(RuntimeError, match=f"{fn}: .*{what}"):
                getattr(EXT, fn)(*call)
    # unsupported head dims: the message names the supported set
    for d in (8, 80, 224):
        qkv = torch.zeros(1, 2, 3, 2, d, device="cuda", dtype=torch.bfloat16)
        v = torch.zeros(d, device="cuda", dtype=torch.bfloat16)
        st = torch.zeros(1, 2, 2, 2, device="cuda")
        bad_d = {"qk_norm_fwd": (qkv, v, v, v, v, EPS),
                 "qk_norm_bwd": (qkv, qkv, v, v, st, st)}[fn]
        with pytest.raises(RuntimeError, match="32, 64, 96, 128, 160, 192"):
            getattr(EXT, fn)(*bad_d)
    torch.cuda.synchronize()


def test_empty_batch():
    D = 64
    qkv = torch.empty(0, 5, 3, 2, D, device="cuda", dtype=torch.bfloat16)
    w = torch.ones(D, device="cuda", dtype=torch.bfloat16)
    out, mean, rstd = EXT.qk_norm_fwd(qkv, w, w, w, w, EPS)
    assert out.shape == qkv.shape and mean.shape == rstd.shape == (0, 5, 2, 2)
    grads = EXT.qk_norm_bwd(qkv.clone(), qkv, w, w, mean, rstd)
    assert len(grads) == 4
    assert all(g.shape == (D,) and not bool(g.any()) for g in grads)


def test_unsupported_head_dim_takes_the_composition():
    B, T, H, D = 2, 128, 2, 80
    assert D not in QK_NORM_HEAD_DIMS
    g = torch.Generator().manual_seed(5)

    def rn(*shape):
        return torch.randn(*shape, generator=g).to("cuda", torch.bfloat16)

    qkv = rn(B, T, 3, H, D).requires_grad_(True)
    wq, bq, wk, bk = 1.0 + 0.5 * rn(D), rn(D), 1.0 + 0.5 * rn(D), rn(D)
    do = rn(B, T, H * D)
    o = attention_qkv(qkv, H, qk_norm=(wq, bq, wk, bk, EPS))
    q, k, v = qkv.unbind(2)
    ref = attention_qkv(torch.stack(
        (F.layer_norm(q, (D,), wq, bq, EPS),
         F.layer_norm(k, (D,), wk, bk, EPS), v), dim=2), H)
    assert torch.equal(_bits(o), _bits(ref))
    (dqkv,) = torch.autograd.grad(o, qkv, do)
    (dref,) = torch.autograd.grad(ref, qkv, do)
    assert torch.equal(_bits(dqkv), _bits(dref))


def test_one_training_step():
    from vit_10b_fsdp_example_amd import dist as xdist
    from vit_10b_fsdp_example_amd.cli import parse_args
    from vit_10b_fsdp_example_amd.models import build_fsdp_vit_model
    from vit_10b_fsdp_example_amd.ops import (
        CrossEntropyLoss, FusedAdamW, LayerNorm,
    )
    from vit_10b_fsdp_example_amd.parallel import CommContext

    CommContext.reset()
    cfg = parse_args(
        "--fake_data --image_size 224 --patch_size 14 --embed_dim 640 "
        "--num_heads 4 --num_blocks 2 --num_classes 100 --batch_size 8 "
        "--num_workers 0 --qk_norm".split())
    device = xdist.init_distributed()
    torch.manual_seed(0)
    model = build_fsdp_vit_model(cfg, device, compute_dtype=torch.bfloat16)
    opt = FusedAdamW(model.parameters(), lr=1e-2, weight_decay=0.1)
    x = torch.randn(8, 3, 224, 224, device=device, dtype=torch.bfloat16)
    y = torch.randint(0, 100, (8,), device=device)

    def norm_params():
        # ws = 1: a unit's fp32 master shard is its whole flat buffer
        return [unit.flat_param.data[off:off + numel].clone()
                for unit in model._all_units()
                for mod, _, _, numel, off in unit._param_infos
                if isinstance(mod, LayerNorm) and mod.dim == 160]

    before = norm_params()
    assert len(before) == 2 * 4
    loss = CrossEntropyLoss()(model(x), y)
    loss.backward()
    gn = model.clip_grad_norm_(1.0)
    opt.step()
    opt.zero_grad(set_to_none=True)
    assert math.isfinite(float(loss.detach())) and math.isfinite(float(gn))
    for i, (a, b) in enumerate(zip(before, norm_params())):
        assert not torch.equal(a, b), i
