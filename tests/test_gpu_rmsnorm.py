"""csrc/rmsnorm.hip through ops.rms_norm / ops.fused_add_rms_norm and
autograd, against fp64 from the same bf16 inputs, at the shapes where a
register-resident row and a block that walks many rows can go wrong.

Bounds, applied to every element: one bf16 rounding of the result (2^-8
relative, stated as 2^-7) plus fp32 arithmetic whose reduction chains stay
under 64 additions (2^-17 of the magnitude sum of the terms); for dw the
accumulation term of tests/test_gpu_ln_bwd_fused.py."""

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-6
SHAPES = [
    (1, 8),        # one vector, 255 idle threads
    (3, 64),       # a small row
    (5, 2056),     # VPT 2 with a single thread in the second slot
    (3, 5120),     # VPT 3, partly filled
    (3, 8192),     # VPT 4, full
    (769, 64),     # one more row than the backward's grid: block 0 walks two
    (1037, 1024),  # rows no multiple of the grid
]


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("family", ["randn", "zero_and_constant_rows"])
@pytest.mark.parametrize("add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_against_fp64(shape, add, family):
    from vit_10b_fsdp_example_amd import _C
    from vit_10b_fsdp_example_amd.ops import fused_add_rms_norm, rms_norm

    rows, d = shape
    torch.manual_seed(0)
    bf = dict(device=_dev(), dtype=torch.bfloat16)
    x = torch.randn(rows, d, **bf)
    if family != "randn" and rows >= 3:
        x[0] = 0.0
        x[1] = 0.30078125
    res = 0.5 * torch.randn(rows, d, **bf)
    w = (1 + 0.5 * torch.randn(d, device=_dev())).bfloat16()
    dy, dsum = torch.randn(rows, d, **bf), torch.randn(rows, d, **bf)
    for t in (x, res, w):
        t.requires_grad_(True)

    if add:
        s, y = fused_add_rms_norm(x, res, w, EPS)
        assert torch.equal(s, x.detach() + res.detach())  # bit for bit
        torch.autograd.backward([s, y], [dsum, dy])
        # equal values in distinct storage
        assert torch.equal(x.grad, res.grad)
        assert x.grad.data_ptr() != res.grad.data_ptr()
        s64, ds64 = s.detach().double(), dsum.double()
    else:
        y = rms_norm(x, w, EPS)
        y.backward(dy)
        s64, ds64 = x.detach().double(), torch.zeros_like(dy).double()

    rstd = torch.rsqrt(s64.pow(2).mean(1, keepdim=True) + EPS)
    xhat, g = s64 * rstd, dy.double() * w.detach().double()
    y64 = xhat * w.detach().double()
    dx64 = rstd * (g - xhat * (g * xhat).mean(1, keepdim=True)) + ds64
    dw64 = (dy.double() * xhat).sum(0)
    m = rstd * (g.abs() + xhat.abs() * (g * xhat).abs().mean(1, keepdim=True))
    y_tol = 2.0 ** -7 * y64.abs()
    dx_tol = 2.0 ** -7 * dx64.abs() + 2.0 ** -17 * (m + ds64.abs())
    dw_tol = 2.0 ** -7 * dw64.abs() + (rows + 4 * d) * 2.0 ** -24 * (
        dy.double().abs() * (xhat.abs() + 1)).sum(0)
    for name, got, want, tol in (("y", y, y64, y_tol),
                                 ("dx", x.grad, dx64, dx_tol),
                                 ("dw", w.grad, dw64, dw_tol)):
        err = (got.detach().double() - want).abs()
        print(f"{name}: max err / bound {(err / tol.clamp_min(1e-300)).max():.3f}")
        assert bool((err <= tol).all()), (name, (err - tol).max().item())

    if family != "randn" and rows >= 3 and not add:  # row 0 is all zeros
        assert not bool(y[0].detach().any())
        stat = _C.rmsnorm_fwd(x.detach(), w.detach(), EPS)[1]
        assert abs(float(stat[0]) * EPS ** 0.5 - 1) <= 2.0 ** -20


@pytest.mark.parametrize("case", ["D=8200", "D=12", "fp32 weight"])
def test_kernel_refuses_and_op_takes_the_composition(case):
    from vit_10b_fsdp_example_amd import _C
    from vit_10b_fsdp_example_amd.ops import rms_norm
    from vit_10b_fsdp_example_amd.ops.rmsnorm import _composition

    d = {"D=8200": 8200, "D=12": 12}.get(case, 64)
    torch.manual_seed(0)
    x = torch.randn(3, d, device=_dev(), dtype=torch.bfloat16)
    w = 1 + 0.5 * torch.randn(d, device=_dev())
    if case != "fp32 weight":
        w = w.bfloat16()
    with pytest.raises(RuntimeError, match="rmsnorm_fwd"):
        _C.rmsnorm_fwd(x, w, EPS)
    assert torch.equal(rms_norm(x, w, EPS), _composition(x, w, EPS))


@pytest.mark.parametrize("fuse_residual", [False, True])
def test_model_trains(fuse_residual):
    from vit_10b_fsdp_example_amd import dist as xdist
    from vit_10b_fsdp_example_amd.cli import parse_args
    from vit_10b_fsdp_example_amd.models import build_fsdp_vit_model
    from vit_10b_fsdp_example_amd.ops import (
        CrossEntropyLoss, FusedAdamW, LayerNorm, RMSNorm,
    )
    from vit_10b_fsdp_example_amd.parallel import CommContext

    CommContext.reset()
    cfg = parse_args([
        "--fake_data", "--image_size", "56", "--patch_size", "14",
        "--embed_dim", "640", "--num_heads", "4", "--num_blocks", "2",
        "--num_classes", "100", "--batch_size", "4", "--num_workers", "0",
        "--norm_type", "rmsnorm", "--mlp_type", "swiglu",
    ] + (["--fuse_residual"] if fuse_residual else []))
    device = xdist.init_distributed()
    torch.manual_seed(0)
    model = build_fsdp_vit_model(cfg, device, compute_dtype=torch.bfloat16)
    norms = [m for m in model.modules() if isinstance(m, (LayerNorm, RMSNorm))]
    assert len(norms) == 5
    assert all(isinstance(m, RMSNorm) and not hasattr(m, "bias") for m in norms)
    loss_fn = CrossEntropyLoss()
    opt = FusedAdamW(model.parameters(), lr=3e-3, weight_decay=0.1)
    x = torch.randn(4, 3, 56, 56, device=device, dtype=torch.bfloat16)
    y = torch.randint(0, 100, (4,), device=device)
    losses = []
    for _ in range(5):
        loss = loss_fn(model(x), y)
        loss.backward()
        gn = model.clip_grad_norm_(1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(float(loss.detach()))
        assert losses[-1] == losses[-1] and abs(losses[-1]) != float("inf")
        assert float(gn) == float(gn) and float(gn) != float("inf")
    assert losses[-1] < losses[0], losses
