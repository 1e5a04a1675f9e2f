"""csrc/dropout.hip and ops/dropout.py on the GPU: the in-kernel hash
mask is the python reference's bit for bit, the fused values sit inside
rounding-model bounds of an fp64 reference, the backward regenerates the
forward's mask, no mask tensor is stored, and training under gradient
checkpointing reproduces the masks in the recompute."""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None

from vit_10b_fsdp_example_amd.ops import (  # noqa: E402
    dropout_add, dropout_add_reference, gelu_dropout, gelu_dropout_reference,
    hidden_dropout, hidden_dropout_mask,
)
from vit_10b_fsdp_example_amd.ops.attention import (  # noqa: E402
    dropout_mask_reference,
)

# (257, 2048): exactly one 256-thread block of vectors per row;
# (3, 2056): 257 vectors, a ragged second block
SHAPES = [(1, 8), (5, 64), (257, 2048), (3, 2056), (64, 20480)]
PS = [0.1, 0.25, 0.5]
SEEDS = [0, 1234, 2 ** 31 - 2]

# as tests/test_gpu_gelu_bwd_colsum.py: zero crossing of the derivative
# (~ -0.75), erf saturation, exp underflow
SPECIAL = [0.0, 0.75, -0.75, 10.0, -10.0, 40.0, -40.0]

def cases(fn):
    for names, values in (("rows,cols", SHAPES), ("p", PS), ("seed", SEEDS)):
        fn = pytest.mark.parametrize(names, values)(fn)
    return fn


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _inputs(rows, cols, seed=0):
    """(dy, x, res) bf16 on the GPU; every 5th element of x takes one of
    the special values in turn.  Shared between tests: never modified."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * 2.0
    dy = torch.randn(rows, cols, generator=g)
    res = torch.randn(rows, cols, generator=g)
    flat = x.view(-1)
    idx = torch.arange(0, flat.numel(), 5)
    flat[idx] = torch.tensor(SPECIAL)[torch.arange(idx.numel()) % len(SPECIAL)]
    return tuple(t.to(_dev(), torch.bfloat16) for t in (dy, x, res))


@functools.lru_cache(maxsize=None)
def _mask(seed, rows, cols, p):
    return hidden_dropout_mask(seed, rows, cols, p).to(_dev())


def _rscale32(p):
    # the kernel's scale: 1 / (1 - p) in double, rounded to fp32
    return torch.tensor(1.0 / (1.0 - p), dtype=torch.float32, device=_dev())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _dropout_expected(x, mask, p):
    scaled = (x.float() * _rscale32(p)).bfloat16()
    return torch.where(mask, scaled, torch.zeros_like(scaled))


@cases
def test_dropout_fwd_bit_exact(rows, cols, p, seed):
    dy, x, _ = _inputs(rows, cols)
    mask = _mask(seed, rows, cols, p)
    y = EXT.dropout_fwd(x, p, seed)
    assert y.shape == x.shape and y.dtype == torch.bfloat16
    assert torch.equal(_bits(y), _bits(_dropout_expected(x, mask, p)))
    # dropout is its own adjoint: the same call on dy is the backward
    dx = EXT.dropout_fwd(dy, p, seed)
    assert torch.equal(_bits(dx), _bits(_dropout_expected(dy, mask, p)))


@cases
def test_dropout_add_fwd(rows, cols, p, seed):
    _, x, res = _inputs(rows, cols)
    mask = _mask(seed, rows, cols, p)
    out = EXT.dropout_add_fwd(x, res, p, seed)
    assert out.shape == x.shape and out.dtype == torch.bfloat16
    # wherever the mask drops, the residual stream passes through bitwise
    assert torch.equal(_bits(out)[~mask], _bits(x)[~mask])
    ref = dropout_add_reference(x, res, p, seed)
    err = (out.double() - ref).abs()
    # one bf16 rounding plus fp32 arithmetic slack (an FMA contraction
    # may move the last fp32 bit)
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -23 * (
        x.double().abs() + res.double().abs() / (1.0 - p))
    print(f"max err {err.max().item():.3e}, min slack "
          f"{(bound - err)[mask].min().item():.3e}")
    assert bool((err <= bound)[mask].all()), (err - bound)[mask].max().item()


@cases
def test_gelu_dropout_fwd(rows, cols, p, seed):
    _, x, _ = _inputs(rows, cols)
    mask = _mask(seed, rows, cols, p)
    y = EXT.gelu_dropout_fwd(x, p, seed)
    assert y.shape == x.shape and y.dtype == torch.bfloat16
    # dropped positions are exactly +0
    assert bool((_bits(y)[~mask] == 0).all())
    ref = gelu_dropout_reference(x, p, seed)
    err = (y.double() - ref).abs()
    # one bf16 rounding; the absolute term is the fp32 cancellation in
    # 1 + erf(x / sqrt(2)) for negative x
    slack = 2.0 ** -23 * x.double().abs() / (1.0 - p)
    bound = 2.0 ** -8 * ref.abs() + slack
    print(f"max err {err[mask].max().item():.3e}, min slack "
          f"{(bound - err)[mask].min().item():.3e}")
    assert bool((err <= bound)[mask].all()), (err - bound)[mask].max().item()
    # the zero pattern is the mask's.  A kept element may itself be 0
    # (gelu(0), and gelu(-10), gelu(-40) below fp32's 1 + erf), so the
    # pattern is compared where the reference is nonzero beyond the
    # bound's absolute term
    nonzero_ref = (1.0 - 2.0 ** -8) * ref.abs() > slack
    assert bool((y != 0)[mask & nonzero_ref].all())
    assert torch.equal((y != 0) & nonzero_ref, mask & nonzero_ref)


@cases
def test_gelu_dropout_bwd(rows, cols, p, seed):
    dy, x, _ = _inputs(rows, cols)
    mask = _mask(seed, rows, cols, p)
    dx = EXT.gelu_dropout_bwd(dy, x, p, seed)
    assert dx.shape == x.shape and dx.dtype == torch.bfloat16
    assert bool((_bits(dx)[~mask] == 0).all())
    # torch's kernel in fp32 on the scaled gradient: the existing GELU
    # backward bound (tests/test_gpu_gelu_bwd_colsum.py), scaled
    ref = torch.ops.aten.gelu_backward(
        dy.float() * _rscale32(p), x.float(), approximate="none").double()
    err = (dx.double() - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + (
        2.0 ** -14 * dy.double().abs().max() / (1.0 - p))
    print(f"max err {err[mask].max().item():.3e}, min slack "
          f"{(bound - err)[mask].min().item():.3e}")
    assert bool((err <= bound)[mask].all()), (err - bound)[mask].max().item()


def test_leading_dims_flatten():
    dy, x, res = _inputs(6, 64, seed=1)
    v = (2, 3, 64)
    for out3, out2 in [
        (EXT.dropout_fwd(x.view(v), 0.25, 7), EXT.dropout_fwd(x, 0.25, 7)),
        (EXT.dropout_add_fwd(x.view(v), res.view(v), 0.25, 7),
         EXT.dropout_add_fwd(x, res, 0.25, 7)),
        (EXT.gelu_dropout_fwd(x.view(v), 0.25, 7),
         EXT.gelu_dropout_fwd(x, 0.25, 7)),
        (EXT.gelu_dropout_bwd(dy.view(v), x.view(v), 0.25, 7),
         EXT.gelu_dropout_bwd(dy, x, 0.25, 7)),
    ]:
        assert out3.shape == v
        assert torch.equal(_bits(out3).view(6, 64), _bits(out2))


def test_non_finite_dropped_is_zero_kept_propagates():
    _, x, res = _inputs(5, 64, seed=2)
    p, seed = 0.5, 1234
    mask = _mask(seed, 5, 64, p)
    bad = torch.full_like(x, float("nan"))
    bad[:, ::2] = float("inf")
    for y in (EXT.dropout_fwd(bad, p, seed),
              EXT.gelu_dropout_bwd(bad, x, p, seed)):
        assert bool((_bits(y)[~mask] == 0).all())
        assert not torch.isfinite(y.float()[mask]).any()
    y = EXT.gelu_dropout_fwd(bad, p, seed)
    assert bool((_bits(y)[~mask] == 0).all())
    assert not torch.isfinite(y.float()[mask]).any()
    out = EXT.dropout_add_fwd(x, bad, p, seed)
    assert torch.equal(_bits(out)[~mask], _bits(x)[~mask])
    assert not torch.isfinite(out.float()[mask]).any()


def test_autograd_matches_direct_backward():
    dy, x, res = _inputs(257, 2048)
    p, seed = 0.25, 1234

    xr = x.clone().requires_grad_(True)
    y = hidden_dropout(xr, p, True, seed=seed)
    assert torch.equal(_bits(y), _bits(EXT.dropout_fwd(x, p, seed)))
    (g,) = torch.autograd.grad(y, xr, dy)
    assert torch.equal(_bits(g), _bits(EXT.dropout_fwd(dy, p, seed)))

    xr = x.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True)
    out = dropout_add(xr, rr, p, True, seed=seed)
    assert torch.equal(_bits(out), _bits(EXT.dropout_add_fwd(x, res, p, seed)))
    gx, gr = torch.autograd.grad(out, (xr, rr), dy)
    assert torch.equal(_bits(gx), _bits(dy))
    assert torch.equal(_bits(gr), _bits(EXT.dropout_fwd(dy, p, seed)))

    xr = x.clone().requires_grad_(True)
    y = gelu_dropout(xr, p, True, seed=seed)
    assert torch.equal(_bits(y), _bits(EXT.gelu_dropout_fwd(x, p, seed)))
    (g,) = torch.autograd.grad(y, xr, dy)
    assert torch.equal(_bits(g), _bits(EXT.gelu_dropout_bwd(dy, x, p, seed)))


def test_seed_determinism():
    _, x, res = _inputs(257, 2048)
    for fn in (lambda s: hidden_dropout(x, 0.25, True, seed=s),
               lambda s: dropout_add(x, res, 0.25, True, seed=s),
               lambda s: gelu_dropout(x, 0.25, True, seed=s)):
        assert torch.equal(_bits(fn(11)), _bits(fn(11)))
        assert not torch.equal(_bits(fn(11)), _bits(fn(12)))
    # the default seed comes from the CPU generator
    torch.manual_seed(5)
    a = hidden_dropout(x, 0.25, True)
    b = hidden_dropout(x, 0.25, True)
    torch.manual_seed(5)
    assert torch.equal(_bits(a), _bits(hidden_dropout(x, 0.25, True)))
    assert not torch.equal(_bits(a), _bits(b))


def test_offsets_past_2_31_elements():
    """(65537, 32768) is 2^31 + 32768 elements: the smallest row count at
    this width where a 32-bit element offset wraps.  First row and last
    two rows against the reference."""
    rows, cols, p, seed = 65537, 32768, 0.25, 1234
    x = torch.randn(rows, cols, device=_dev(), dtype=torch.bfloat16)
    y = EXT.dropout_fwd(x, p, seed)
    pick = torch.tensor([0, rows - 2, rows - 1])
    mask = dropout_mask_reference(seed, pick, torch.arange(cols), p).to(_dev())
    pick = pick.to(_dev())
    assert torch.equal(
        _bits(y[pick]), _bits(_dropout_expected(x[pick], mask, p)))
    del x, y
    torch.cuda.empty_cache()


def test_refusals_and_stock_fallback():
    dev = _dev()
    odd = torch.randn(4, 100, device=dev, dtype=torch.bfloat16)
    f32 = torch.randn(4, 64, device=dev)
    ok = torch.randn(4, 64, device=dev, dtype=torch.bfloat16)
    calls = [
        lambda t, p: EXT.dropout_fwd(t, p, 1),
        lambda t, p: EXT.dropout_add_fwd(t, t, p, 1),
        lambda t, p: EXT.gelu_dropout_fwd(t, p, 1),
        lambda t, p: EXT.gelu_dropout_bwd(t, t, p, 1),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="multiple of 8"):
            call(odd, 0.1)
        with pytest.raises(RuntimeError, match="bf16 only"):
            call(f32, 0.1)
        for p in (0.0, 1.0, -0.1, 1.5):
            with pytest.raises(RuntimeError, match=r"p must be in \(0, 1\)"):
                call(ok, p)
    with pytest.raises(RuntimeError, match="one shape"):
        EXT.dropout_add_fwd(ok, ok[:2], 0.1, 1)

    # the public functions take the stock composition for those inputs
    def same_as_stock(ours, stock):
        torch.manual_seed(3)
        a = ours()
        torch.manual_seed(3)
        assert torch.equal(a, stock())

    for t in (odd, f32):
        same_as_stock(lambda: hidden_dropout(t, 0.1, True),
                      lambda: F.dropout(t, 0.1, True))
        same_as_stock(lambda: dropout_add(t, t, 0.1, True),
                      lambda: t + F.dropout(t, 0.1, True))
        same_as_stock(lambda: gelu_dropout(t, 0.1, True),
                      lambda: F.dropout(F.gelu(t), 0.1, True))
    for p in (0.0, 1.0):
        same_as_stock(lambda: hidden_dropout(ok, p, True),
                      lambda: F.dropout(ok, p, True))
        same_as_stock(lambda: gelu_dropout(ok, p, True),
                      lambda: F.dropout(F.gelu(ok), p, True))
    assert torch.equal(hidden_dropout(ok, 0.1, False), ok)


def _saved_dtypes():
    from vit_10b_fsdp_example_amd.models.vit import Block

    torch.manual_seed(0)
    blk = Block(640, 4, drop=0.2).to(_dev(), torch.bfloat16).train()
    x = torch.randn(2, 256, 640, device=_dev(), dtype=torch.bfloat16,
                    requires_grad=True)
    dtypes = []

    def pack(t):
        dtypes.append(t.dtype)
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = blk(x)
    out.float().sum().backward()
    assert torch.isfinite(x.grad.float()).all()
    return dtypes


def test_block_stores_no_mask(monkeypatch):
    """The memory claim: with hidden dropout on, a block's forward saves
    no mask tensor for the backward."""
    monkeypatch.delenv("VITFSDP_NATIVE_DROPOUT", raising=False)
    dtypes = _saved_dtypes()
    assert dtypes
    assert torch.bool not in dtypes and torch.uint8 not in dtypes, dtypes
    # the probe does see the stock path's masks
    monkeypatch.setenv("VITFSDP_NATIVE_DROPOUT", "0")
    assert torch.bool in _saved_dtypes()


def test_hidden_dropout_with_checkpointing():
    """--mlp_dropout / --pos_dropout under gradient checkpointing, after
    test_att_dropout_with_checkpointing: the per-site seeds come from
    the CPU generator, so the recompute must regenerate the forward's
    masks.  Two identical runs agree, and so does a run without
    checkpointing under the same seed, which has no recompute at all."""
    from vit_10b_fsdp_example_amd.cli import parse_args
    from vit_10b_fsdp_example_amd import dist as xdist
    from vit_10b_fsdp_example_amd.models import build_fsdp_vit_model
    from vit_10b_fsdp_example_amd.ops import CrossEntropyLoss, FusedAdamW
    from vit_10b_fsdp_example_amd.parallel import CommContext

    def build(extra=()):
        CommContext.reset()
        cfg = parse_args([
            "--fake_data", "--image_size", "224", "--patch_size", "14",
            "--embed_dim", "640", "--num_heads", "4", "--num_blocks", "2",
            "--num_classes", "100", "--batch_size", "8",
            "--num_workers", "0", "--mlp_dropout", "0.2",
            "--pos_dropout", "0.1", *extra,
        ])
        device = xdist.init_distributed()
        torch.manual_seed(0)
        model = build_fsdp_vit_model(cfg, device, compute_dtype=torch.bfloat16)
        assert cfg.grad_ckpt == ("--no_grad_ckpt" not in extra)
        x = torch.randn(8, 3, 224, 224, device=device, dtype=torch.bfloat16)
        y = torch.randint(0, 100, (8,), device=device)
        return model, x, y

    def one_step_grads(extra=()):
        model, x, y = build(extra)
        torch.manual_seed(4321)  # governs the per-call dropout seeds
        loss = CrossEntropyLoss()(model(x), y)
        loss.backward()
        grads = [
            u.flat_param._comm_grad.clone() for u in model._all_units()
        ]
        return float(loss.detach()), grads

    def assert_same(a, b, what):
        (l1, g1), (l2, g2) = a, b
        assert abs(l1 - l2) < 5e-3 * max(abs(l1), 1.0), (
            f"{what}: dropout fwd diverged: {l1} vs {l2}")
        # a wrong recompute mask moves gradients by O(1); GEMM algorithm
        # jitter between in-process runs by up to ~1e-2 max-rel
        for u, v in zip(g1, g2):
            scale = u.float().abs().max() + 1e-6
            rel = (u.float() - v.float()).abs().max() / scale
            assert float(rel) < 5e-2, f"{what}: mask mismatch: rel {rel}"

    r1 = one_step_grads()
    r2 = one_step_grads()
    r3 = one_step_grads(["--no_grad_ckpt"])
    assert_same(r1, r2, "ckpt vs ckpt")
    assert_same(r1, r3, "ckpt vs no ckpt")

    f1 = one_step_grads(["--fuse_residual"])
    f2 = one_step_grads(["--fuse_residual", "--no_grad_ckpt"])
    assert_same(f1, f2, "fuse_residual, ckpt vs no ckpt")
    # same per-site seed order in both interfaces: the same masks, and
    # values that differ by the branch's extra bf16 rounding only
    assert abs(f1[0] - r1[0]) < 5e-3 * max(abs(r1[0]), 1.0), (f1[0], r1[0])

    # training health over full steps (clip + AdamW included)
    model, x, y = build()
    opt = FusedAdamW(model.parameters(), lr=3e-3, weight_decay=0.1)
    loss_fn = CrossEntropyLoss()
    torch.manual_seed(4321)
    losses = []
    for _ in range(8):
        loss = loss_fn(model(x), y)
        loss.backward()
        model.clip_grad_norm_(1.0, defer_scale=True)
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(float(loss.detach()))
    assert all(v == v for v in losses), f"NaN loss: {losses}"
    assert min(losses) < losses[0], f"no progress under dropout: {losses}"
