"""csrc/wgemm.hip after its ladder pass (clustered 2-D tile mapping,
direct-to-LDS staging with a source-side XOR): every element of
C = A^T B against an fp64 product of the same bf16 inputs.

Tolerance, derived rather than tuned.  Rounding the result to bf16
(round to nearest, 8 significand bits) costs at most 2^-9 relative;
fp32 accumulation of K products costs at most about K * 2^-24 *
(|A|^T |B|).  With a factor 2 on each term:

    |c - ref| <= 2^-8 * |ref| + K * 2^-23 * (|A|^T |B|)     elementwise

with no element excluded.  test_bound_holds_for_fp32_matmul checks on the
CPU that a plain fp32 matmul rounded to bf16 stays inside it for the
seeds used here, so the bound is one a correct kernel meets.

Every call gets fresh seeded random operands: a tile the kernel never
wrote cannot inherit a right answer from recycled allocator memory.
"""

import pytest
import torch

import vit_10b_fsdp_example_amd.ops.linear as linear_mod

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None

# K = 64*j: j = 1 is the prologue only, j = 2 uses both LDS buffers,
# j = 3 is an odd count, j = 5 is steady state plus drain.  The shipped
# pipeline keeps d = 1 K-tile in flight; j = 1 .. 5 covers d + 2 = 3
# with room for one more stage.
K_EDGES = [64, 128, 192, 256, 320]

# tile grids (M/256, N/256) at K = 128, one per branch of
# xcd_cluster_tile (csrc/mfma_tiles.h)
GRIDS = [
    (1, 1),  # single tile
    (3, 1),  # count not a multiple of 8: identity mapping
    (2, 4),  # multiple-of-8 count, one tile per XCD
    (8, 4),  # clustered, 2x4 sub-rectangles
    (4, 6),  # the sy = 2 branch
    (8, 1),  # the sx = 8 branch
    (3, 8),  # multiple of 8 but not divisible: M-major fallback
]


def _seed(k, m, n):
    return 1000003 * k + 1009 * m + n


def _operands(k, m, n, device):
    g = torch.Generator(device="cpu")
    g.manual_seed(_seed(k, m, n))
    a = torch.randn(k, m, generator=g).to(torch.bfloat16)
    b = torch.randn(k, n, generator=g).to(torch.bfloat16)
    return a.to(device), b.to(device)


def _check(c, a, b, what):
    """All elements of c against the fp64 product of the bf16 inputs."""
    k = a.shape[0]
    a64, b64 = a.double(), b.double()
    ref = a64.t() @ b64
    bound = 2.0 ** -8 * ref.abs() + k * 2.0 ** -23 * (a64.abs().t() @ b64.abs())
    err = (c.double() - ref).abs()
    assert torch.isfinite(c.float()).all(), f"{what}: non-finite output"
    excess = err - bound
    worst = int(excess.argmax())
    i, j = divmod(worst, c.shape[1])
    n_bad = int((excess > 0).sum())
    assert n_bad == 0, (
        f"{what}: {n_bad} of {c.numel()} elements outside the bound; worst "
        f"at [{i}, {j}] (tile {i // 256}, {j // 256}): |err| = "
        f"{float(err[i, j]):.4g}, bound = {float(bound[i, j]):.4g}"
    )


def _run(k, m, n, with_bias=False):
    a, b = _operands(k, m, n, torch.device("cuda", 0))
    out = EXT.wgrad_gemm(a, b, with_bias)
    _check(out[0], a, b, f"wgrad_gemm K{k} M{m} N{n} bias={with_bias}")
    return a, out


@pytest.mark.gpu
@pytest.mark.parametrize("k", K_EDGES)
def test_k_loop_edges(k):
    _run(k, 256, 256)


@pytest.mark.gpu
@pytest.mark.parametrize("gx,gy", GRIDS)
def test_tile_mapping_branches(gx, gy):
    """A tile mapped twice or never shows up as a whole wrong tile."""
    _run(128, 256 * gx, 256 * gy)


@pytest.mark.gpu
def test_with_bias_instantiation():
    """The WITH_BIAS kernel shares the staging and the reads: same bound
    for C, and fp32 column sums of dY for the bias gradient."""
    a, (c, db) = _run(192, 512, 256, with_bias=True)
    k = a.shape[0]
    ref = a.double().sum(0)
    # fp32 accumulation of K terms (split over lanes and atomics)
    bound = k * 2.0 ** -23 * a.double().abs().sum(0)
    assert ((db.double() - ref).abs() <= bound).all()


@pytest.mark.gpu
def test_dispatch_mode_rectangular(monkeypatch):
    """M != N, both > 256, K = 192, through NativeWgradMode against
    stock autograd (and both against fp64)."""
    import torch.nn as nn

    monkeypatch.setattr(linear_mod, "_MIN_TILES", 0)
    dev = torch.device("cuda", 0)
    k, n_in, n_out = 192, 512, 768
    g = torch.Generator(device="cpu")
    g.manual_seed(_seed(k, n_out, n_in))
    lin = nn.Linear(n_in, n_out).to(dev, torch.bfloat16)
    x = torch.randn(k, n_in, generator=g).to(dev, torch.bfloat16)
    x.requires_grad_(True)
    dy = torch.randn(k, n_out, generator=g).to(dev, torch.bfloat16)

    lin(x).backward(dy)
    stock_w, stock_x = lin.weight.grad.clone(), x.grad.clone()
    lin.weight.grad = lin.bias.grad = x.grad = None

    mode = linear_mod.NativeWgradMode()
    with mode:
        lin(x).backward(dy)
    assert mode.hits == 1, "dW mm was not routed to the native kernel"
    got_w = lin.weight.grad

    # dW [out, in] = dy^T x
    _check(got_w, dy, x.detach(), "NativeWgradMode dW")
    _check(stock_w, dy, x.detach(), "stock dW")
    # both within the bound of the same reference: twice the bound apart
    ref = dy.double().t() @ x.detach().double()
    bound = 2.0 ** -8 * ref.abs() + k * 2.0 ** -23 * (
        dy.double().abs().t() @ x.detach().double().abs())
    assert ((got_w.double() - stock_w.double()).abs() <= 2 * bound).all()
    # the input gradient is not routed: same library call as stock
    torch.testing.assert_close(x.grad, stock_x, atol=1e-3, rtol=1e-3)


# smallest shape the default gate accepts: 16 x 16 = 256 tiles
GATE_SHAPE = (4096, 4096, 64)  # m, n, k

# routed by default only where the kernel beat the library in the step
# (profiles/PROFILES.md "wgemm NT ladder")
GATE_10B = {
    (15360, 5120): True,   # qkv
    (5120, 5120): True,    # proj
    (20480, 5120): False,  # fc1 / fc2
}


@pytest.mark.gpu
def test_gate_accepted_shape_runs():
    """What the Python gate accepts, the kernel's own shape check must
    accept too (and compute)."""
    m, n, k = GATE_SHAPE
    assert linear_mod._wgrad_mm_shapes_ok(m, n, k)
    _run(k, m, n)


def test_gate_arithmetic(monkeypatch):
    monkeypatch.setattr(linear_mod, "_MIN_TILES", 256)
    ok = linear_mod._wgrad_mm_shapes_ok
    m, n, k = GATE_SHAPE
    assert ok(m, n, k)
    assert not ok(m, n, k + 32)      # K must be a multiple of 64
    assert not ok(m + 128, n, k)     # M a multiple of 256
    assert not ok(m, n + 128, k)     # N a multiple of 256
    assert not ok(m - 256, n, k)     # 15 x 16 tiles: below _MIN_TILES
    # the four ViT-10B dW shapes (K = batch * tokens), either orientation
    for m, n in GATE_10B:
        assert ok(m, n, 32768) is GATE_10B[(m, n)], (m, n)
        assert ok(n, m, 32768) is GATE_10B[(m, n)], (n, m)
    monkeypatch.setattr(linear_mod, "_MIN_TILES", 0)
    assert ok(256, 256, 64)
    assert ok(768, 512, 192)


def test_bound_holds_for_fp32_matmul():
    """The bound is one a correct implementation meets: a plain fp32
    matmul rounded to bf16, same seeds, stays inside it."""
    shapes = [(k, 256, 256) for k in K_EDGES]
    shapes += [(128, 256 * gx, 256 * gy) for gx, gy in GRIDS]
    shapes += [(192, 512, 256)]
    for k, m, n in shapes:
        a, b = _operands(k, m, n, torch.device("cpu"))
        c = (a.float().t() @ b.float()).to(torch.bfloat16)
        _check(c, a, b, f"fp32 matmul K{k} M{m} N{n}")
