"""csrc/transpose.hip and the TN weight-gradient route of
ops/linear.py TunedGemmMode on the GPU.

Reordered sums and GEMMs are held to the criterion of the project's
earlier kernel changes (profiles/PROFILES.md): the max abs error
against the fp64 result computed from the same bf16 inputs may exceed
the stock op's by at most one bf16 ulp of the largest reference value.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None

# partial tiles in each dimension, fewer rows than a tile, rows that are
# no multiple of 8 (scalar stores), more than one tile per block
# (256 x 15360: 960 tiles)
SHAPES = [(1, 8), (7, 8), (65, 72), (15, 5120), (1037, 1024), (256, 15360)]


def _dev():
    return torch.device("cuda", 0)


def _randn(rows, cols, seed=0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) + shift
    return x.to(_dev(), torch.bfloat16)


def _bf16_ulp(v):
    """Spacing of bf16 (8 significand bits) at magnitude v."""
    return 2.0 ** (math.floor(math.log2(v)) - 7) if v > 0 else 0.0


def _within(err_new, err_stock, ref, what):
    bound = err_stock + _bf16_ulp(ref.abs().max().item())
    print(f"{what}: max err new {err_new:.4g}, stock {err_stock:.4g}, "
          f"max |ref| {ref.abs().max().item():.4g}, bound {bound:.4g}")
    assert err_new <= bound, (what, err_new, bound)


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_transpose2d(rows, cols):
    x = _randn(rows, cols)
    y = EXT.transpose2d(x)
    assert y.shape == (cols, rows) and y.is_contiguous()
    assert torch.equal(y, x.t().contiguous())
    assert torch.equal(EXT.transpose2d(x), y)


@pytest.mark.parametrize("shift", [0.0, 1.0])  # 1.0: sums that keep growing
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_transpose_colsum(rows, cols, shift):
    x = _randn(rows, cols, seed=1, shift=shift)
    y, colsum = EXT.transpose_colsum(x)
    assert torch.equal(y, x.t().contiguous())
    assert colsum.shape == (cols,) and colsum.dtype == torch.bfloat16
    ref = x.double().sum(0)
    err = (colsum.double() - ref).abs().max().item()
    err_stock = (x.sum(0).double() - ref).abs().max().item()
    _within(err, err_stock, ref, f"colsum {rows}x{cols} shift {shift}")
    # fixed summation order: the same bytes on every call
    y2, colsum2 = EXT.transpose_colsum(x)
    assert torch.equal(y2, y) and torch.equal(colsum2, colsum)


def test_transpose_refuses_what_it_would_have_to_copy():
    x = _randn(16, 64)
    for fn in (EXT.transpose2d, EXT.transpose_colsum):
        with pytest.raises(RuntimeError, match="bf16"):
            fn(x.float())
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(x.t())
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(x[:, :32])
        with pytest.raises(RuntimeError, match="multiple of 8"):
            fn(_randn(16, 60))
        with pytest.raises(RuntimeError, match="2-D"):
            fn(x.view(2, 8, 64))


def test_transpose_no_rows():
    x = torch.empty(0, 16, device=_dev(), dtype=torch.bfloat16)
    y, colsum = EXT.transpose_colsum(x)
    assert y.shape == (16, 0) and torch.equal(colsum, torch.zeros_like(colsum))
    assert EXT.transpose2d(x).shape == (16, 0)


# ---- GELU backward that also writes dx^T ----------------------------------

# one partial tile; rows that are no multiple of 8 with chunks that end
# inside a 64-row tile and several 256-column tiles; the 10B width with
# fewer rows than a tile
GELU_SHAPES = [(16, 64), (1037, 1024), (33, 20480)]


@pytest.mark.parametrize("rows,hid", GELU_SHAPES)
def test_gelu_bwd_colsum_t(rows, hid):
    dy = _randn(rows, hid, seed=7)
    x = _randn(rows, hid, seed=8) * 2.0
    dx0, colsum0 = EXT.gelu_bwd_colsum(dy, x)
    dx, colsum, dxt = EXT.gelu_bwd_colsum_t(dy, x)
    assert torch.equal(dx, dx0)
    assert torch.equal(colsum, colsum0)
    assert dxt.shape == (hid, rows) and dxt.is_contiguous()
    assert torch.equal(dxt, dx0.t().contiguous())


def test_gelu_bwd_colsum_t_chunk_boundaries_and_leading_dims():
    """2048 rows x 2048 columns: 16-row chunks, 16-byte stores throughout;
    34816 x 264: 17-row chunks, so most chunk boundaries cut an 8-row
    group of the transposed store, which is then stored by element."""
    for b, t, hid in ((8, 256, 2048), (4, 8704, 264)):
        dy = _randn(b * t, hid, seed=9).view(b, t, hid)
        x = _randn(b * t, hid, seed=10).view(b, t, hid)
        dx0, colsum0 = EXT.gelu_bwd_colsum(dy, x)
        dx, colsum, dxt = EXT.gelu_bwd_colsum_t(dy, x)
        assert dx.shape == dy.shape and torch.equal(dx, dx0)
        assert torch.equal(colsum, colsum0)
        assert torch.equal(dxt, dx0.view(-1, hid).t().contiguous())


# ---- the route: dW = lt_gemm(dy^T, (x^T).t()) ----------------------------

WGRAD_SHAPES = [(64, 256, 256), (200, 512, 768), (2048, 512, 256)]


@pytest.fixture()
def linmod(monkeypatch):
    from vit_10b_fsdp_example_amd.ops import linear

    monkeypatch.delenv("VITFSDP_TN_WGRAD", raising=False)
    monkeypatch.setattr(linear, "_TN_MIN_ELEMS", 0)  # open the shape gate
    return linear


@pytest.mark.parametrize("k,out,inn", WGRAD_SHAPES)
def test_tn_wgrad_and_bias_sum(linmod, monkeypatch, k, out, inn):
    monkeypatch.setitem(linmod._GELU_CFG, "hid", 0)
    dy = _randn(k, out, seed=2)
    x = _randn(k, inn, seed=3)
    ref = dy.double().t() @ x.double()
    stock = torch.mm(dy.t(), x)
    with linmod.TunedGemmMode(table={}, native_wgrad=False) as m:
        dw = torch.mm(dy.t(), x)
        assert m.tn_hits == 1 and m._tn_stash is not None
        db = dy.sum(0, keepdim=True)
        assert m.tn_dbias_hits == 1 and m._tn_stash is None
    assert dw.shape == (out, inn) and dw.is_contiguous()
    _within((dw.double() - ref).abs().max().item(),
            (stock.double() - ref).abs().max().item(), ref,
            f"dW K{k} {out}x{inn}")
    sref = dy.double().sum(0, keepdim=True)
    assert db.shape == (1, out)
    _within((db.double() - sref).abs().max().item(),
            (dy.sum(0, keepdim=True).double() - sref).abs().max().item(),
            sref, f"db K{k} {out}")


# ---- one Block, forward + backward ----------------------------------------

DIM, HEADS, BATCH, TOKENS = 256, 4, 2, 256  # 512 token rows


def _block_and_input(device, dtype):
    from vit_10b_fsdp_example_amd.models.vit import Block

    torch.manual_seed(0)
    blk = Block(DIM, HEADS)  # same CPU-seeded init for every copy
    # biases and LN offsets start at zero; move them so that a wrong
    # bias gradient cannot hide
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    x = torch.randn(BATCH, TOKENS, DIM, generator=g)
    dout = torch.randn(BATCH, TOKENS, DIM, generator=g)
    # the values every copy computes from are the bf16-rounded ones
    blk = blk.to(torch.bfloat16).to(device, dtype)
    x = x.to(torch.bfloat16).to(device, dtype).requires_grad_(True)
    return blk, x, dout.to(torch.bfloat16).to(device, dtype)


def _block_grads(blk, x, dout, ckpt, mode):
    from vit_10b_fsdp_example_amd.parallel.checkpoint import checkpoint_module

    run = checkpoint_module(blk) if ckpt else blk
    with mode:
        run(x).backward(dout)
    grads = {n: p.grad.detach().double().cpu()
             for n, p in blk.named_parameters()}
    grads["input"] = x.grad.detach().double().cpu()
    return grads


@pytest.fixture(scope="module")
def block_reference():
    """fp64 gradients on the CPU from the same bf16 parameters and input,
    computed once."""
    import contextlib

    blk, x, dout = _block_and_input(torch.device("cpu"), torch.float64)
    return _block_grads(blk, x, dout, False, contextlib.nullcontext())


@pytest.mark.parametrize("fused_dgelu", [True, False])
@pytest.mark.parametrize("ckpt", [False, True])
def test_block_gradients(linmod, monkeypatch, block_reference, ckpt,
                         fused_dgelu):
    monkeypatch.setenv("VITFSDP_FUSED_DGELU_DBIAS", "1" if fused_dgelu else "0")
    ref = block_reference

    def run(route_on):
        monkeypatch.setenv("VITFSDP_TN_WGRAD", "1" if route_on else "0")
        blk, x, dout = _block_and_input(_dev(), torch.bfloat16)
        mode = linmod.TunedGemmMode(table={}, native_wgrad=False)
        assert mode.tn_wgrad == route_on
        assert mode.fused_dgelu == fused_dgelu
        return _block_grads(blk, x, dout, ckpt, mode), mode

    off, m_off = run(False)
    on, m_on = run(True)
    assert m_off.tn_hits == 0 and m_off.tn_dbias_hits == 0
    # qkv, proj, fc1, fc2; fc1's bias sum is the GELU backward's when
    # that kernel is on, the route's otherwise
    assert m_on.tn_hits == 4
    assert m_on.tn_dbias_hits == (3 if fused_dgelu else 4)
    assert m_on.tn_dbias_hits + m_on.dbias_hits == 4
    assert m_on._tn_stash is None and m_on._dgelu_stash is None
    assert set(on) == set(ref)
    for name in sorted(ref):
        r = ref[name]
        _within((on[name] - r).abs().max().item(),
                (off[name] - r).abs().max().item(), r, name)
