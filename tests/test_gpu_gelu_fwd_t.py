"""_C.gelu_fwd_t (csrc/gelu.hip) and the Block that rebuilds gelu(h) with
it in the backward, on the GPU.  The kernel's result is F.gelu's in bits
(exact erf in fp32, one rounding to bf16), so every check is torch.equal."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None


def _dev():
    return torch.device("cuda", 0)


def _equal_with_nans(got, want):
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan)
    assert torch.equal(got.masked_fill(nan, 0), want.masked_fill(nan, 0))


def test_every_bf16_value():
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    h = bits.view(torch.bfloat16).view(256, 256).to(_dev())
    want = F.gelu(h).t().contiguous()
    got = EXT.gelu_fwd_t(h)
    assert got.shape == (256, 256) and got.is_contiguous()
    assert int(want.isnan().sum()) > 0  # the NaN patterns are in there
    _equal_with_nans(got, want)


# one 64 x 64 tile, tile - 1 and tile + 1 in either direction, more than
# one tile each way; rows that are no multiple of 8 store by element
@pytest.mark.parametrize("cols", [8, 248, 256, 264, 520])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
def test_ragged_shapes(rows, cols):
    g = torch.Generator(device="cpu").manual_seed(rows * 1000 + cols)
    h = (2.0 * torch.randn(rows, cols, generator=g)).to(_dev(), torch.bfloat16)
    want = F.gelu(h).t().contiguous()
    got = EXT.gelu_fwd_t(h)
    assert got.shape == (cols, rows) and got.is_contiguous()
    assert got.dtype == torch.bfloat16
    assert torch.equal(got, want)
    assert torch.equal(EXT.gelu_fwd_t(h), got)  # the same bytes again


def test_more_than_one_tile_per_block():
    """2235 x 15360 is 35 x 240 tiles, past the 8192 from which a block
    walks two row tiles: 18 blocks per column, the last with one tile,
    and a ragged last row tile."""
    g = torch.Generator(device="cpu").manual_seed(7)
    h = torch.randn(2235, 15360, generator=g).to(_dev(), torch.bfloat16)
    assert torch.equal(EXT.gelu_fwd_t(h), F.gelu(h).t().contiguous())


def test_refuses_what_it_would_have_to_copy():
    h = torch.randn(16, 64, device=_dev(), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="bf16"):
        EXT.gelu_fwd_t(h.float())
    with pytest.raises(RuntimeError, match="contiguous"):
        EXT.gelu_fwd_t(h.t())
    with pytest.raises(RuntimeError, match="contiguous"):
        EXT.gelu_fwd_t(h[:, :32])
    with pytest.raises(RuntimeError, match="multiple of 8"):
        EXT.gelu_fwd_t(torch.randn(16, 60, device=_dev(),
                                   dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="2-D"):
        EXT.gelu_fwd_t(h.view(2, 8, 64))
    assert EXT.gelu_fwd_t(h[:0]).shape == (64, 0)


# ---- one Block, switch on against switch off --------------------------------

DIM, HEADS, BATCH, TOKENS = 256, 4, 2, 64  # 128 token rows, hid 1024


def _block_run(monkeypatch, switch):
    from vit_10b_fsdp_example_amd.models.vit import Block
    from vit_10b_fsdp_example_amd.ops import linear as linmod

    monkeypatch.setenv("VITFSDP_MLP_RECOMPUTE_ACT", switch)
    monkeypatch.delenv("VITFSDP_TN_WGRAD", raising=False)
    for name in ("VITFSDP_FUSED_GELU", "VITFSDP_TN_DGELU_T",
                 "VITFSDP_FUSED_DGELU_DBIAS"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", 0)  # open the shape gate
    torch.manual_seed(0)
    blk = Block(DIM, HEADS)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    x = torch.randn(BATCH, TOKENS, DIM, generator=g)
    dout = torch.randn(BATCH, TOKENS, DIM, generator=g)
    blk = blk.to(_dev(), torch.bfloat16)
    x = x.to(_dev(), torch.bfloat16).requires_grad_(True)
    dout = dout.to(_dev(), torch.bfloat16)
    calls = []

    def transposed(t, want_colsum):
        calls.append((tuple(t.shape), want_colsum))
        return linmod._transposed(t, want_colsum)

    monkeypatch.setitem(linmod._KERNELS, "transpose", transposed)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    with linmod.TunedGemmMode(table={}, native_wgrad=False) as m:
        out = blk(x)
        kept = torch.cuda.memory_allocated() - base
        out.backward(dout)
        assert m.tn_hits == 4  # qkv, proj, fc1, fc2 either way
    grads = {n: p.grad for n, p in blk.named_parameters()}
    grads["input"] = x.grad
    return out.detach(), grads, kept, calls


def test_block_switch_on_equals_switch_off(monkeypatch):
    """The only GEMM whose operand path changes, fc2's weight gradient,
    gets a bit-identical operand: outputs and gradients are equal."""
    # once unmeasured: the first run allocates the workspaces that stay
    _block_run(monkeypatch, "0")
    out_on, g_on, kept_on, calls_on = _block_run(monkeypatch, "1")
    out_off, g_off, kept_off, calls_off = _block_run(monkeypatch, "0")
    assert torch.equal(out_on, out_off)
    assert set(g_on) == set(g_off)
    for name in sorted(g_on):
        assert torch.equal(g_on[name], g_off[name]), name
    rows, hid = BATCH * TOKENS, 4 * DIM
    # fc2's x is no longer transposed by transpose2d ...
    assert ((rows, hid), False) in calls_off
    assert ((rows, hid), False) not in calls_on
    assert len(calls_on) == len(calls_off) - 1
    # ... and gelu(h) [rows, hid] bf16 is not kept between the passes
    print(f"kept after forward: on {kept_on} B, off {kept_off} B")
    assert kept_off - kept_on >= rows * hid * 2, (kept_on, kept_off)
