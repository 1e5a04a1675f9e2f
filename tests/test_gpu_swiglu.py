"""csrc/swiglu.hip on the GPU against the formula in fp64 on the bf16
inputs, the bit identities between its kernels, and one Block with
mlp_type="swiglu" against the stock composition.

Element bound: 2^-7 |ref| + 2^-20 floor with floor = |g||u| for a,
|da||u| for dg, |da||g| for du.  The first term is one bf16 rounding with
room for the fp32 steps before it, the second covers the fp32 cancellation
in 1 + g (1 - s) near g = -1.28, which row 0 holds."""

import copy

import pytest
import torch

from vit_10b_fsdp_example_amd.ops import (
    hidden_dropout_mask, swiglu_bwd_reference, swiglu_reference,
)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None

DEV = "cuda:0"
TILE = 128  # gate columns per block of swiglu_bwd_colsum_t_kernel


def _inputs(rows, H, scale=2.0):
    g = torch.Generator().manual_seed(rows * 1000 + H)
    h = (scale * torch.randn(rows, 2 * H, generator=g)).bfloat16()
    if rows:
        h[0, :H] = -1.28
    return torch.randn(rows, H, generator=g).bfloat16(), h


def _within(got, ref, floor, name, scale=1.0):
    tol = scale * (2.0 ** -7 * ref.abs() + 2.0 ** -20 * floor)
    err = (got.double().cpu() - ref).abs()
    assert bool((err <= tol).all()), (name, float((err - tol).max()))


def _check_values(da, h, a, dh, p=0.0, seed=0):
    H = da.shape[-1]
    g, u, d = h[:, :H].double(), h[:, H:].double(), da.double()
    scale = 1.0 / (1.0 - p)
    _within(a, swiglu_reference(h, p, seed), (g * u).abs(), "a", scale)
    dg, du = swiglu_bwd_reference(da, h, p, seed)
    _within(dh[:, :H], dg, (d * u).abs(), "dg", scale)
    _within(dh[:, H:], du, (d * g).abs(), "du", scale)


# 104 rows take the vector stores and cross row chunks; 63 and 130 store by
# element and cross a 64-row tile.  34824 x 8 has 18-row chunks: 8-row
# groups that straddle a chunk edge (bit identities only at that size).
@pytest.mark.parametrize("rows,H", [
    (r, c) for r in (1, 63, 104, 130)
    for c in (8, TILE - 8, TILE, TILE + 8, 2 * TILE + 8)] + [(34824, 8)])
def test_values_and_bit_identities(rows, H):
    da_c, h_c = _inputs(rows, H)
    da, h = da_c.to(DEV), h_c.to(DEV)
    a = EXT.swiglu_fwd(h, 0.0, 0)
    dh, colsum = EXT.swiglu_bwd_colsum(da, h, 0.0, 0)
    assert a.shape == (rows, H) and dh.shape == (rows, 2 * H)
    if rows < 1000:
        _check_values(da_c, h_c, a, dh)
    sums = dh.double().sum(0)
    tol = 2.0 ** -7 * sums.abs() + rows * 2.0 ** -24 * dh.double().abs().sum(0)
    assert bool(((colsum.double() - sums).abs() <= tol).all())
    dh_t, colsum_t, dht = EXT.swiglu_bwd_colsum_t(da, h)
    assert torch.equal(dh_t, dh) and torch.equal(colsum_t, colsum)
    assert dht.is_contiguous() and torch.equal(dht, dh.t())
    at = EXT.swiglu_fwd_t(h)
    assert at.is_contiguous() and torch.equal(at, a.t())
    # the same bytes again
    again = EXT.swiglu_bwd_colsum_t(da, h)
    assert all(torch.equal(x, y) for x, y in zip(again, (dh, colsum, dht)))
    assert torch.equal(EXT.swiglu_fwd_t(h), at)
    assert torch.equal(EXT.swiglu_fwd(h, 0.0, 0), a)
    assert torch.equal(EXT.swiglu_bwd_colsum(da, h, 0.0, 0)[0], dh)


def test_dropout_mask_and_values():
    rows, H, p, seed = 130, TILE + 8, 0.25, 1234
    da_c, h_c = _inputs(rows, H)
    a = EXT.swiglu_fwd(h_c.to(DEV), p, seed)
    dh, colsum = EXT.swiglu_bwd_colsum(da_c.to(DEV), h_c.to(DEV), p, seed)
    keep = hidden_dropout_mask(seed, rows, H, p).to(DEV)
    assert torch.equal(a == 0, ~keep) and 0 < int((~keep).sum())
    assert bool((dh[:, :H][~keep] == 0).all())
    assert bool((dh[:, H:][~keep] == 0).all())
    _check_values(da_c, h_c, a, dh, p, seed)
    sums = dh.double().sum(0)
    tol = 2.0 ** -7 * sums.abs() + rows * 2.0 ** -24 * dh.double().abs().sum(0)
    assert bool(((colsum.double() - sums).abs() <= tol).all())


def test_extreme_gates_stay_finite():
    da_c, h_c = _inputs(63, TILE + 8)
    h_c[:, :TILE + 8] = torch.where(h_c[:, :TILE + 8] > 0, 80.0, -80.0)
    a = EXT.swiglu_fwd(h_c.to(DEV), 0.0, 0)
    dh, _, dht = EXT.swiglu_bwd_colsum_t(da_c.to(DEV), h_c.to(DEV))
    assert bool(a.isfinite().all()) and bool(dh.isfinite().all())
    _check_values(da_c, h_c, a, dh)
    assert torch.equal(dht, dh.t())


def test_refusals_and_zero_rows():
    h = torch.randn(16, 64, device=DEV, dtype=torch.bfloat16)
    da = torch.randn(16, 32, device=DEV, dtype=torch.bfloat16)
    bad = [("bf16", h.float(), da), ("contiguous", h.t(), da),
           ("contiguous", h[:, :32], da[:, :16]),
           ("multiple of 8", h[:, :24].contiguous(), da[:, :12].contiguous()),
           ("even", torch.zeros(16, 63, device=DEV, dtype=torch.bfloat16), da)]
    for match, hh, dd in bad:
        with pytest.raises(RuntimeError, match=match):
            EXT.swiglu_fwd(hh, 0.0, 0)
        with pytest.raises(RuntimeError, match=match):
            EXT.swiglu_fwd_t(hh)
        with pytest.raises(RuntimeError, match=match):
            EXT.swiglu_bwd_colsum(dd, hh, 0.0, 0)
        with pytest.raises(RuntimeError, match=match):
            EXT.swiglu_bwd_colsum_t(dd, hh)
    with pytest.raises(RuntimeError, match="shape"):
        EXT.swiglu_bwd_colsum(da[:8].contiguous(), h, 0.0, 0)
    assert EXT.swiglu_fwd(h[:0], 0.0, 0).shape == (0, 32)
    assert EXT.swiglu_fwd_t(h[:0]).shape == (32, 0)
    dh, colsum, dht = EXT.swiglu_bwd_colsum_t(da[:0], h[:0])
    assert dh.shape == (0, 64) and dht.shape == (64, 0)
    assert not bool(colsum.any())


# ---- one Block ----------------------------------------------------------------

DIM, HEADS, BATCH, TOKENS = 256, 4, 2, 64  # 128 token rows, H = 768


def _block_run(monkeypatch, blk, x_c, dout_c, native="1", recompute="1"):
    from vit_10b_fsdp_example_amd.ops import linear as linmod

    monkeypatch.setenv("VITFSDP_NATIVE_SWIGLU", native)
    monkeypatch.setenv("VITFSDP_MLP_RECOMPUTE_ACT", recompute)
    for name in ("VITFSDP_TN_WGRAD", "VITFSDP_FUSED_GELU",
                 "VITFSDP_TN_DGELU_T", "VITFSDP_FUSED_DGELU_DBIAS"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", 0)  # open the shape gate
    blk = copy.deepcopy(blk).to(DEV)
    x = x_c.to(DEV).requires_grad_(True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    with linmod.TunedGemmMode(table={}, native_wgrad=False) as m:
        out = blk(x)
        kept = torch.cuda.memory_allocated() - base
        out.backward(dout_c.to(DEV))
    res = {n: p.grad for n, p in blk.named_parameters()}
    res.update(input=x.grad, output=out.detach())
    return res, kept, m


def test_block_against_the_composition(monkeypatch):
    from vit_10b_fsdp_example_amd.models.vit import Block

    torch.manual_seed(0)
    blk = Block(DIM, HEADS, mlp_type="swiglu")
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    blk = blk.bfloat16()
    x = torch.randn(BATCH, TOKENS, DIM, generator=g).bfloat16()
    dout = torch.randn(BATCH, TOKENS, DIM, generator=g).bfloat16()
    rows, H = BATCH * TOKENS, blk.mlp.fc2.in_features
    assert H == 768 and blk.mlp.fc1.out_features == 2 * H

    ref_blk = copy.deepcopy(blk).double()
    x64 = x.double().requires_grad_(True)
    out64 = ref_blk(x64)
    out64.backward(dout.double())
    ref = {n: p.grad for n, p in ref_blk.named_parameters()}
    ref.update(input=x64.grad, output=out64.detach())

    # once unmeasured: the first run allocates the workspaces that stay
    _block_run(monkeypatch, blk, x, dout)
    on, kept_on, m = _block_run(monkeypatch, blk, x, dout)
    assert m.dswiglu_hits == 1 and m.dbias_hits == 1 and m.tn_hits == 4
    _, kept_off, _ = _block_run(monkeypatch, blk, x, dout, recompute="0")
    print(f"kept after forward: on {kept_on} B, off {kept_off} B")
    assert kept_off - kept_on >= rows * H * 2, (kept_on, kept_off)
    comp, _, m = _block_run(monkeypatch, blk, x, dout, native="0")
    assert m.dswiglu_hits == 0

    def err(got, name):
        d = (got[name].double().cpu() - ref[name]).abs().max()
        return float(d / ref[name].abs().max())

    errs = {n: (err(on, n), err(comp, n)) for n in sorted(ref)}
    for n, (e_on, e_comp) in errs.items():
        print(f"{n}: native {e_on:.3e}, composition {e_comp:.3e}")
    for n, (e_on, e_comp) in errs.items():
        assert e_on <= 2.0 * e_comp, (n, e_on, e_comp)
