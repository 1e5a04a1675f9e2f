"""_C.gelu_dropout_bwd_colsum and _C.gelu_dropout_bwd_colsum_t (the DROP
instantiations of csrc/gelu.hip): the backward of dropout(gelu(x)) with
the column sums of its bf16 result (fc1's bias gradient) and dx^T in the
same pass.  dx is gelu_dropout_bwd's bit for bit, the sums sit inside the
bound of tests/test_gpu_gelu_bwd_colsum.py, and one Block under
TunedGemmMode takes the route, checkpointed or not."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None

from vit_10b_fsdp_example_amd.ops import hidden_dropout_mask  # noqa: E402

# (3, 2056): a ragged 256-column tile; (1037, 1024): rows that are no
# multiple of 8 and chunks that end inside a 64-row tile; (33, 20480):
# the 10B width with fewer rows than a tile
SHAPES = [(1, 8), (5, 64), (257, 2048), (3, 2056), (1037, 1024), (33, 20480)]
PS = [0.1, 0.5]
SEEDS = [0, 2 ** 31 - 2]

# as tests/test_gpu_hidden_dropout.py: zero crossing of the derivative
# (~ -0.75), erf saturation, exp underflow
SPECIAL = [0.0, 0.75, -0.75, 10.0, -10.0, 40.0, -40.0]


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _inputs(rows, cols, seed=0):
    """(dy, x) bf16 on the GPU; every 5th element of x takes one of the
    special values in turn.  Shared between tests: never modified."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * 2.0
    dy = torch.randn(rows, cols, generator=g)
    flat = x.view(-1)
    idx = torch.arange(0, flat.numel(), 5)
    flat[idx] = torch.tensor(SPECIAL)[torch.arange(idx.numel()) % len(SPECIAL)]
    return tuple(t.to(_dev(), torch.bfloat16) for t in (dy, x))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_colsum_in_bound(colsum, dx, what):
    """colsum against the fp64 column sum of the kernel's own dx: one bf16
    rounding plus the worst-case fp32 accumulation error over the rows
    (the bound of tests/test_gpu_gelu_bwd_colsum.py)."""
    dx64 = dx.double().reshape(-1, dx.shape[-1])
    rows = dx64.shape[0]
    cref = dx64.sum(0)
    cerr = (colsum.double() - cref).abs()
    cbound = 2.0 ** -7 * cref.abs() + rows * 2.0 ** -24 * dx64.abs().sum(0)
    print(f"{what}: colsum max err {cerr.max().item():.3e}, min slack "
          f"{(cbound - cerr).min().item():.3e}")
    assert bool((cerr <= cbound).all()), (cerr - cbound).max().item()


def _check_both_variants(dy, x, p, seed):
    hid = dy.shape[-1]
    want = EXT.gelu_dropout_bwd(dy, x, p, seed)
    dx, colsum = EXT.gelu_dropout_bwd_colsum(dy, x, p, seed)
    dx_t, colsum_t, dxt = EXT.gelu_dropout_bwd_colsum_t(dy, x, p, seed)
    for got in (dx, dx_t):
        assert got.shape == dy.shape and got.dtype == torch.bfloat16
        assert torch.equal(_bits(got), _bits(want))
    assert colsum.shape == (hid,) and colsum.dtype == torch.bfloat16
    _assert_colsum_in_bound(colsum, dx, f"{tuple(dy.shape)} p={p}")
    _assert_colsum_in_bound(colsum_t, dx_t, f"{tuple(dy.shape)} p={p} _t")
    assert torch.equal(_bits(colsum_t), _bits(colsum))
    assert dxt.shape == (hid, dy.numel() // hid) and dxt.is_contiguous()
    assert dxt.dtype == torch.bfloat16
    assert torch.equal(_bits(dxt), _bits(want.view(-1, hid).t().contiguous()))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("rows,hid", SHAPES)
def test_dx_colsum_and_transpose(rows, hid, p, seed):
    dy, x = _inputs(rows, hid)
    _check_both_variants(dy, x, p, seed)


def test_chunk_boundaries_and_leading_dims():
    """2048 rows x 2048 columns: 16-row chunks, 16-byte stores throughout;
    34816 x 264: 17-row chunks, so most chunk boundaries cut an 8-row
    group of the transposed store, which is then stored by element.  Both
    as [B, T, hid]: rows are all leading dims, and the mask's row is the
    flattened one."""
    for b, t, hid in ((8, 256, 2048), (4, 8704, 264)):
        dy, x = _inputs(b * t, hid, seed=9)
        _check_both_variants(dy.view(b, t, hid), x.view(b, t, hid), 0.1, 1234)


def test_dropped_positions_are_zero_and_leak_nothing():
    rows, hid, p, seed = 37, 64, 0.5, 1234
    dy, x = (t.clone() for t in _inputs(rows, hid, seed=2))
    mask = hidden_dropout_mask(seed, rows, hid, p)
    # one dropped and one kept position for each of dy (NaN) and x (inf),
    # in four different columns
    cols, picks = [], {}
    for name, keep in (("dy_drop", False), ("dy_keep", True),
                       ("x_drop", False), ("x_keep", True)):
        r, c = next((r, c) for c in range(hid) if c not in cols
                    for r in range(rows) if bool(mask[r, c]) == keep)
        cols.append(c)
        picks[name] = (r, c)
    dy[picks["dy_drop"]] = float("nan")
    dy[picks["dy_keep"]] = float("nan")
    x[picks["x_drop"]] = float("inf")
    x[picks["x_keep"]] = float("inf")  # inf * exp(-inf) = inf * 0

    want = EXT.gelu_dropout_bwd(dy, x, p, seed)
    dx, colsum = EXT.gelu_dropout_bwd_colsum(dy, x, p, seed)
    dx_t, colsum_t, dxt = EXT.gelu_dropout_bwd_colsum_t(dy, x, p, seed)
    gmask = mask.to(_dev())
    for got, cs in ((dx, colsum), (dx_t, colsum_t)):
        assert torch.equal(_bits(got), _bits(want))
        assert bool((_bits(got)[~gmask] == 0).all())  # exactly +0
        cs = cs.float()
        for name in ("dy_drop", "x_drop"):
            assert _bits(got)[picks[name]] == 0
            assert torch.isfinite(cs[picks[name][1]])
        for name in ("dy_keep", "x_keep"):
            assert not torch.isfinite(got.float()[picks[name]])
            assert not torch.isfinite(cs[picks[name][1]])
        others = torch.ones(hid, dtype=torch.bool, device=_dev())
        others[[picks["dy_keep"][1], picks["x_keep"][1]]] = False
        assert torch.isfinite(cs[others]).all()
    assert torch.equal(_bits(dxt), _bits(want.t().contiguous()))


def test_refusals_and_empty_input():
    dev = _dev()
    odd = torch.randn(4, 100, device=dev, dtype=torch.bfloat16)
    f32 = torch.randn(4, 64, device=dev)
    ok = torch.randn(4, 64, device=dev, dtype=torch.bfloat16)
    for fn in (EXT.gelu_dropout_bwd_colsum, EXT.gelu_dropout_bwd_colsum_t):
        with pytest.raises(RuntimeError, match="multiple of 8"):
            fn(odd, odd, 0.1, 1)
        with pytest.raises(RuntimeError, match="bf16 only"):
            fn(f32, f32, 0.1, 1)
        for p in (0.0, 1.0):
            with pytest.raises(RuntimeError, match=r"p must be in \(0, 1\)"):
                fn(ok, ok, p, 1)
        with pytest.raises(RuntimeError, match="one shape"):
            fn(ok, ok[:2], 0.1, 1)
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(ok.t(), ok.t(), 0.1, 1)
        empty = torch.empty(0, 64, device=dev, dtype=torch.bfloat16)
        out = fn(empty, empty, 0.1, 1)
        assert out[0].shape == (0, 64)
        assert out[1].shape == (64,) and bool((_bits(out[1]) == 0).all())
        if len(out) == 3:
            assert out[2].shape == (64, 0)


# ---- one Block under TunedGemmMode -----------------------------------------


def _block_run(linmod, ckpt):
    """Gradients of one Block forward+backward with drop = 0.2 under the
    mode, and dx of the GELU+dropout backward as fc1's output receives
    it."""
    from vit_10b_fsdp_example_amd.models.vit import Block
    from vit_10b_fsdp_example_amd.parallel.checkpoint import checkpoint_module

    torch.manual_seed(0)
    blk = Block(640, 4, drop=0.2).to(_dev(), torch.bfloat16).train()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():  # biases start at zero: move them
        for q in blk.parameters():
            if q.dim() == 1:
                q.add_((0.1 * torch.randn(q.shape, generator=g)).to(q))
    x = torch.randn(2, 256, 640, generator=g).to(_dev(), torch.bfloat16)
    x.requires_grad_(True)
    dout = torch.randn(2, 256, 640, generator=g).to(_dev(), torch.bfloat16)
    seen = []

    def watch(mod, inp, out):
        if out.requires_grad:
            out.register_hook(lambda grad: seen.append(grad.detach().clone()))

    hook = blk.mlp.fc1.register_forward_hook(watch)
    run = checkpoint_module(blk) if ckpt else blk
    mode = linmod.TunedGemmMode(table={}, native_wgrad=False)
    torch.manual_seed(4321)  # governs the per-site dropout seeds
    with mode:
        out = run(x)
        before = (mode.dgelu_drop_hits, mode.dbias_hits, mode.tn_hits)
        out.backward(dout)
        assert mode._dgelu_stash is None and mode._tn_stash is None
    hook.remove()
    grads = {n: q.grad.detach().float() for n, q in blk.named_parameters()}
    grads["input"] = x.grad.detach().float()
    assert before == (0, 0, 0)  # the counters below are the backward's
    return grads, mode, seen[-1]


@pytest.fixture()
def linmod(monkeypatch):
    from vit_10b_fsdp_example_amd.ops import linear

    for name in ("VITFSDP_TN_WGRAD", "VITFSDP_TN_DGELU_T",
                 "VITFSDP_NATIVE_DROPOUT", "VITFSDP_FUSED_GELU"):
        monkeypatch.delenv(name, raising=False)
    return linear


@pytest.mark.parametrize("tn", [True, False])
def test_block_takes_the_route(linmod, monkeypatch, tn):
    """tn: the TN weight-gradient gate open and the _t kernel routed
    (_DGELU_DROP_T, off by default), so that fc1's GEMM takes the parked
    dx^T; otherwise the gate at its default, closed at this size, and the
    plain kernel as it is routed by default."""
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", 0 if tn else -1)
    monkeypatch.setattr(linmod, "_DGELU_DROP_T", tn)
    tn_hits = 4 if tn else 0  # qkv, proj, fc1, fc2
    monkeypatch.setenv("VITFSDP_FUSED_DGELU_DBIAS", "0")
    off, m_off, _ = _block_run(linmod, ckpt=False)
    assert m_off.dgelu_drop_hits == 0 and m_off.dbias_hits == 0
    assert m_off.tn_hits == m_off.tn_dbias_hits == tn_hits

    monkeypatch.setenv("VITFSDP_FUSED_DGELU_DBIAS", "1")
    for ckpt in (False, True):
        on, m, dx = _block_run(linmod, ckpt=ckpt)
        # one routed GELU+dropout backward, its sums answering fc1's bias
        # gradient, and fc1's weight gradient among the TN GEMMs
        assert m.dgelu_drop_hits == 1 and m.dgelu_hits == 0
        assert m.dbias_hits == 1
        assert m.tn_hits == tn_hits
        assert m.tn_dbias_hits == (3 if tn else 0)
        assert dx.shape == (2, 256, 2560)
        _assert_colsum_in_bound(on["mlp.fc1.bias"].bfloat16(), dx,
                                f"fc1.bias.grad ckpt={ckpt}")
        # dx is bit-identical between the routes, so what is left is GEMM
        # algorithm jitter (the tolerance of
        # test_hidden_dropout_with_checkpointing)
        assert set(on) == set(off)
        for name in sorted(off):
            if name == "mlp.fc1.bias":
                continue
            scale = off[name].abs().max() + 1e-6
            rel = float((on[name] - off[name]).abs().max() / scale)
            assert rel < 5e-2, f"{name} ckpt={ckpt}: rel {rel}"
