"""LayerNorm (csrc/layernorm.hip) and cross-entropy (csrc/cross_entropy.hip)
against fp64, at every D / C / row count where the kernels take another
path, under the bounds of tests/kernel_reference.py: bf16 outputs within
MARGIN x the rounding model's own error, whole tensor and per row; the
fp32 mean, rstd, lse and loss within per-element bounds derived from the
arithmetic.  The extension's entry points are called directly so that
the saved statistics are seen.  Also: every operand check of those entry
points, and the empty batch."""

import pytest
import torch

from tests import kernel_reference as kr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None

EPS = kr.LN_EPS


def _dev():
    return torch.device("cuda", 0)


def _finite(got, name):
    for k, t in got.items():
        assert bool(torch.isfinite(t.float()).all()), (name, k)


# --------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------

def _ln_cases():
    for rows, d in kr.LN_CASES:
        for family in kr.LN_FAMILIES:
            if family == "special" and rows < 3:
                continue
            yield rows, d, family


def _check_special_rows(family, rows, y, b):
    if family != "special":
        return
    zero, _ = kr.ln_special_rows(rows)
    for r in zero:
        # (0 - 0) * rstd * w + b, rounded once: b bit for bit
        assert torch.equal(y[r], b), f"zero row {r}: y != b"


@pytest.mark.parametrize("rows,d,family", list(_ln_cases()))
def test_layernorm_fwd_bwd_vs_fp64(rows, d, family):
    inp = kr.ln_make_inputs(family, rows, d, kr.LN_SEED, _dev())
    x, _, w, b, dy, _ = inp
    y, mean, rstd = EXT.layernorm_fwd(x, w, b, EPS)
    dx, dw, db = EXT.layernorm_bwd(dy, x, w, mean, rstd)
    got = {"y": y, "mean": mean, "rstd": rstd, "dx": dx}
    name = f"ln/{family}/{rows}x{d}"
    _finite(got, name)
    assert dw.shape == w.shape and db.shape == w.shape
    _, ref, _ = kr.ln_check(got, inp, "plain", name)
    kr.ln_assert_family(family, ref["sum"], rows)
    _check_special_rows(family, rows, y, b)


@pytest.mark.parametrize("rows,d,family", list(_ln_cases()))
def test_layernorm_add_fwd_bwd_vs_fp64(rows, d, family):
    inp = kr.ln_make_inputs(family, rows, d, kr.LN_SEED + 1, _dev())
    x, res, w, b, dy, dsum = inp
    s, y, mean, rstd = EXT.layernorm_add_fwd(x, res, w, b, EPS)
    dx1, dx2, dw, db = EXT.layernorm_add_bwd(dy, dsum, s, w, mean, rstd)
    got = {"sum": s, "y": y, "mean": mean, "rstd": rstd, "dx": dx1}
    name = f"ln_add/{family}/{rows}x{d}"
    _finite(got, name)
    # the gradients of x and res: the same values in distinct buffers
    assert torch.equal(dx1, dx2) and dx1.data_ptr() != dx2.data_ptr()
    _, ref, model = kr.ln_check(got, inp, "add", name)
    kr.ln_assert_family(family, model["sum"].double(), rows)
    _check_special_rows(family, rows, y, b)


def test_layer_norm_ops_path_vs_fp64():
    """Once through ops.layer_norm / ops.fused_add_layer_norm and autograd
    ([B, T, D] input, VPT 2 with one thread in the second slot)."""
    from vit_10b_fsdp_example_amd.ops import fused_add_layer_norm, layer_norm

    rows, d = 6, 2056
    inp = kr.ln_make_inputs("row_scale", rows, d, 5, _dev())
    x, res, w, b, dy, dsum = inp
    xr = x.view(2, 3, d).clone().requires_grad_(True)
    y = layer_norm(xr, w, b, EPS)
    y.backward(dy.view(2, 3, d))
    kr.ln_check({"y": y.detach().view(rows, d), "dx": xr.grad.view(rows, d)},
                inp, "plain", "ops.layer_norm")

    xr = x.view(2, 3, d).clone().requires_grad_(True)
    rr = res.view(2, 3, d).clone().requires_grad_(True)
    s, y = fused_add_layer_norm(xr, rr, w, b, EPS)
    torch.autograd.backward([s, y], [dsum.view(2, 3, d), dy.view(2, 3, d)])
    assert torch.equal(xr.grad, rr.grad)
    kr.ln_check({"sum": s.detach().view(rows, d),
                 "y": y.detach().view(rows, d), "dx": xr.grad.view(rows, d)},
                inp, "add", "ops.fused_add_layer_norm")


def test_layernorm_empty_batch_returns_empty_outputs():
    d = 64
    x = torch.empty(0, d, device=_dev(), dtype=torch.bfloat16)
    w = torch.ones(d, device=_dev(), dtype=torch.bfloat16)
    b = torch.zeros(d, device=_dev(), dtype=torch.bfloat16)
    y, mean, rstd = EXT.layernorm_fwd(x, w, b, EPS)
    assert y.shape == (0, d) and mean.shape == (0,) and rstd.shape == (0,)
    assert mean.dtype == torch.float32 and y.dtype == torch.bfloat16
    s, y, mean, rstd = EXT.layernorm_add_fwd(x, x.clone(), w, b, EPS)
    assert s.shape == (0, d) and y.shape == (0, d) and mean.shape == (0,)
    dx, dw, db = EXT.layernorm_bwd(x, x, w, mean, rstd)
    assert dx.shape == (0, d) and not bool(dw.any()) and not bool(db.any())
    dx1, dx2, dw, db = EXT.layernorm_add_bwd(x, x, x, w, mean, rstd)
    assert dx1.shape == (0, d) and not bool(dw.any())
    torch.cuda.synchronize()


def _bad_variants(t, what):
    """(label, tensor) that the entry points must refuse in place of t:
    wrong dtype, not contiguous, wrong size, wrong device."""
    other = torch.float32 if t.dtype != torch.float32 else torch.float16
    if t.dtype == torch.int64:
        other = torch.int32
    yield f"{what} dtype", t.to(other)
    if t.numel() > 1:
        nc = torch.stack([t, t], -1)[..., 0]
        assert not nc.is_contiguous() and nc.shape == t.shape
        yield f"{what} non-contiguous", nc
    yield f"{what} size", torch.cat([t.reshape(-1), t.reshape(-1)[:8]]) \
        if t.dim() <= 1 else torch.cat([t, t[:1]])
    yield f"{what} device", t.cpu()


def _ln_good():
    rows, d = 5, 64
    x, res, w, b, dy, dsum = kr.ln_make_inputs("randn", rows, d, 2, _dev())
    y, mean, rstd = EXT.layernorm_fwd(x, w, b, EPS)
    s, _, mean_a, rstd_a = EXT.layernorm_add_fwd(x, res, w, b, EPS)
    return {
        "layernorm_fwd": (["x", "weight", "bias"], [x, w, b, EPS]),
        "layernorm_add_fwd": (["x", "res", "weight", "bias"],
                              [x, res, w, b, EPS]),
        "layernorm_bwd": (["dy", "x", "weight", "mean", "rstd"],
                          [dy, x, w, mean, rstd]),
        "layernorm_add_bwd": (["dy", "dsum", "sum", "weight", "mean", "rstd"],
                              [dy, dsum, s, w, mean_a, rstd_a]),
    }


@pytest.mark.parametrize("fn", ["layernorm_fwd", "layernorm_add_fwd",
                                "layernorm_bwd", "layernorm_add_bwd"])
def test_layernorm_refuses_bad_operands(fn):
    names, args = _ln_good()[fn]
    getattr(EXT, fn)(*args)  # the good call passes
    n_refused = 0
    for i, what in enumerate(names):
        for label, bad in _bad_variants(args[i], what):
            if fn == "layernorm_fwd" and label == "x size":
                continue  # x alone fixes the shape there: one more row is fine
            call = list(args)
            call[i] = bad
            with pytest.raises(RuntimeError, match=fn):
                getattr(EXT, fn)(*call)
            n_refused += 1
    assert n_refused == 4 * len(names) - (fn == "layernorm_fwd")
    # D that is no multiple of 8
    x = torch.zeros(3, 12, device=_dev(), dtype=torch.bfloat16)
    v = torch.zeros(12, device=_dev(), dtype=torch.bfloat16)
    st = torch.zeros(3, device=_dev())
    bad_d = {"layernorm_fwd": (x, v, v, EPS),
             "layernorm_add_fwd": (x, x, v, v, EPS),
             "layernorm_bwd": (x, x, v, st, st),
             "layernorm_add_bwd": (x, x, x, v, st, st)}[fn]
    with pytest.raises(RuntimeError, match="multiple of 8"):
        getattr(EXT, fn)(*bad_d)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------
# cross-entropy
# --------------------------------------------------------------------------

@pytest.mark.parametrize("family", kr.CE_FAMILIES)
@pytest.mark.parametrize("n", kr.CE_ROWS)
@pytest.mark.parametrize("c", kr.CE_CLASSES)
def test_cross_entropy_vs_fp64(c, n, family):
    logits, target = kr.ce_make_inputs(family, n, c, n, _dev())
    assert int(target.min()) >= 0 and int(target.max()) < c
    loss, lse = EXT.cross_entropy_fwd(logits, target)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    for dloss in kr.CE_DLOSS:
        dl = torch.tensor(dloss, device=_dev())
        dlogits = EXT.cross_entropy_bwd(dl, logits, target, lse)
        assert dlogits.dtype == torch.bfloat16
        got = {"lse": lse, "loss": loss, "dlogits": dlogits}
        name = f"ce/{family}/{n}x{c}/dloss{dloss}"
        _finite(got, name)
        _, ref, _ = kr.ce_check(got, logits, target, dloss, name)
    kr.ce_assert_family(family, logits, target, ref)


def test_cross_entropy_ops_path_non_contiguous_logits():
    """ops.cross_entropy on a strided view (every second column of a
    wider tensor), with a scaled loss so that dloss != 1."""
    from vit_10b_fsdp_example_amd.ops import cross_entropy

    n, c = 3, 1001
    logits, target = kr.ce_make_inputs("randn", n, c, 4, _dev())
    wide = torch.zeros(n, 2 * c, device=_dev(), dtype=torch.bfloat16)
    wide[:, ::2] = logits
    wide.requires_grad_(True)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    loss = cross_entropy(view, target)
    (loss * 0.37).backward()
    grad = wide.grad[:, ::2]
    assert not bool(wide.grad[:, 1::2].any())
    fwd = EXT.cross_entropy_fwd(logits, target)
    kr.ce_check({"lse": fwd[1], "loss": loss.detach(), "dlogits": grad},
                logits, target, 0.37, "ops.cross_entropy")


def test_cross_entropy_refuses_empty_batch():
    logits = torch.empty(0, 10, device=_dev(), dtype=torch.bfloat16)
    target = torch.empty(0, device=_dev(), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="non-empty"):
        EXT.cross_entropy_fwd(logits, target)
    with pytest.raises(RuntimeError, match="non-empty"):
        EXT.cross_entropy_bwd(torch.ones((), device=_dev()), logits, target,
                              torch.empty(0, device=_dev()))
    with pytest.raises(RuntimeError, match="non-empty"):
        EXT.cross_entropy_fwd(
            torch.empty(4, 0, device=_dev(), dtype=torch.bfloat16),
            torch.zeros(4, device=_dev(), dtype=torch.int64))
    torch.cuda.synchronize()


@pytest.mark.parametrize("fn", ["cross_entropy_fwd", "cross_entropy_bwd"])
def test_cross_entropy_refuses_bad_operands(fn):
    n, c = 5, 24
    logits, target = kr.ce_make_inputs("randn", n, c, 1, _dev())
    loss, lse = EXT.cross_entropy_fwd(logits, target)
    dl = torch.ones((), device=_dev())
    if fn == "cross_entropy_fwd":
        names, args = ["logits", "target"], [logits, target]
    else:
        names, args = (["dloss", "logits", "target", "lse"],
                       [dl, logits, target, lse])
    getattr(EXT, fn)(*args)
    n_refused = 0
    for i, what in enumerate(names):
        for label, bad in _bad_variants(args[i], what):
            call = list(args)
            call[i] = bad
            with pytest.raises(RuntimeError, match=fn):
                getattr(EXT, fn)(*call)
            n_refused += 1
    # dloss has one element: no non-contiguous form of it exists
    assert n_refused == 4 * len(names) - (fn == "cross_entropy_bwd")
    with pytest.raises(RuntimeError, match=fn):  # 1-D logits
        getattr(EXT, fn)(*[a.reshape(-1) if a is logits else a for a in args])
    torch.cuda.synchronize()
