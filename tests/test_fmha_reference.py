"""CPU tests of the flash-attention checker (tests/fmha_reference.py):
the fp64 reference is sound, the rounding model passes its own check,
the input families stress what they claim, and ``check_against_model``
rejects deliberately wrong attention variants -- most of which the fixed
tolerances the suite used before let through (printed, not asserted)."""

import math

import pytest
import torch

from tests.fmha_reference import (
    FAMILIES, MARGIN, TENSORS, _bf, assert_family_stress, attention_fp64,
    attention_rounding_model, check_against_model, compare_with_model,
    error_metrics, keep_mask, lse_bound, make_inputs, old_tolerance_passes,
)

B, H, T, D = 1, 2, 97, 48
SCALE = D ** -0.5

_CASES = {}


def _case(family):
    """Inputs, fp64 reference and rounding model of one family, computed
    once and shared (read-only) by the tests below."""
    if family not in _CASES:
        inp = make_inputs(family, B, H, T, D, seed=11)
        _CASES[family] = (inp, attention_fp64(*inp, SCALE),
                          attention_rounding_model(*inp, SCALE))
    return _CASES[family]


def tiled_model(q, k, v, do, scale, ref64, defect=None):
    """The rounding model restructured the way the kernels work -- an
    online softmax over 32-key tiles, P rounded relative to the running
    max, lse-based recompute in the backward -- with one optional
    defect.  Without a defect it must pass the check like the model.
    ``skip_alpha`` omits the rescale on the last full key tile: earlier
    tiles' omissions are themselves rescaled away by later alphas."""
    q, k, v, do = (t.float() for t in (q, k, v, do))
    n_t, d = q.shape[-2], q.shape[-1]
    v_read = v.roll(-1, dims=1) if defect == "swap_heads_v" else v
    if defect == "d_tail":
        s = (q[..., :d - 16] @ k[..., :d - 16].transpose(-2, -1)) * scale
    else:
        s = (q @ k.transpose(-2, -1)) * scale
    n_keys = n_t
    if defect == "drop_last_tile":
        n_keys = ((n_t - 1) // 32) * 32
    elif defect == "drop_last_key":
        n_keys = n_t - 1
    assert n_keys >= 1
    s = s.masked_fill(torch.arange(n_t) >= n_keys, float("-inf"))

    m = torch.full(s.shape[:-1] + (1,), float("-inf"))
    l = torch.zeros_like(m)
    acc = torch.zeros_like(q)
    for ti, k0 in enumerate(range(0, n_t, 32)):
        st = s[..., k0:k0 + 32]
        m_new = torch.maximum(m, st.max(-1, keepdim=True).values)
        alpha = torch.exp(m - m_new)
        e = torch.exp(st - m_new)
        l = l * alpha + e.sum(-1, keepdim=True)
        if not (defect == "skip_alpha" and ti == n_t // 32 - 1):
            acc = acc * alpha
        acc = acc + _bf(e) @ v_read[..., k0:k0 + 32, :]
        m = m_new
    o = _bf(acc / l)
    lse = m + torch.log(l)

    if defect == "delta_1pct":
        delta = (1.01 * (do.double() * ref64["o"]).sum(-1, keepdim=True)
                 ).float()
    else:
        delta = (do * o).sum(-1, keepdim=True)
    p = torch.exp(s - lse)
    dp = do @ v_read.transpose(-2, -1)
    ds = _bf((1.0 if defect == "ds_noscale" else scale) * p * (dp - delta))
    return {"o": o, "lse": lse.squeeze(-1), "dq": _bf(ds @ k),
            "dk": _bf(ds.transpose(-2, -1) @ q),
            "dv": _bf(_bf(p).transpose(-2, -1) @ do)}


# defect -> families in which it is active.  Two are not active
# everywhere:
#  * skip_alpha: bites on rows whose running max rises in the tile that
#    skips the rescale.  `rising` does that on every row and tile; with
#    randn / peaked scores about a quarter of the rows do, which is
#    enough.  In `offset` the score varies over keys by a term common to
#    all rows, so every row has the same arg-max key, and it need not
#    lie in that tile (at this seed it does not).
#  * delta_1pct: with randn scores Delta/dP ~ T_eff^-1/2 ~ 0.1, so 1 % of
#    Delta is ~1e-3 of dS, below the 2^-9 bf16 rounding of dS itself
#    (measured RMS ratio 1.4: visible, under the margin).  The other
#    families make dP - Delta cancel (peaked, rising) or dq cancel over
#    keys (offset), which exposes it.
DEFECTS = {
    "drop_last_tile": FAMILIES,
    "drop_last_key": FAMILIES,
    "skip_alpha": ("randn", "peaked", "rising"),
    "delta_1pct": ("peaked", "rising", "offset"),
    "ds_noscale": FAMILIES,
    "d_tail": FAMILIES,
    "swap_heads_v": FAMILIES,
}


@pytest.mark.parametrize("family", FAMILIES)
def test_model_passes_own_check_with_ratio_one(family):
    inp, ref, model = _case(family)
    res = check_against_model(model, model, ref, f"model/{family}")
    assert all(rm == 1.0 and rr == 1.0 for rm, rr, _ in res.values())
    # sanity of the scheme: the model's own error is a few bf16 ulps
    # (2^-9 = 2e-3 per rounding) except where the family makes dq / dk
    # cancel
    for t in ("o", "dv"):
        e_max, e_rms = error_metrics(model[t], ref[t])
        assert e_rms < 4 * 2.0 ** -9 and e_max < 4 * 2.0 ** -9, (t, e_max)


@pytest.mark.parametrize("family", FAMILIES)
def test_tiled_model_without_defect_passes(family):
    """Online softmax over tiles differs from the model only in where
    the running max sits when P is rounded: same error, ratio near 1."""
    inp, ref, model = _case(family)
    got = tiled_model(*inp, SCALE, ref)
    res = check_against_model(got, model, ref, f"tiled/{family}")
    assert all(rr < 1.25 for _, rr, _ in res.values()), res
    err = (got["lse"].double() - ref["lse"]).abs()
    assert bool((err <= lse_bound(inp[0], inp[1], SCALE, ref)).all())


def test_fp64_gradients_equal_autograd():
    q, k, v, do = (t.double() for t in _case("randn")[0])
    ref = _case("randn")[1]
    for t in (q, k, v):
        t.requires_grad_(True)
    s = (q @ k.transpose(-2, -1)) * SCALE
    o = torch.softmax(s, dim=-1) @ v
    o.backward(do)
    for got, want in ((ref["o"], o.detach()), (ref["dq"], q.grad),
                      (ref["dk"], k.grad), (ref["dv"], v.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * float(
            want.abs().max())
    want_lse = torch.logsumexp(s.detach(), dim=-1)
    assert float((ref["lse"] - want_lse).abs().max()) < 1e-12


def test_fp64_dropout_equals_explicit_masked_composition():
    p_drop, seed = 0.3, 4242
    q, k, v, do = (t.double() for t in _case("randn")[0])
    keep = keep_mask(seed, p_drop, B, H, T)
    assert abs(keep.double().mean().item() - (1 - p_drop)) < 0.02
    ref = attention_fp64(q, k, v, do, SCALE, keep, p_drop)
    for t in (q, k, v):
        t.requires_grad_(True)
    probs = torch.softmax((q @ k.transpose(-2, -1)) * SCALE, dim=-1)
    o = (probs * keep / (1 - p_drop)) @ v
    o.backward(do)
    for got, want in ((ref["o"], o.detach()), (ref["dq"], q.grad),
                      (ref["dk"], k.grad), (ref["dv"], v.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * float(
            want.abs().max())
    # and the dropout rounding model passes its own scheme's sanity
    model = attention_rounding_model(*_case("randn")[0], SCALE, keep, p_drop)
    for t in TENSORS:
        assert error_metrics(model[t], ref[t])[1] < 4 * 2.0 ** -9, t


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_defect_is_rejected(defect):
    """Every defect is rejected for at least one tensor in every family
    where it is active.  Which of them the old fixed tolerances pass is
    printed: it is the record of the gap."""
    for family in DEFECTS[defect]:
        inp, ref, model = _case(family)
        got = tiled_model(*inp, SCALE, ref, defect)
        res = compare_with_model(got, model, ref, f"{defect}/{family}")
        old = old_tolerance_passes(got, ref)
        rejected = [t for t, (_, _, ok) in res.items() if not ok]
        print(f"defect {defect:>14} / {family:<6}: new check rejects "
              f"{rejected or 'NOTHING'}; old tolerances pass "
              f"{[t for t in TENSORS if old[t]] or 'nothing'}"
              f"{' (ALL: defect invisible)' if all(old.values()) else ''}")
        assert rejected, (defect, family, res)
        with pytest.raises(AssertionError):
            check_against_model(got, model, ref, f"{defect}/{family}")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("t_d", [(33, 64), (256, 160), (80, 64), (129, 16),
                                 (129, 192), (200, 112)])
def test_family_stress_at_gpu_shapes(family, t_d):
    """The smallest and largest T (and D) at which each family runs on
    the GPU, with the GPU tests' B = 2, H = 3."""
    t, d = t_d
    inp = make_inputs(family, 2, 3, t, d, seed=0)
    ref = attention_fp64(*inp, d ** -0.5)
    assert_family_stress(family, ref, d, t)
    if family == "offset":
        # what the family is for: the model's own dq error is an order
        # of magnitude above plain bf16 rounding (cancellation)
        model = attention_rounding_model(*inp, d ** -0.5)
        assert error_metrics(model["dq"], ref["dq"])[1] > 1e-2


def test_margin_and_metric_definitions():
    assert MARGIN == 2.0
    ref = torch.tensor([3.0, -4.0], dtype=torch.float64)
    x = torch.tensor([3.5, -4.0])
    e_max, e_rms = error_metrics(x, ref)
    assert e_max == pytest.approx(0.5 / 4.0)
    assert e_rms == pytest.approx(math.sqrt(0.125) / math.sqrt(12.5))


def test_attention_fp16_predicate_routes_to_math(monkeypatch):
    """ops.attention must not send fp16 to the bf16-only kernel: even
    where the HIP path is available, fp16 takes math_attention."""
    import importlib

    # ops/__init__ re-exports the function under the module's name
    attn_mod = importlib.import_module(
        "vit_10b_fsdp_example_amd.ops.attention")

    class _NoKernel:
        def __getattr__(self, name):
            if name in ("fmha_fwd", "fmha_bwd"):
                return lambda *a, **k: pytest.fail("fp16 reached the kernel")
            raise AttributeError(name)

    monkeypatch.setattr(attn_mod, "use_hip", lambda *ts: True)
    monkeypatch.setattr(attn_mod, "ext", lambda: _NoKernel())
    torch.manual_seed(0)
    q, k, v = (torch.randn(1, 2, 8, 16).to(torch.float16) for _ in range(3))
    out = attn_mod.attention(q, k, v)
    assert out.dtype == torch.float16
    assert torch.equal(out, attn_mod.math_attention(q, k, v))
    assert attn_mod._kernel_dtype(torch.bfloat16)
    assert not attn_mod._kernel_dtype(torch.float16)
    assert not attn_mod._kernel_dtype(torch.float32)
