"""Reference, rounding model and checker for the flash-attention kernels
(csrc/fmha.hip).  Plain torch, importable without a GPU.

Three things are compared per case:

* ``attention_fp64``: o, lse, dq, dk, dv in float64 from the bf16 inputs.
  This is the truth.
* ``attention_rounding_model``: the same operation in fp32 with a bf16
  rounding at every point where the kernels round, and nowhere else.  Its
  distance from the fp64 result is what a *correct* kernel must be off by.
* the kernel's output.

``check_against_model`` asserts, for each of o, dq, dk, dv and for two
error metrics, ``E(kernel) <= MARGIN * E(model)``.  The bound therefore
follows the arithmetic: it is tight (a few 1e-3) where bf16 rounding is
all that separates the kernel from fp64, and loosens by itself where the
operation is ill-conditioned (the ``offset`` family's cancellation in dq
and dk), which no fixed tolerance can do.

Rounding points of the kernels (read from csrc/fmha.hip), reproduced by
the model:

forward (``fmha_fwd_kernel``)
  1. scores: fp32 MFMA accumulation of exact bf16 products, then
     ``* scale`` in fp32 -- no bf16 rounding.
  2. ``P = exp(s - rowmax)`` in fp32; the row sum ``l`` accumulates the
     UNROUNDED, UNMASKED P.
  3. with dropout P is masked and multiplied by ``1/(1-p)`` (fp32), then
     packed to bf16 (``pack_bf16x2``) as the A operand of ``P @ V``.  [bf16]
  4. ``o = acc / l`` stored as bf16 (epilogue ``f32_to_bf16``).      [bf16]
  5. ``lse = m + log(l)`` stored in fp32.

backward (``fmha_rowdot_kernel``, ``fmha_bwd_dq_kernel``,
``fmha_bwd_dkv_kernel``)
  6. ``Delta = rowsum(dO * o)`` in fp32 from the bf16 o of step 4.
  7. ``P = exp(s * scale - lse)`` in fp32, s recomputed as in step 1.
  8. ``dP = dO @ V^T`` in fp32, masked and scaled by ``1/(1-p)`` with
     dropout.
  9. ``dS = scale * P * (dP - Delta)`` rounded to bf16 before BOTH
     ``dS @ K`` (dq kernel, ``pack_bf16x2``) and ``dS^T @ Q`` (dkv
     kernel, the ``dst_tile`` store).                                [bf16]
  10. ``P^T`` (masked and scaled with dropout) rounded to bf16 before
      ``P^T @ dO`` (the ``pt_tile`` store).                          [bf16]
  11. dq, dk, dv stored as bf16 (epilogues).                         [bf16]

The kernels round P relative to the RUNNING row max of the key tiles seen
so far and rescale the accumulator by ``alpha`` in fp32; the model rounds
relative to the final row max.  bf16 rounding is scale-invariant in
relative terms, so both give the same error statistics.

All bf16 conversions are round-to-nearest-even on both sides
(``__float2bfloat16`` / ``Tensor.to(torch.bfloat16)``).
"""

import math

import numpy as np
import torch

MARGIN = 2.0
TENSORS = ("o", "dq", "dk", "dv")
FAMILIES = ("randn", "peaked", "rising", "offset")
HEAD_DIMS = tuple(range(16, 193, 16))

_U = 2.0 ** -24  # fp32 unit roundoff

# Allowance for the fast exp/log intrinsics (``__expf``, ``__logf``) in
# the forward's lse.  The ISA and programming guides give no accuracy
# figure for them, so it is measured: the worst |lse(kernel) - lse(fp32
# rounding model)| over every case of tests/test_gpu_fmha_numerics.py on
# an MI355X, normalised by (1 + |lse|) because both sides store an fp32
# value of that magnitude, was 6.3e-7 (family `rising`, T = 129,
# D = 192, |lse| ~ 170; 1.5e-7 to 3e-7 for `randn` and `peaked`).  The
# figure also contains the two sides' different fp32 summation orders,
# so it over-states the intrinsics; the constant is 4x it all the same.
# check_lse prints the figure for every case ("vs model/(1+|lse|)").
LSE_INTRINSIC_ALLOWANCE = 4 * 6.3e-7


def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def drop_rscale(p_drop):
    """1/(1-p) exactly as the host code computes it (fp32)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p_drop)))


def make_inputs(family, B, H, T, D, seed, device="cpu"):
    """bf16 q, k, v, do of shape [B, H, T, D].  Values are drawn on the
    CPU so that a (family, shape, seed) names the same numbers on every
    device."""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    shape = (B, H, T, D)
    if family == "randn":
        q, k = rn(*shape), rn(*shape)
    elif family == "peaked":
        q, k = 4.0 * rn(*shape), rn(*shape)
    elif family == "rising":
        u = rn(B, H, 1, D)
        u = u / u.norm(dim=-1, keepdim=True)
        ramp = torch.arange(T, dtype=torch.float32) / max(T - 1, 1)
        k = ramp.view(1, 1, T, 1) * math.sqrt(D) * u + 0.3 * rn(*shape)
        q = 12.0 * math.sqrt(D) * u + rn(*shape)
    elif family == "offset":
        q, k = 3.0 + 0.25 * rn(*shape), 3.0 + 0.25 * rn(*shape)
    else:
        raise ValueError(family)
    v, do = rn(*shape), rn(*shape)
    return tuple(t.to(torch.bfloat16).to(device) for t in (q, k, v, do))


def keep_mask(seed, p_drop, B, H, T, device="cpu"):
    """The kernels' dropout keep mask [B, H, T, T] (bool), bit-exact."""
    from vit_10b_fsdp_example_amd.ops.attention import dropout_mask_reference

    rows = torch.arange(B * H * T)
    # the host code turns p into a threshold from its fp32 value
    keep = dropout_mask_reference(seed, rows, torch.arange(T),
                                  float(np.float32(p_drop)))
    return keep.view(B, H, T, T).to(device)


def attention_fp64(q, k, v, do, scale, keep=None, p_drop=0.0):
    """softmax(q k^T scale) v and its gradients in float64.

    With a keep mask: the softmax normaliser is unmasked, P*keep/(1-p)
    goes into PV, and the gradient goes back through the mask.  Returns a
    dict with o, lse, dq, dk, dv and the intermediate s (scaled scores)
    and p (unmasked probabilities) for the family stress assertions."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    s = (q @ k.transpose(-2, -1)) * scale
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    if keep is not None:
        m = keep.double() / (1.0 - p_drop)
        pd = p * m
    else:
        m, pd = None, p
    o = pd @ v
    dv = pd.transpose(-2, -1) @ do
    dp = do @ v.transpose(-2, -1)
    if m is not None:
        dp = dp * m
    delta = (dp * p).sum(-1, keepdim=True)  # == rowsum(do * o)
    ds = p * (dp - delta)
    dq = (ds @ k) * scale
    dk = (ds.transpose(-2, -1) @ q) * scale
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv, "s": s, "p": p}


def attention_rounding_model(q, k, v, do, scale, keep=None, p_drop=0.0):
    """fp32 attention with bf16 roundings exactly at the kernels' rounding
    points (module docstring, steps 1-11)."""
    q, k, v, do = (t.float() for t in (q, k, v, do))
    scale = float(np.float32(scale))
    if keep is not None:
        m = keep.float() * drop_rscale(p_drop)
    else:
        m = None
    # forward
    s = (q @ k.transpose(-2, -1)) * scale                       # 1
    smax = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - smax)                                     # 2
    l = e.sum(-1, keepdim=True)
    pd = e if m is None else e * m                              # 3
    o = _bf((_bf(pd) @ v) / l)                                  # 3, 4
    lse = smax + torch.log(l)                                   # 5
    # backward
    delta = (do * o).sum(-1, keepdim=True)                      # 6
    p = torch.exp(s - lse)                                      # 7
    dp = do @ v.transpose(-2, -1)                               # 8
    if m is not None:
        dp = dp * m
    ds = _bf(scale * p * (dp - delta))                          # 9
    dq = _bf(ds @ k)                                            # 11
    dk = _bf(ds.transpose(-2, -1) @ q)
    pt = _bf(p if m is None else p * m)                         # 10
    dv = _bf(pt.transpose(-2, -1) @ do)
    return {"o": o, "lse": lse.squeeze(-1), "dq": dq, "dk": dk, "dv": dv}


def error_metrics(x, ref):
    """(E_max, E_rms) of x against the fp64 ref:
    max|x-ref|/max|ref| and rms(x-ref)/rms(ref).

    A ref that is identically zero (dq and dk at T = 1, where P = 1 and
    dS = 0 exactly) has no scale to divide by; the absolute errors are
    returned then, so that kernel and model are still compared like with
    like."""
    ref = ref.double()
    d = x.double() - ref
    e_max, e_rms = d.abs().max().item(), d.pow(2).mean().sqrt().item()
    r_max, r_rms = ref.abs().max().item(), ref.pow(2).mean().sqrt().item()
    if r_max == 0.0:
        return e_max, e_rms
    return e_max / r_max, e_rms / r_rms


def _ratio(a, b):
    if b == 0.0:
        return 1.0 if a == 0.0 else float("inf")
    return a / b


def compare_with_model(got, model, ref64, name="", floors=None):
    """Per tensor: metrics of kernel and model, their ratios, pass/fail.
    Prints one line per tensor and returns
    {tensor: (ratio_max, ratio_rms, ok)}.

    ``floors`` optionally maps a tensor name to an absolute error that is
    accepted regardless of the model (only used where the fp64 result is
    exactly zero and both errors are pure fp32 summation-order noise)."""
    out = {}
    for t in TENSORS:
        if t not in got:
            continue
        gm, gr = error_metrics(got[t], ref64[t])
        mm, mr = error_metrics(model[t], ref64[t])
        floor = (floors or {}).get(t, 0.0)
        ok = (gm <= max(MARGIN * mm, floor)) and (gr <= max(MARGIN * mr, floor))
        rm, rr = _ratio(gm, mm), _ratio(gr, mr)
        print(f"fmha-check {name} {t:>2}: E_max kernel {gm:.3e} model "
              f"{mm:.3e} ratio {rm:.2f} | E_rms kernel {gr:.3e} model "
              f"{mr:.3e} ratio {rr:.2f} | {'ok' if ok else 'FAIL'}")
        out[t] = (rm, rr, ok)
    return out


def check_against_model(got, model, ref64, name="", floors=None):
    """Assert E(kernel) <= MARGIN * E(model), both metrics, every tensor
    of o/dq/dk/dv present in ``got``."""
    res = compare_with_model(got, model, ref64, name, floors)
    bad = {t: (round(rm, 3), round(rr, 3))
           for t, (rm, rr, ok) in res.items() if not ok}
    assert not bad, (
        f"{name}: error exceeds {MARGIN} x the rounding model's "
        f"(tensor: (max ratio, rms ratio)): {bad}")
    return res


def lse_bound(q, k, scale, ref64):
    """Per-row absolute bound [B, H, T] on |lse(kernel) - lse(fp64)|.

    logsumexp is 1-Lipschitz in the sup norm of the scores, so a
    per-score error bound carries over.  A score is a fp32 accumulation
    of DP exact bf16 products (DP = D padded to a multiple of 32):
    worst case DP * 2^-24 * scale * max_j sum_d |q_d k_jd|.  The
    ``* scale`` and ``s - m`` roundings add 2 * 2^-24 * max_j |s_j|; the
    row sum of T fp32 terms adds at most T * 2^-24 relative to l, i.e.
    absolute to log(l); m + log(l) is rounded to fp32 once
    (2^-24 * |lse|).  On top comes LSE_INTRINSIC_ALLOWANCE * (1 + |lse|)
    for ``__expf`` / ``__logf``."""
    D, T = q.shape[-1], q.shape[-2]
    dp = ((D + 31) // 32) * 32
    absdot = q.double().abs() @ k.double().abs().transpose(-2, -1)
    acc = dp * _U * scale * absdot.max(dim=-1).values
    s_abs = ref64["s"].abs().max(dim=-1).values
    lse_abs = ref64["lse"].abs()
    return (acc + 2 * _U * s_abs + T * _U + _U * lse_abs
            + LSE_INTRINSIC_ALLOWANCE * (1.0 + lse_abs))


def check_lse(lse, q, k, scale, ref64, name="", model=None):
    bound = lse_bound(q, k, scale, ref64)
    err = (lse.double() - ref64["lse"]).abs()
    worst = (err / bound).max().item()
    vs_model = ""
    if model is not None:
        # the figure LSE_INTRINSIC_ALLOWANCE was measured from
        d = (lse.double() - model["lse"].double()).abs()
        vs_model = (", vs model/(1+|lse|) "
                    f"{(d / (1 + ref64['lse'].abs())).max().item():.3e}")
    print(f"fmha-check {name} lse: max err {err.max().item():.3e}, "
          f"min bound {bound.min().item():.3e}, worst err/bound {worst:.3f}"
          f"{vs_model}")
    assert lse.dtype == torch.float32
    assert bool((err <= bound).all()), (name, err.max().item(), worst)


def check_kernel_outputs(q, k, v, do, scale, got, name="", keep=None,
                         p_drop=0.0, floors=None):
    """fp64 reference and rounding model on the inputs' device, then the
    lse bound (if ``got`` has an lse) and the model-relative check of
    whichever of o/dq/dk/dv ``got`` holds, all [B, H, T, D]."""
    ref64 = attention_fp64(q, k, v, do, scale, keep, p_drop)
    model = attention_rounding_model(q, k, v, do, scale, keep, p_drop)
    if "lse" in got:
        check_lse(got["lse"], q, k, scale, ref64, name, model)
    res = check_against_model(got, model, ref64, name, floors)
    return ref64, model, res


def old_tolerance_passes(got, ref64):
    """The fixed tolerances the suite used before (rtol=0.1, atol=0.06
    for gradients; 0.05 / 0.03 for o).  Reported, never asserted: it is
    the record of what those tolerances let through."""
    res = {}
    for t in TENSORS:
        rtol, atol = (0.05, 0.03) if t == "o" else (0.1, 0.06)
        ref = ref64[t].double()
        res[t] = bool(((got[t].double() - ref).abs()
                       <= atol + rtol * ref.abs()).all())
    return res


def family_stats(ref64):
    """What a family claims to stress, from the fp64 reference."""
    s, p = ref64["s"], ref64["p"]
    T = s.shape[-1]
    stats = {
        "smax": s.max().item(),
        "smin": s.min().item(),
        "pmax_mean": p.max(dim=-1).values.mean().item(),
        "pmax_max": p.max().item(),
    }
    # fraction of (row, key tile > 0) pairs whose 32-key tile raises the
    # running max, i.e. where the online softmax rescales with alpha < 1.
    # A ragged last tile of fewer than 16 keys is left out: its handful
    # of keys need not beat the noise of the 32 before them.
    n_tiles = T // 32 + (1 if T % 32 >= 16 else 0)
    if n_tiles > 1:
        sp = s[..., :n_tiles * 32]
        pad = n_tiles * 32 - sp.shape[-1]
        sp = torch.nn.functional.pad(sp, (0, pad), value=float("-inf"))
        tile_max = sp.view(*s.shape[:-1], n_tiles, 32).max(-1).values
        run = torch.cummax(tile_max, dim=-1).values
        stats["rescale_frac"] = (
            (tile_max[..., 1:] > run[..., :-1]).double().mean().item())
    return stats


def assert_family_stress(family, ref64, D, T):
    """A family that stops stressing what it claims fails loudly.  The
    bounds follow from the constructions in make_inputs (they describe
    the inputs, not any kernel)."""
    st = family_stats(ref64)
    print(f"fmha-family {family} D={D} T={T}: " +
          ", ".join(f"{k}={v:.3g}" for k, v in st.items()))
    if family == "peaked":
        # logits are N(0, 16): extremes beyond +-8 at T >= 33 keys per
        # row and thousands of rows, and rows dominated by one key
        assert st["smax"] > 8 and st["smin"] < -8, st
        assert st["pmax_mean"] > 0.25 and st["pmax_max"] > 0.99, st
    elif family == "rising":
        # the last key's logit is 12 sqrt(D) + noise of std ~3.6
        assert st["smax"] > 11 * math.sqrt(D), st
        if D >= 64:
            # fp32 exp overflows above 88.7: an un-shifted exp is inf
            assert st["smax"] > 88.7, st
        assert st["pmax_mean"] > 0.25, st
        if "rescale_frac" in st:
            assert st["rescale_frac"] > 0.9, st
    elif family == "offset":
        # common logit 9 sqrt(D) with a spread of std ~1.06 at every D
        # (sum of D terms (3+a)(3+b), a, b ~ 0.25 N(0,1), times D^-1/2);
        # near-uniform softmax on top of it
        assert st["smin"] > 9 * math.sqrt(D) - 6, st
        if D >= 128:
            assert st["smin"] > 88.7, st
        assert st["pmax_mean"] < 8.0 / T + 0.05, st
    return st
