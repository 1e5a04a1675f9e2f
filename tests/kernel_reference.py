"""References, rounding models, bounds and wrong variants for the row-wise
and optimizer kernels: csrc/layernorm.hip, csrc/cross_entropy.hip and
csrc/adamw.hip.  Plain torch, importable without a GPU; the counterpart
of tests/fmha_reference.py.

For every operation three things exist side by side:

* an fp64 reference computed from the same bf16 / fp32 inputs: the truth;
* a rounding model: the kernel's formula in fp32 torch with a bf16
  rounding exactly where the kernel rounds.  Its distance from fp64 is
  what a correct kernel must be off by;
* deliberately wrong plain-torch variants (``LN_DEFECTS``, ``CE_DEFECTS``,
  ``ADAMW_DEFECTS``), which tests/test_kernel_reference.py shows the
  checks reject.

Two kinds of bound (tests/README.md, "Row-wise and optimizer kernels"):

* outputs the kernels round to bf16 (y, sum, dx, dlogits):
  ``E(kernel) <= MARGIN * E(model)`` for E_max and E_rms, over the whole
  tensor AND per row (``compare_rows``), so a row with a small scale cannot
  hide behind the largest one;
* fp32 outputs (mean, rstd, lse, loss, AdamW's p, m, v, the squared
  norm): a bound per element written out from the arithmetic, no element
  excluded (``ln_stat_bounds``, ``ce_lse_bound``, ``ce_loss_bound``,
  ``adamw_bounds``, ``sqnorm_bound``).

Rounding points, by kernel line
-------------------------------

LayerNorm (csrc/layernorm.hip); ``ln_model``:

  L1. ``ln_add_fwd_kernel`` l.334-338: ``sum = bf16(x + res)``, and the
      statistics and the normalisation use that ROUNDED sum.       [bf16]
      ``ln_fwd_kernel`` l.40: x enters unrounded (it is bf16 already).
  L2. l.41-42 / l.339-340, l.45-48 / l.344-347: one pass, fp32:
      ``s = sum x``, ``ss = sum x*x``, ``mean = s * (1/D)``,
      ``var = max(ss * (1/D) - mean*mean, 0)``, with ``1/D`` the host's
      ``1.f / d`` (fp32), and l.49 / l.348 ``rstd = rsqrtf(var + eps)``
      with eps cast to fp32.  mean and rstd are stored in fp32.
  L3. l.59-60 / l.358-359: ``y = bf16((x - mean) * rstd * w + b)``.  [bf16]
  L4. backward (``ln_bwd_fused_kernel`` l.233-241, ``ln_bwd_dx_kernel``
      l.87-94, ``ln_add_bwd_dx_kernel`` l.392-399): ``g = dy * w``,
      ``xhat = (x - mean) * rstd``, ``sg = sum(g) * (1/D)``,
      ``sgx = sum(g * xhat) * (1/D)``, all fp32, from the SAVED fp32 mean
      and rstd.
  L5. l.102 / l.261: ``dx = bf16(rstd * (g - sg - xhat * sgx))``;
      l.258-259 / l.407: the ADD form adds ``dsum`` in fp32 BEFORE the one
      rounding: ``bf16(rstd * (...) + dsum)``.                      [bf16]

Cross-entropy (csrc/cross_entropy.hip); ``ce_model``:

  C1. ``ce_fwd_kernel`` l.31-33: row max in fp32 (exact).
  C2. l.36-38: ``s = sum __expf(l - m)`` in fp32.
  C3. l.40-42: ``lse = m + __logf(s)``, stored in fp32.
  C4. l.43-44: ``loss += (lse - l[target]) * (1/N)`` by fp32 atomics, in
      any row order; ``1/N`` is the host's ``1.f / n``.
  C5. ``ce_bwd_kernel`` l.57, l.61-63: ``scale = dloss * (1/N)``,
      ``p = __expf(l - lse)`` from the SAVED lse,
      ``dlogits = bf16((p - onehot) * scale)``.                     [bf16]

AdamW (csrc/adamw.hip ``fused_adamw_kernel``); ``adamw_model`` (all fp32,
the only bf16 is the optional mirror):

  A1. l.63: ``gs = grad_scale * prescale``; l.64-66 ``decay = 1 - lr*wd``,
      ``step_size = lr / bias_c1``, ``inv_sqrt_c2 = rsqrtf(bias_c2)``.
  A2. l.89 / l.118: ``g' = g * gs`` (bf16 grads widen exactly first).
  A3. l.90-91 / l.120-121: ``m = beta1*m + omb1*g'``,
      ``v = beta2*v + omb2*g'*g'``, omb = ``float(1 - beta)`` formed in
      double on the host.
  A4. l.92-93 / l.122: ``p = p*decay - step_size*m/(sqrtf(v)*inv_sqrt_c2
      + eps)``.
  A5. l.108 / l.126: ``mirror = bf16(p)``.                           [bf16]

``mt_sqnorm_kernel`` squares and sums in fp32 in an unspecified order
(grid-stride partial sums, a block tree, fp32 atomics); ``mt_scale_kernel``
is one fp32 multiply by ``float(factor)`` and, for bf16, one rounding.

All bf16 conversions are round-to-nearest-even on both sides.
"""

import math

import numpy as np
import torch

from tests.fmha_reference import MARGIN, error_metrics

_U = 2.0 ** -24  # fp32 unit roundoff
LN_EPS = 1e-6

# --------------------------------------------------------------------------
# measured constants
# --------------------------------------------------------------------------

# One-pass fp32 statistics.  The worst-case bound D * u has no teeth (it
# allows 12 % on the variance at D = 8192, mean = 16 std), so the bound is
#   |var32 - var64|   <= C_VAR  * u * (var + mean^2)
#   |mean32 - mean64| <= C_MEAN * u * sqrt(var + mean^2)
# i.e. c * u * (1 + mean^2/var) relative on the variance, with c fixed as
# 8 times the worst value an fp32 EMULATION reaches on the CPU (never the
# kernel): ``ln_stats_emulated`` in the three orders of ``_sum32`` over
# every (family, rows, D) of LN_CASES and both forms at LN_SEED.  The
# emulation includes the fp32 ``1/D`` and the products, so the constants
# cover them.  Measured worst
# (test_kernel_reference.test_stat_constants_cover_the_emulation prints
# and re-asserts it): variance 5.40 (`offset`, 769 x 8200, pairwise; 4.6
# in the block order, 4.3 by cumsum), mean 1.20 (`offset`, 769 x 5120).
STAT_WORST_VAR = 5.41
STAT_WORST_MEAN = 1.20
C_VAR = 8 * STAT_WORST_VAR
C_MEAN = 8 * STAT_WORST_MEAN
LN_SEED = 0

# Allowance for ``__expf`` / ``__logf`` in the cross-entropy lse, by the
# rule of fmha_reference.LSE_INTRINSIC_ALLOWANCE: measured once on an
# MI355X as the worst |lse(kernel) - lse(fp64)| / (1 + |lse|) over every
# case of tests/test_gpu_rowwise_numerics.py: 1.21e-7 (`randn`, 128 x 8,
# |lse| ~ 2: half an fp32 ulp of the stored value; 0 in both `peaked`
# families, where lse is the peak logit exactly).  The figure contains
# the fp32 summation and the final rounding too, so it over-states the
# intrinsics; the constant is 8 times it all the same.  ce_check prints
# the figure for every case ("err/(1+|lse|)").
CE_LSE_MEASURED = 1.21e-7
CE_LSE_ALLOWANCE = 8 * CE_LSE_MEASURED


def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _f32(v):
    return float(np.float32(v))


# --------------------------------------------------------------------------
# generic checkers
# --------------------------------------------------------------------------

def row_metrics(x, ref):
    """Per-row (E_max, E_rms) of x against the fp64 ref [rows, n], defined
    like fmha_reference.error_metrics; a row whose ref is identically zero
    gets its absolute errors."""
    ref = ref.double()
    d = x.double() - ref
    e_max, e_rms = d.abs().amax(-1), d.pow(2).mean(-1).sqrt()
    r_max, r_rms = ref.abs().amax(-1), ref.pow(2).mean(-1).sqrt()
    zero = r_max == 0
    one = torch.ones_like(r_max)
    return (e_max / torch.where(zero, one, r_max),
            e_rms / torch.where(zero, one, r_rms))


def compare_rows(got, model, ref64, name="", floor=None):
    """E(kernel) vs MARGIN * E(model), E_max and E_rms, whole tensor and
    per row.  ``floor`` is an optional per-row ABSOLUTE error [rows] that
    is accepted whatever the model's error (derived bounds for rows where
    a ratio says nothing: ``ln_floors``, ``ce_dlogits_floor``).  Prints
    one line; returns (ok, worst whole-tensor max ratio, rms ratio,
    worst per-row max ratio, rms ratio, number of bad rows)."""
    ref64 = ref64.double().reshape(-1, ref64.shape[-1])
    got = got.reshape(ref64.shape)
    model = model.reshape(ref64.shape)
    gm, gr = error_metrics(got, ref64)
    mm, mr = error_metrics(model, ref64)
    rgm, rgr = row_metrics(got, ref64)
    rmm, rmr = row_metrics(model, ref64)
    if floor is None:
        fl_max = fl_rms = torch.zeros_like(rgm)
        fl_all = 0.0
    else:
        floor = floor.double().reshape(-1)
        r_max, r_rms = ref64.abs().amax(-1), ref64.pow(2).mean(-1).sqrt()
        one = torch.ones_like(r_max)
        fl_max = floor / torch.where(r_max == 0, one, r_max)
        fl_rms = floor / torch.where(r_max == 0, one, r_rms)
        t_max = ref64.abs().max().item()
        fl_all = floor.max().item() / (t_max if t_max else 1.0)
    ok_all = gm <= max(MARGIN * mm, fl_all) and gr <= max(MARGIN * mr, fl_all)
    row_ok = ((rgm <= torch.maximum(MARGIN * rmm, fl_max))
              & (rgr <= torch.maximum(MARGIN * rmr, fl_rms)))
    n_bad = int((~row_ok).sum())

    def worst(a, b, fl):
        # ratio of rows the floor does not already accept
        live = a > fl
        r = torch.where(live & (b > 0), a / b.clamp_min(1e-300),
                        torch.where(live, torch.full_like(a, float("inf")),
                                    torch.zeros_like(a)))
        return r.max().item()

    w_max, w_rms = worst(rgm, rmm, fl_max), worst(rgr, rmr, fl_rms)
    a_max = gm / mm if mm else (0.0 if gm <= fl_all else float("inf"))
    a_rms = gr / mr if mr else (0.0 if gr <= fl_all else float("inf"))
    ok = bool(ok_all and n_bad == 0)
    print(f"rowwise-check {name}: E_max kernel {gm:.3e} model {mm:.3e} ratio "
          f"{a_max:.2f} | E_rms kernel {gr:.3e} model {mr:.3e} ratio "
          f"{a_rms:.2f} | per row: worst max ratio {w_max:.2f}, rms ratio "
          f"{w_rms:.2f}, {n_bad} of {row_ok.numel()} rows out | "
          f"{'ok' if ok else 'FAIL'}")
    return ok, a_max, a_rms, w_max, w_rms, n_bad


# --------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------

LN_FAMILIES = ("randn", "offset", "row_scale", "special")
CONST_VALUE = 0.30078125  # bf16(0.3), the `special` family's constant row

# (rows, D) of tests/test_gpu_rowwise_numerics.py.  D: 8 one vector, 64 a
# small row, 2048 VPT 1 full, 2056 VPT 2 with one thread in the second
# slot, 4096 VPT 2 full, 5120 VPT 3 (production), 8192 VPT 4, 8200 the
# two-kernel path.  Rows: 769 = kFusedBlocks + 1, so block 0 walks two
# rows; 1037 is no multiple of anything.  Every D has rows = 3 and one
# count above 768; rows x D stays below 10M elements.
LN_CASES = (
    (1, 8), (3, 8), (769, 8),
    (3, 64), (1037, 64),
    (1, 2048), (3, 2048), (769, 2048),
    (3, 2056), (769, 2056),
    (3, 4096), (1037, 4096),
    (1, 5120), (3, 5120), (769, 5120),
    (3, 8192), (1037, 8192),
    (3, 8200), (769, 8200),
)


def ln_special_rows(rows):
    """(zero rows, constant rows) of the `special` family."""
    if rows < 3:
        return [], []
    zero, const = [0], [1]
    if rows > 768:  # rows a block reaches on its second walk
        zero.append(rows - 2)
        const.append(rows - 1)
    return zero, const


def ln_make_inputs(family, rows, d, seed, device="cpu"):
    """bf16 x, res, w, b, dy, dsum.  Drawn on the CPU so that (family,
    shape, seed) names the same numbers everywhere.  w, b, dy and dsum
    are random, never ones or zeros."""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    x, res = rn(rows, d), 0.5 * rn(rows, d)
    if family == "offset":
        x = x + 16.0
    elif family == "row_scale":
        k = (torch.arange(rows) % 13 - 6).float()
        sc = torch.pow(2.0, k).unsqueeze(1)
        x, res = x * sc, res * sc
    elif family == "special":
        zero, const = ln_special_rows(rows)
        for r in zero:
            x[r], res[r] = 0.0, 0.0
        for r in const:
            x[r], res[r] = CONST_VALUE, 0.0
    elif family != "randn":
        raise ValueError(family)
    w, b = 1.0 + 0.5 * rn(d), rn(d)
    dy, dsum = rn(rows, d), rn(rows, d)
    return tuple(t.to(torch.bfloat16).to(device)
                 for t in (x, res, w, b, dy, dsum))


def ln_fp64(x, w, b, dy=None, dsum=None, res=None, eps=LN_EPS, s_bf16=None):
    """y, mean, var, rstd (and sum, dx) in float64.

    Forward of the ADD form: the exact sum x + res and its LayerNorm.
    Backward: dx of the plain form from x, of the ADD form from the bf16
    sum ``s_bf16`` the forward SAVED (that tensor is the backward's
    input), plus dsum."""
    xs = x.double() if res is None else x.double() + res.double()
    w, b = w.double(), b.double()
    mean = xs.mean(-1, keepdim=True)
    var = ((xs - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    out = {"sum": xs, "y": (xs - mean) * rstd * w + b,
           "mean": mean.squeeze(-1), "var": var.squeeze(-1),
           "rstd": rstd.squeeze(-1)}
    if dy is not None:
        xb = xs if s_bf16 is None else s_bf16.double()
        mb = xb.mean(-1, keepdim=True)
        vb = ((xb - mb) ** 2).mean(-1, keepdim=True)
        rb = 1.0 / torch.sqrt(vb + eps)
        gg = dy.double() * w
        xh = (xb - mb) * rb
        dx = rb * (gg - gg.mean(-1, keepdim=True)
                   - xh * (gg * xh).mean(-1, keepdim=True))
        if dsum is not None:
            dx = dx + dsum.double()
        out.update(dx=dx, bwd_mean=mb.squeeze(-1), bwd_var=vb.squeeze(-1),
                   bwd_rstd=rb.squeeze(-1), g=gg, xhat=xh)
    return out


SUM_ORDERS = ("pairwise", "cumsum", "block")


def _sum32(t, order):
    """fp32 sum of [rows, D] over D in one of three orders:

    'pairwise': ``torch.sum`` (blocked cascade);
    'cumsum':   the last element of ``torch.cumsum`` (sequential; on the
                CPU torch carries this one in a wider accumulator, so it
                is the nearly-exact end of the range);
    'block':    the order of the kernels' 256-thread block in plain fp32:
                thread t adds elements 8 (t + 256 k) + j in sequence
                (k outer, j inner), a butterfly over the 64 lanes of a
                wave (``wave_all_sum``), then the four waves in sequence
                (``block_sum``).
    A naive sequential fp32 sum of a whole row (numpy's float32 cumsum)
    reaches 350 in the units of C_VAR at D = 8200, mean = 16 std; no
    kernel here chains more than about 50 additions (40 per thread at
    D = 8200, the wave butterfly, four waves), and one that chained
    thousands would rightly fail the bound."""
    if order == "pairwise":
        return t.sum(-1, keepdim=True)
    if order == "cumsum":
        return t.cumsum(-1)[..., -1:]
    assert order == "block", order
    rows, d = t.shape
    nvec = d // 8
    vpt = (nvec + 255) // 256
    tv = torch.zeros(rows, vpt * 256, 8, dtype=t.dtype, device=t.device)
    tv[:, :nvec] = t.reshape(rows, nvec, 8)
    tv = tv.view(rows, vpt, 256, 8)
    acc = torch.zeros(rows, 256, dtype=t.dtype, device=t.device)
    for k in range(vpt):
        for j in range(8):
            acc = acc + tv[:, k, :, j]
    a = acc.view(rows, 4, 64)
    lane = torch.arange(64, device=t.device)
    off = 32
    while off:
        a = a + a[:, :, lane ^ off]
        off //= 2
    tot = torch.zeros(rows, dtype=t.dtype, device=t.device)
    for wv in range(4):
        tot = tot + a[:, wv, 0]
    return tot.unsqueeze(-1)


def ln_stats_emulated(xs, eps=LN_EPS, order="pairwise", defect=None):
    """mean, var, rstd [rows, 1] of the fp32 rows xs by the kernels' one-
    pass formula (L2), with an optional defect."""
    d = xs.shape[-1]
    inv_d = torch.tensor(np.float32(1.0) / np.float32(d), device=xs.device)
    eps32 = _f32(1e-5 if defect == "eps_1e-5" else eps)
    src = xs[..., :d - 8] if defect == "stats_skip_last_vec" else xs
    s = _sum32(src, order)
    ss = _sum32(src * src, order)
    if defect == "mean_over_d_minus_8":
        mean = s * torch.tensor(np.float32(1.0) / np.float32(d - 8))
    else:
        mean = s * inv_d
    var = torch.clamp(ss * inv_d - mean * mean, min=0.0)
    if defect == "unbiased_var":
        var = var * _f32(d / (d - 1.0))
    return mean, var, torch.rsqrt(var + eps32)


# defect -> the D below which it does not exist
LN_DEFECTS = {
    "unbiased_var": 8,
    "eps_1e-5": 8,
    "mean_over_d_minus_8": 16,
    "stats_skip_last_vec": 16,
    "dx_no_mean_g": 8,
    "dx_no_xhat_term": 8,
    "dx_w_neighbour_vector": 16,
    "add_no_dsum": 8,
}


def ln_model(x, w, b, dy=None, dsum=None, res=None, eps=LN_EPS,
             order="pairwise", defect=None):
    """The kernels' arithmetic (L1-L5) in fp32 torch, with an optional
    defect from LN_DEFECTS.  The backward uses the model's own mean and
    rstd, as the kernels' backward uses the forward's."""
    w, b = w.float(), b.float()
    if res is None:
        xs = x.float()
    else:
        xs = _bf(x.float() + res.float())                          # L1
    mean, var, rstd = ln_stats_emulated(xs, eps, order, defect)    # L2
    out = {"sum": xs, "y": _bf((xs - mean) * rstd * w + b),        # L3
           "mean": mean.squeeze(-1), "var": var.squeeze(-1),
           "rstd": rstd.squeeze(-1)}
    if dy is not None:
        d = xs.shape[-1]
        inv_d = _f32(np.float32(1.0) / np.float32(d))
        wg = w.roll(8) if defect == "dx_w_neighbour_vector" else w
        gg = dy.float() * wg                                       # L4
        xh = (xs - mean) * rstd
        sg = gg.sum(-1, keepdim=True) * inv_d
        sgx = (gg * xh).sum(-1, keepdim=True) * inv_d
        if defect == "dx_no_mean_g":
            sg = torch.zeros_like(sg)
        if defect == "dx_no_xhat_term":
            sgx = torch.zeros_like(sgx)
        dx = rstd * (gg - sg - xh * sgx)                           # L5
        if dsum is not None and defect != "add_no_dsum":
            dx = dx + dsum.float()
        out["dx"] = _bf(dx)
    return out


def ln_stat_bounds(xs64, eps=LN_EPS):
    """Per-row absolute bounds on the kernels' fp32 mean and rstd, from
    the fp64 rows the statistics are taken of.

    mean: C_MEAN * u * sqrt(var + mean^2) (sum, ``1.f / d`` and product).
    var: C_VAR * u * (var + mean^2) =: dvar.  rstd = (var + eps)^-1/2 is
    monotone, so it lies between its values at var +- dvar (clamped at 0
    like the kernel); on top 4u relative: eps cast to fp32 and added (2u
    on the radicand, u on rstd) and ``rsqrtf`` within 1 ulp (2u) and a
    spare u.  No linearisation: for a constant row dvar exceeds eps and
    the interval is wide, as the kernel's rstd really is."""
    mean = xs64.mean(-1)
    var = ((xs64 - mean.unsqueeze(-1)) ** 2).mean(-1)
    ms = var + mean * mean
    dmean = C_MEAN * _U * torch.sqrt(ms)
    dvar = C_VAR * _U * ms
    rstd = 1.0 / torch.sqrt(var + eps)
    hi = 1.0 / torch.sqrt(torch.clamp(var - dvar, min=0.0) + eps)
    lo = 1.0 / torch.sqrt(var + dvar + eps)
    drstd = torch.maximum(hi - rstd, rstd - lo) + 4 * _U * hi
    return {"mean": mean, "var": var, "rstd": rstd, "dmean": dmean,
            "dvar": dvar, "drstd": drstd, "rstd_hi": hi}


def ln_floors(xs64, w, b, dy=None, dsum=None, eps=LN_EPS):
    """Absolute per-row error floors for y and dx, used ONLY on rows whose
    fp64 variance is exactly zero (zero rows and constant rows); every
    other row gets 0, i.e. the pure model-relative check.

    On such a row the fp64 answers are y = b and dx = rstd (g - mean g),
    the model may hit them exactly and the kernel need not: with another
    summation order its mean is off by up to dmean and its rstd lies
    anywhere in the interval of ln_stat_bounds.  Like _floors in
    test_gpu_fmha_numerics.py the floor is what that leaves:

      |xhat| <= dmean * rstd_hi =: xh
      |y - b| <= xh * max|w|, plus the bf16 store (2^-8 relative, on
          max|b| + xh max|w|)
      |dx - dx64| <= drstd * max|g - mean g|            (rstd)
                     + rstd_hi * C_MEAN u rms(g)        (fp32 sum of g)
                     + rstd_hi * xh^2 * mean|g|         (xhat * sgx)
          plus the bf16 store on max|dx64| (+ max|dsum|) + the above.
    For a zero row dmean = dvar = 0 and only the bf16 store and the sum
    of g are left."""
    st = ln_stat_bounds(xs64, eps)
    degenerate = st["var"] == 0
    w64 = w.double()
    xh = st["dmean"] * st["rstd_hi"]
    wmax = w64.abs().max()
    fy = xh * wmax
    fy = fy + 2.0 ** -8 * (b.double().abs().max() + fy)
    out = {"y": torch.where(degenerate, fy, torch.zeros_like(fy))}
    if dy is not None:
        gg = dy.double() * w64
        gc = gg - gg.mean(-1, keepdim=True)
        fdx = (st["drstd"] * gc.abs().amax(-1)
               + st["rstd_hi"] * C_MEAN * _U * gg.pow(2).mean(-1).sqrt()
               + st["rstd_hi"] * xh * xh * gg.abs().mean(-1))
        mag = st["rstd"] * gc.abs().amax(-1) + fdx
        if dsum is not None:
            mag = mag + dsum.double().abs().amax(-1)
        fdx = fdx + 2.0 ** -8 * mag
        out["dx"] = torch.where(degenerate, fdx, torch.zeros_like(fdx))
    return out


def ln_assert_family(family, xs64, rows):
    """Each family re-asserts from the fp64 rows what it claims to
    stress."""
    mean = xs64.mean(-1)
    std = ((xs64 - mean.unsqueeze(-1)) ** 2).mean(-1).sqrt()
    if family == "offset":
        # bf16 has 3 fractional bits at 16, the rows keep a std near 1.
        # The sample std of only 8 draws scatters: chi^2 with 7 degrees
        # puts it outside (0.1, 2.5) with probability < 1e-5 per row; the
        # ADD form's sum has std 1.12 (x + 0.5 randn), and the largest
        # sample std of 1037 rows of 64 is a third above that.
        k, lo = (8, 0.5) if xs64.shape[-1] >= 64 else (5, 0.1)
        assert bool((mean.abs() > k * std).all()), "offset: mean too small"
        assert bool((std > lo).all())
    elif family == "row_scale" and rows >= 13:
        assert std.max() / std.min() > 2.0 ** 11, "row_scale: < 2^11 spread"
    elif family == "special" and rows >= 3:
        zero, const = ln_special_rows(rows)
        for r in zero:
            assert float(xs64[r].abs().max()) == 0.0
        for r in const:
            assert float(std[r]) == 0.0 and float(mean[r]) != 0.0
        assert int((std == 0).sum()) == len(zero) + len(const)


def ln_old_tolerance_passes(got, ref64):
    """The fixed tolerances of test_gpu_kernels.py / test_gpu_ln_bwd_fused
    (y: rtol 0.05, atol 0.03; dx: rtol 0.1, atol 0.05; the ADD form's dx:
    atol 0.1).  Reported, never asserted."""
    res = {}
    for t, rtol, atol in (("y", 0.05, 0.03), ("dx", 0.1, 0.05)):
        if t in got and t in ref64:
            ref = ref64[t].double()
            res[t] = bool(((got[t].double() - ref).abs()
                           <= atol + rtol * ref.abs()).all())
    return res


# --------------------------------------------------------------------------
# cross-entropy
# --------------------------------------------------------------------------

CE_FAMILIES = ("randn", "peaked_target", "peaked_other", "common_offset",
               "masked")
CE_CLASSES = (1, 8, 255, 256, 257, 1000, 1001, 4099)
CE_ROWS = (1, 3, 128)
CE_DLOSS = (1.0, 0.37)


def ce_make_inputs(family, n, c, seed, device="cpu"):
    """bf16 logits [n, c] and int64 in-range targets that include 0 and
    c - 1 in every case (row 0 -> class 0, the last row -> c - 1 when
    n > 1; with one row the target is c - 1 and `seed` odd/even picks 0
    instead)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, c, generator=g)
    target = torch.randint(0, c, (n,), generator=g)
    if n == 1:
        target[0] = 0 if seed % 2 else c - 1
    else:
        target[0], target[-1] = 0, c - 1
    rows = torch.arange(n)
    if family == "peaked_target":
        logits[rows, target] += 30.0
    elif family == "peaked_other" and c > 1:
        logits[rows, (target + 1 + c // 2) % c if c > 2 else 1 - target] += 30.0
    elif family == "common_offset":
        logits += 200.0
    elif family == "masked" and c > 1:
        mask = torch.rand(n, c, generator=g) < 0.3
        mask[rows, target] = False
        logits[mask] = float("-inf")
    elif family not in CE_FAMILIES:
        raise ValueError(family)
    return logits.to(torch.bfloat16).to(device), target.to(device)


def ce_fp64(logits, target, dloss=1.0):
    l = logits.double()
    n = l.shape[0]
    lse = torch.logsumexp(l, dim=-1)
    tl = l.gather(1, target.view(-1, 1)).squeeze(1)
    p = torch.exp(l - lse.unsqueeze(1))
    onehot = torch.zeros_like(l).scatter_(1, target.view(-1, 1), 1.0)
    return {"lse": lse, "loss": (lse - tl).mean(), "p": p, "tl": tl,
            "dlogits": (p - onehot) * (float(dloss) / n)}


CE_DEFECTS = ("lse_first_full_blocks", "grad_n_plus_1", "lse_off_0.04",
              "target_shifted", "dloss_ignored")


def ce_model(logits, target, dloss=1.0, defect=None):
    """The kernels' arithmetic (C1-C5) in fp32 torch, ``torch.exp`` /
    ``torch.log`` in place of the fast intrinsics, with an optional
    defect.  The backward runs from the model's own lse, as the kernel's
    runs from the forward's."""
    l = logits.float()
    n, c = l.shape
    inv_n = _f32(np.float32(1.0) / np.float32(n))
    lv = l
    if defect == "lse_first_full_blocks" and c >= 256 and c % 256:
        lv = l[:, :c - c % 256]
    m = lv.max(-1, keepdim=True).values                             # C1
    s = torch.exp(lv - m).sum(-1, keepdim=True)                     # C2
    lse = (m + torch.log(s)).squeeze(1)                             # C3
    if defect == "lse_off_0.04":
        lse = lse + _f32(0.04)
    tgt = (target + 1) % c if defect == "target_shifted" else target
    tl = l.gather(1, tgt.view(-1, 1)).squeeze(1)
    loss = ((lse - tl) * inv_n).sum()                               # C4
    scale = _f32(1.0 if defect == "dloss_ignored" else dloss)
    if defect == "grad_n_plus_1":
        scale = _f32(np.float32(scale) * np.float32(1.0)
                     / np.float32(n + 1))
    else:
        scale = _f32(np.float32(scale) * np.float32(inv_n))         # C5
    p = torch.exp(l - lse.unsqueeze(1))
    onehot = torch.zeros_like(l).scatter_(1, tgt.view(-1, 1), 1.0)
    return {"lse": lse, "loss": loss, "dlogits": _bf((p - onehot) * scale)}


def ce_lse_bound(logits, ref64):
    """Per-row absolute bound on |lse(kernel) - lse(fp64)|.

    ``l - m`` is a difference of two bf16 values formed in fp32: rounded
    once, u |l - m|, which the exponential turns into a relative error of
    its term; over the row that is u * sum_j p_j |l_j - m| of log(s).  The
    sum of C positive fp32 terms in ANY order is within (C - 1) u
    relative, absolute on log(s).  ``m + log(s)`` is rounded once,
    u |lse|.  On top CE_LSE_ALLOWANCE * (1 + |lse|) for the intrinsics."""
    l = logits.double()
    c = l.shape[1]
    m = l.max(-1, keepdim=True).values
    gap = torch.where(torch.isfinite(l), (l - m).abs(), torch.zeros_like(l))
    lse = ref64["lse"].abs()
    return (_U * (ref64["p"] * gap).sum(-1) + (c - 1) * _U + _U * lse
            + CE_LSE_ALLOWANCE * (1.0 + lse))


def ce_loss_bound(logits, ref64):
    """Absolute bound on the mean loss: per row the lse bound, u for the
    subtraction and u for the ``* (1/N)`` with its fp32 ``1/N`` (3u on
    |lse - tl| with the product's rounding); the N atomics add in any
    order, within (N - 1) u of the sum of the |terms|; the terms are
    non-negative up to the lse bound."""
    n = logits.shape[0]
    t = (ref64["lse"] - ref64["tl"]).abs()
    per_row = ce_lse_bound(logits, ref64) + 3 * _U * t
    return per_row.mean() + (n - 1) * _U * (t + per_row).mean()


def ce_dlogits_floor(logits, ref64, dloss):
    """Absolute per-row floor for dlogits.  The backward forms
    ``p = exp(l - lse)`` from an fp32 lse that may be off by the lse bound
    and an argument rounded once (u |l - lse|), so p carries that much
    RELATIVE error however small ``p - 1`` is: at a `peaked_target` row
    the true gradient is ~1e-10 and every fp32 evaluation is off by up to
    ulp(lse).  |scale| * max_j p_j (bound_lse + u |l_j - lse| + allowance)
    is what that leaves; on ordinary rows it is three orders of magnitude
    below the bf16 rounding and changes nothing."""
    l = logits.double()
    n = l.shape[0]
    lse = ref64["lse"].unsqueeze(1)
    gap = torch.where(torch.isfinite(l), (l - lse).abs(), torch.zeros_like(l))
    rel = (ce_lse_bound(logits, ref64).unsqueeze(1) + _U * gap
           + CE_LSE_ALLOWANCE)
    return (abs(float(dloss)) / n) * (ref64["p"] * rel).amax(-1) * (
        1 + 2.0 ** -8)


def ce_assert_family(family, logits, target, ref64):
    c = logits.shape[1]
    if c == 1:
        return
    pt = ref64["p"].gather(1, target.view(-1, 1)).squeeze(1)
    row_loss = ref64["lse"] - ref64["tl"]
    if family == "peaked_target":
        # p - 1 cancels below fp32 resolution
        assert bool((1.0 - pt < 2.0 ** -24).all()), float((1 - pt).max())
    elif family == "peaked_other":
        assert bool((row_loss > 20).all()), float(row_loss.min())
    elif family == "common_offset":
        # an unshifted fp32 exp overflows at 88.7
        assert float(logits.double().min()) > 150
    elif family == "masked":
        ninf = torch.isinf(logits.double())
        assert bool(ninf.any()) or c < 8
        assert bool(torch.isfinite(ref64["tl"]).all())
        assert bool((ref64["dlogits"][ninf] == 0).all())


def ce_old_tolerance_passes(got, ref64):
    """test_cross_entropy_fwd_bwd: |loss - ref| < 0.02; dlogits rtol 0.05,
    atol 1e-4."""
    ref = ref64["dlogits"]
    return {
        "loss": abs(float(got["loss"]) - float(ref64["loss"])) < 0.02,
        "dlogits": bool(((got["dlogits"].double() - ref).abs()
                         <= 1e-4 + 0.05 * ref.abs()).all()),
    }


# --------------------------------------------------------------------------
# AdamW
# --------------------------------------------------------------------------

ADAMW_SIZES = (1, 2, 3, 4, 5, 7, 8, 1023, 100003)
BETA1, BETA2 = 0.9, 0.999


def adamw_hyper(t, wd=0.1, lr=1e-2, eps=1e-8, prescale=1.0, grad_scale=None):
    return dict(lr=lr, beta1=BETA1, beta2=BETA2, eps=eps, wd=wd,
                bias_c1=1.0 - BETA1 ** t, bias_c2=1.0 - BETA2 ** t,
                prescale=prescale, grad_scale=grad_scale, t=t)


def adamw_make_inputs(n, seed, state="random", grad_dtype=torch.float32,
                      extra=0, device="cpu"):
    """p, m, v (fp32) and g (``grad_dtype``, ``extra`` elements longer
    than p).  Magnitudes span four decades per element (scale
    10^-4..1), so that eps is felt next to sqrt(v) on part of the
    elements; state='zeros' is the state of a real first step."""
    gen = torch.Generator().manual_seed(seed)

    def rn(k):
        return torch.randn(k, generator=gen)

    sc = torch.pow(10.0, -4.0 * torch.rand(n + extra, generator=gen))
    p = rn(n)
    g = (rn(n + extra) * sc).to(grad_dtype)
    if state == "zeros":
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m = 0.3 * rn(n) * sc[:n]
        m = torch.where(m == 0, torch.full_like(m, 1e-3), m)
        v = (rn(n) * sc[:n]) ** 2
    return tuple(t.to(device) for t in (p, m, v, g))


def _gs64(h):
    gs = 1.0 if h["grad_scale"] is None else float(h["grad_scale"])
    return gs * h["prescale"]


def adamw_fp64(p, m, v, g, h):
    """One decoupled-weight-decay Adam step in float64 (the math of
    torch.optim.AdamW), hyper-parameters as python doubles."""
    n = p.numel()
    p, m, v = p.double(), m.double(), v.double()
    gj = g.double()[:n] * _gs64(h)
    m2 = h["beta1"] * m + (1.0 - h["beta1"]) * gj
    v2 = h["beta2"] * v + (1.0 - h["beta2"]) * gj * gj
    denom = torch.sqrt(v2) / math.sqrt(h["bias_c2"]) + h["eps"]
    upd = (h["lr"] / h["bias_c1"]) * m2 / denom
    pd = p * (1.0 - h["lr"] * h["wd"])
    return {"p": pd - upd, "m": m2, "v": v2, "gj": gj, "upd": upd,
            "pd": pd, "denom": denom}


ADAMW_DEFECTS = ("decay_after_update", "eps_inside_sqrt", "prescale_m_only",
                 "bias_prev_step", "one_minus_beta2_fp32")


def adamw_model(p, m, v, g, h, defect=None):
    """The kernel's arithmetic (A1-A4) in fp32 torch with an optional
    defect.  ``one_minus_beta2_fp32`` is what the kernel did before
    1 - beta came from the host in double."""
    n = p.numel()
    f = np.float32
    lr, b1, b2, eps, wd = (f(h[k]) for k in ("lr", "beta1", "beta2", "eps",
                                              "wd"))
    c1, c2 = h["bias_c1"], h["bias_c2"]
    if defect == "bias_prev_step":
        c1, c2 = 1.0 - BETA1 ** (h["t"] - 1), 1.0 - BETA2 ** (h["t"] - 1)
    c1, c2 = f(c1), f(c2)
    omb1 = f(1.0 - h["beta1"])
    omb2 = (f(1.0) - b2) if defect == "one_minus_beta2_fp32" else f(
        1.0 - h["beta2"])
    gscale = f(1.0) if h["grad_scale"] is None else f(h["grad_scale"])
    gs = float(gscale * f(h["prescale"]))                           # A1
    decay = float(f(1.0) - lr * wd)
    step = float(lr / c1)
    isc2 = float(f(1.0) / np.sqrt(c2))
    p, m, v = p.float(), m.float(), v.float()
    gj = g.float()[:n] * gs                                         # A2
    gv = g.float()[:n] * float(gscale) if defect == "prescale_m_only" else gj
    m2 = float(b1) * m + float(omb1) * gj                           # A3
    v2 = float(b2) * v + float(omb2) * gv * gv
    if defect == "eps_inside_sqrt":
        denom = torch.sqrt(v2 * (isc2 * isc2) + float(eps))
    else:
        denom = torch.sqrt(v2) * isc2 + float(eps)
    if defect == "decay_after_update":
        p2 = (p - step * m2 / denom) * decay
    else:
        p2 = p * decay - step * m2 / denom                          # A4
    return {"p": p2, "m": m2, "v": v2}


def adamw_bounds(ref64, p, m, v, h, prev=None):
    """Per-element absolute bounds on the kernel's p, m, v against
    adamw_fp64, u = 2^-24 per fp32 rounding (a fused multiply-add rounds
    less, never more).

    g' = g * gs: gs = fl(fl(grad_scale) * fl(prescale)) 2u (the device
      scalar is fp32 already), the product u: 3u.
    m: fl(beta1) u and its product u: 2u on |beta1 m|; omb1 u, product u,
      g' 3u: 5u on |omb1 g'|; the sum u on both: 3u, 6u.
    v: likewise 3u on beta2 v; omb2 u, two products 2u, g' twice 6u, the
      sum u: 10u on omb2 g'^2.  Both terms are non-negative, so v is
      within 10u RELATIVE and sqrt(v) within 5u.
    p: decay = fl(1 - fl(fl(lr) fl(wd))) is within u + 3u lr wd <= 2u of
      1 - lr wd, the product p * decay u: 3u on |p decay|.
      step_size = fl(lr) / fl(c1): 3u.  inv_sqrt_c2: c2 u -> u/2, rsqrtf
      1 ulp = 2u: 2.5u.  sqrtf 1 ulp = 2u after v's 5u, the product u:
      10.5u on sqrt(v) inv_sqrt_c2; fl(eps) u; the sum u: denom within
      11.5u.  update = step_size * m / denom: 3u + 11.5u + u + 2u (the
      division within 1 ulp) = 17.5u -> 18u relative, plus m's absolute
      error times step_size / denom.  The final subtraction u on
      |p decay| + |update|."""
    gj = ref64["gj"].abs()
    b1, b2 = h["beta1"], h["beta2"]
    bm = _U * (3 * (b1 * m.double()).abs() + 6 * (1 - b1) * gj)
    bv = _U * (3 * b2 * v.double().abs() + 10 * (1 - b2) * gj * gj)
    step = h["lr"] / h["bias_c1"]
    upd, pd = ref64["upd"].abs(), ref64["pd"].abs()
    bp = 4 * _U * pd + 19 * _U * upd
    if prev is not None:
        # the step started from a state that was already off by `prev`
        # (to first order): m and v carry beta times it, p the decay
        # times it, and the update half of v's relative error
        bm = bm + b1 * prev["m"]
        bp = bp + (1.0 - h["lr"] * h["wd"]) * prev["p"]
        carried = b2 * prev["v"]
        bv = bv + carried
        bp = bp + upd * 0.5 * torch.where(
            ref64["v"] > 0, carried / ref64["v"].clamp_min(1e-300),
            torch.zeros_like(carried))
    bp = bp + step * bm / ref64["denom"]
    return {"p": bp, "m": bm, "v": bv}


def adamw_old_tolerance_passes(got, ref64):
    """test_fused_adamw_matches_torch: p at rtol 1e-5, atol 1e-6 (m and v
    were never looked at)."""
    ref = ref64["p"]
    return bool(((got["p"].double() - ref).abs()
                 <= 1e-6 + 1e-5 * ref.abs()).all())


# --------------------------------------------------------------------------
# multi-tensor squared norm / scale
# --------------------------------------------------------------------------

MT_LIST_LENGTHS = (1, 32, 33, 65)


def mt_sizes(count, base):
    """`count` sizes whose tails (n mod 8) run through 0..7, starting at
    `base`: base, base + 1, ..."""
    return [base + i for i in range(count)]


def small_int_tensor(n, seed, dtype, device="cpu"):
    """Integers in -2..2: squares and their sums are exact in fp32 in any
    order while the total stays below 2^24."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, (n,), generator=g).to(dtype).to(device)


def sqnorm_bound(tensors):
    """|sqnorm(kernel) - fp64| for arbitrary data: each square is rounded
    once (u), and a sum of n non-negative fp32 terms in ANY order is
    within (n - 1) u relative.  n u * total is all that can be said
    without fixing the order, and it is weak (6e-3 at 1e5 elements): the
    exact small-integer tests are what sees a dropped element."""
    n = sum(t.numel() for t in tensors)
    total = sum(float(t.double().pow(2).sum()) for t in tensors)
    return total, n * _U * total * (1 + _U) + _U * total


def scale_reference(x, factor):
    """mt_scale bit for bit: one fp32 multiply by float(factor), one
    rounding to the tensor's dtype."""
    f = torch.tensor(np.float32(factor), device=x.device)
    return (x.float() * f).to(x.dtype)


# --------------------------------------------------------------------------
# whole-operation checks (shared by the CPU and the GPU tests)
# --------------------------------------------------------------------------

def _finish(results, name, do_assert):
    bad = {k: v[1:] for k, v in results.items() if not v[0]}
    if do_assert:
        assert not bad, f"{name}: outside the bound: {bad}"
    return results


def ln_check(got, inp, form, name="", do_assert=True, eps=LN_EPS):
    """Every output of one LayerNorm forward (+ backward) against fp64.

    ``got``: y, mean, rstd, for form 'add' also sum, and dx if the
    backward ran.  The statistics' reference is the fp64 statistics of
    what the kernel takes them of: x, or the bf16 sum, which must equal
    ``bf16(x + res)`` bit for bit (one add, one rounding).  Returns
    {tensor: (ok, figures...)}."""
    x, res, w, b, dy, dsum = inp
    add = form == "add"
    has_dx = "dx" in got
    args = dict(dy=dy if has_dx else None, dsum=dsum if add and has_dx else
                None, res=res if add else None, eps=eps)
    model = ln_model(x, w, b, **args)
    ref = ln_fp64(x, w, b, s_bf16=model["sum"] if add else None, **args)
    xs = model["sum"].double()
    st = ln_stat_bounds(xs, eps)
    fl = ln_floors(xs, w, b, args["dy"], args["dsum"], eps)
    out = {}
    for t, bound in (("mean", "dmean"), ("rstd", "drstd")):
        if t not in got:  # through the autograd op: not returned
            continue
        assert got[t].dtype == torch.float32 and got[t].shape == st[t].shape
        err = (got[t].double() - st[t]).abs()
        ratio = (err / st[bound].clamp_min(1e-300)).max().item()
        ok = bool((err <= st[bound]).all())
        print(f"rowwise-check {name} {t}: max err {err.max().item():.3e}, "
              f"worst err/bound {ratio:.3f} | {'ok' if ok else 'FAIL'}")
        out[t] = (ok, ratio)
    if add:
        same = torch.equal(got["sum"].float(), model["sum"])
        out["sum"] = (same,) + compare_rows(got["sum"], model["sum"],
                                            ref["sum"], f"{name} sum")[1:]
    out["y"] = compare_rows(got["y"], model["y"], ref["y"], f"{name} y",
                            fl["y"])
    if has_dx:
        out["dx"] = compare_rows(got["dx"], model["dx"], ref["dx"],
                                 f"{name} dx", fl["dx"])
    return _finish(out, name, do_assert), ref, model


def ce_check(got, logits, target, dloss, name="", do_assert=True):
    """lse and loss (fp32, absolute bounds) and dlogits (bf16, model-
    relative per row with the fp32-resolution floor) against fp64."""
    ref = ce_fp64(logits, target, dloss)
    model = ce_model(logits, target, dloss)
    out = {}
    bound = ce_lse_bound(logits, ref)
    err = (got["lse"].double() - ref["lse"]).abs()
    ok = bool((err <= bound).all()) and got["lse"].dtype == torch.float32
    fig = (err / (1.0 + ref["lse"].abs())).max().item()
    print(f"rowwise-check {name} lse: max err {err.max().item():.3e}, worst "
          f"err/bound {(err / bound).max().item():.3f}, err/(1+|lse|) "
          f"{fig:.3e} | {'ok' if ok else 'FAIL'}")
    out["lse"] = (ok, (err / bound).max().item(), fig)
    lb = ce_loss_bound(logits, ref).item()
    le = abs(float(got["loss"]) - float(ref["loss"]))
    print(f"rowwise-check {name} loss: err {le:.3e}, bound {lb:.3e} | "
          f"{'ok' if le <= lb else 'FAIL'}")
    out["loss"] = (le <= lb, le / lb)
    if "dlogits" in got:
        out["dlogits"] = compare_rows(
            got["dlogits"], model["dlogits"], ref["dlogits"],
            f"{name} dlogits", ce_dlogits_floor(logits, ref, dloss))
    return _finish(out, name, do_assert), ref, model


def adamw_check(got, p, m, v, g, h, name="", do_assert=True):
    """p, m, v of one step against fp64, every element."""
    ref = adamw_fp64(p, m, v, g, h)
    bounds = adamw_bounds(ref, p, m, v, h)
    out = {}
    for t in ("p", "m", "v"):
        assert got[t].dtype == torch.float32
        err = (got[t].double() - ref[t]).abs()
        n_bad = int((err > bounds[t]).sum())
        ratio = torch.where(bounds[t] > 0, err / bounds[t].clamp_min(1e-300),
                            torch.where(err > 0, torch.full_like(err, math.inf),
                                        torch.zeros_like(err)))
        worst = ratio.max().item() if ratio.numel() else 0.0
        out[t] = (n_bad == 0, worst, n_bad)
    print(f"adamw-check {name}: worst err/bound " + ", ".join(
        f"{t} {out[t][1]:.3f}" for t in ("p", "m", "v")) + " | " +
        ("ok" if all(o[0] for o in out.values()) else "FAIL"))
    return _finish(out, name, do_assert), ref
