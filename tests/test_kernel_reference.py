"""CPU tests of the row-wise / optimizer checker (tests/kernel_reference.py):
the fp64 references are sound, the rounding models stay inside every
bound on every shape and family of the GPU files, the measured constants
cover the emulation they were measured from, the families stress what
they claim, and every deliberately wrong variant is rejected in every
family where its defect is active.  Which of the variants the fixed
tolerances of test_gpu_kernels.py accept is printed (run with -s), never
asserted: it is the record of the gap."""

import contextlib
import importlib
import io

import pytest
import torch

from tests import kernel_reference as kr
from tests.fmha_reference import MARGIN

_U = 2.0 ** -24


def _quiet(fn, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kw)


def _ln_args(inp, form):
    x, res, w, b, dy, dsum = inp
    add = form == "add"
    return (x, w, b, dy, dsum if add else None, res if add else None)


# --------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------

def _ln_families(rows):
    return [f for f in kr.LN_FAMILIES if f != "special" or rows >= 3]


_STAT_WORST = {}


@pytest.mark.parametrize("rows,d", kr.LN_CASES)
def test_ln_model_inside_every_bound_at_gpu_shapes(rows, d):
    """Every (rows, D, family, form) of the GPU file: the rounding model
    in the kernels' block order against fp64 under the same check the
    kernel gets (statistics bounds, per-row model-relative check against
    the model in torch's order, floors), the family's stress assertion,
    and the figures the statistics constants were measured from."""
    for family in _ln_families(rows):
        inp = kr.ln_make_inputs(family, rows, d, kr.LN_SEED)
        for form in ("plain", "add"):
            got = kr.ln_model(*_ln_args(inp, form), order="block")
            name = f"model/{form}/{family}/{rows}x{d}"
            res, ref, model = _quiet(kr.ln_check, got, inp, form, name)
            assert res["y"][1] < 1.25 and res["y"][2] < 1.25, res["y"]
            assert res["dx"][2] < 1.25, res["dx"]
            xs = model["sum"].double()
            kr.ln_assert_family(family, xs, rows)
            mean = xs.mean(-1)
            var = ((xs - mean[:, None]) ** 2).mean(-1)
            ms = var + mean * mean
            live = ms > 0
            for order in kr.SUM_ORDERS:
                m32, v32, _ = kr.ln_stats_emulated(model["sum"], order=order)
                rv = ((v32[:, 0].double() - var).abs() / (_U * ms))[live]
                rm = ((m32[:, 0].double() - mean).abs()
                      / (_U * ms.sqrt()))[live]
                key = (family, rows, d, form, order)
                _STAT_WORST[key] = (rv.max().item() if rv.numel() else 0.0,
                                    rm.max().item() if rm.numel() else 0.0)
                # inside the bound with the 8x headroom, every row
                assert _STAT_WORST[key][0] <= kr.C_VAR
                assert _STAT_WORST[key][1] <= kr.C_MEAN


def test_stat_constants_cover_the_emulation():
    """C_VAR and C_MEAN are 8 x the worst the fp32 emulation reaches over
    the GPU file's own shapes, families and seed, in all three orders."""
    if len(_STAT_WORST) < len(kr.LN_CASES):  # run alone: fill the table
        for rows, d in kr.LN_CASES:
            test_ln_model_inside_every_bound_at_gpu_shapes(rows, d)
    wv = max(_STAT_WORST, key=lambda k: _STAT_WORST[k][0])
    wm = max(_STAT_WORST, key=lambda k: _STAT_WORST[k][1])
    print(f"fp32 one-pass statistics, worst over {len(_STAT_WORST)} cases: "
          f"var {_STAT_WORST[wv][0]:.3f} at {wv}, mean "
          f"{_STAT_WORST[wm][1]:.3f} at {wm}")
    assert _STAT_WORST[wv][0] <= kr.STAT_WORST_VAR
    assert _STAT_WORST[wm][1] <= kr.STAT_WORST_MEAN
    # recorded figures are the measurement, not a loose cap on it
    assert _STAT_WORST[wv][0] > 0.9 * kr.STAT_WORST_VAR
    assert _STAT_WORST[wm][1] > 0.9 * kr.STAT_WORST_MEAN
    assert kr.C_VAR == 8 * kr.STAT_WORST_VAR
    assert kr.C_MEAN == 8 * kr.STAT_WORST_MEAN


def test_stat_bound_has_teeth_where_d_times_u_has_none():
    """At D = 8192 and mean = 16 std a worst-case D * u accumulation term
    allows ~12 % on the variance; the bound used here allows well under
    1 %."""
    x = kr.ln_make_inputs("offset", 3, 8192, 0)[0].double()
    st = kr.ln_stat_bounds(x)
    assert float((8192 * _U * (st["var"] + st["mean"] ** 2) / st["var"]).min()
                 ) > 0.1
    assert float((st["dvar"] / st["var"]).max()) < 1e-3
    assert float((st["drstd"] / st["rstd"]).max()) < 5e-4


def test_ln_fp64_equals_autograd():
    x, res, w, b, dy, dsum = (t.double() for t in
                              kr.ln_make_inputs("randn", 5, 64, 3))
    ref = kr.ln_fp64(x, w, b, dy, dsum, res, s_bf16=x + res)
    for t in (x, res):
        t.requires_grad_(True)
    s = x + res
    y = torch.nn.functional.layer_norm(s, (64,), w, b, kr.LN_EPS)
    torch.autograd.backward([s, y], [dsum, dy])
    assert float((ref["y"] - y.detach()).abs().max()) < 1e-12
    assert float((ref["dx"] - x.grad).abs().max()) < 1e-11
    assert torch.equal(x.grad, res.grad)


def _ln_defect_active(defect, family, form, d):
    """Where a defect changes the result by more than the arithmetic
    resolves.  The exceptions, all derived:

    * unbiased_var / eps_1e-5 in `offset` (mean = 16 std): fp32 cannot
      tell.  The one-pass variance is only good to C_VAR u (1 + 256) =
      6.6e-4 there, rstd to half of it; the unbiased divisor moves rstd
      by 1/(2D) (below that from D = 2048 up), eps by 4.5e-6.
    * add_no_dsum exists in the ADD form only.
    * the two that drop or misplace the last vector need a second one."""
    if d < kr.LN_DEFECTS[defect]:
        return False
    if defect == "add_no_dsum":
        return form == "add"
    if family == "offset":
        if defect == "eps_1e-5":
            return False
        if defect == "unbiased_var":
            return 1.0 / (2 * d) > 0.5 * kr.C_VAR * _U * 257 * 2
    return True


_LN_OLD = {}


@pytest.mark.parametrize("defect", sorted(kr.LN_DEFECTS))
@pytest.mark.parametrize("d", [64, 5120, 8192])
def test_ln_defect_is_rejected(defect, d):
    rows = 16
    for family in kr.LN_FAMILIES:
        inp = kr.ln_make_inputs(family, rows, d, 7)
        for form in ("plain", "add"):
            if not _ln_defect_active(defect, family, form, d):
                continue
            got = kr.ln_model(*_ln_args(inp, form), order="block",
                              defect=defect)
            name = f"{defect}/{form}/{family}/D{d}"
            res, ref, _ = _quiet(kr.ln_check, got, inp, form, name, False)
            rejected = [t for t, r in res.items() if not r[0]]
            old = kr.ln_old_tolerance_passes(got, ref)
            _LN_OLD[(defect, d, family, form)] = all(old.values())
            print(f"defect {name}: new check rejects "
                  f"{rejected or 'NOTHING'}; old tolerances pass "
                  f"{[t for t in old if old[t]] or 'nothing'}"
                  f"{' (ALL: defect invisible)' if all(old.values()) else ''}")
            assert rejected, (name, res)
            with pytest.raises(AssertionError):
                _quiet(kr.ln_check, got, inp, form, name)


def test_ln_old_tolerances_accept_what_the_issue_names():
    """The record of the gap, re-derived (plain form, `randn`): the fixed
    tolerances accept an unbiased variance and a 10x eps at every D, and
    a dx without mean(g) at D = 5120 and 8192."""
    for d in (64, 5120, 8192):
        inp = kr.ln_make_inputs("randn", 16, d, 7)
        for defect, tensor in (("unbiased_var", "y"), ("eps_1e-5", "y"),
                               ("dx_no_mean_g", "dx")):
            got = kr.ln_model(*_ln_args(inp, "plain"), defect=defect)
            ref = kr.ln_fp64(*_ln_args(inp, "plain"))
            old = kr.ln_old_tolerance_passes(got, ref)
            print(f"old tolerances, {defect} D={d}: {old}")
            if defect != "dx_no_mean_g" or d >= 5120:
                assert old[tensor], (defect, d)


def test_zero_row_is_bias_bit_for_bit_and_const_row_has_a_floor():
    inp = kr.ln_make_inputs("special", 16, 5120, 1)
    x, res, w, b, dy, dsum = inp
    for order in kr.SUM_ORDERS:
        got = kr.ln_model(x, w, b, order=order)
        assert torch.equal(got["y"][0], b.float())
    fl = kr.ln_floors(x.double(), w, b, dy)
    # floors exist on the two degenerate rows only, and the constant
    # row's is far below the output's own scale
    assert int((fl["y"] > 0).sum()) == 2 and int((fl["dx"] > 0).sum()) == 2
    assert 0 < float(fl["y"][1]) < 0.05


def test_layer_norm_fp32_weight_routes_to_the_framework_op(monkeypatch):
    """bf16 x with an fp32 gamma must never reach the bf16-only kernel
    (it would read the fp32 bits as bf16): even where the HIP path is
    available it takes F.layer_norm."""
    ln_mod = importlib.import_module("vit_10b_fsdp_example_amd.ops.layernorm")

    class _NoKernel:
        def __getattr__(self, name):
            return lambda *a, **k: pytest.fail(f"{name} reached the kernel")

    monkeypatch.setattr(ln_mod, "use_hip", lambda *ts: True)
    monkeypatch.setattr(ln_mod, "ext", lambda: _NoKernel())
    torch.manual_seed(0)
    x = torch.randn(3, 16).to(torch.bfloat16)
    r = torch.randn(3, 16).to(torch.bfloat16)
    w32, b32 = torch.randn(16), torch.randn(16)
    wb, bb = w32.to(torch.bfloat16), b32.to(torch.bfloat16)
    for w, b in ((w32, b32), (w32, bb), (wb, b32)):
        assert not ln_mod._kernel_operands(x, w, b)
    assert ln_mod._kernel_operands(x, wb, bb)
    assert not ln_mod._kernel_operands(x.float(), w32, b32)
    assert not ln_mod._kernel_operands(x[:, :12], wb[:12], bb[:12])
    xf = x.float()
    want = torch.nn.functional.layer_norm(xf, (16,), w32, b32, 1e-6)
    assert torch.equal(ln_mod.layer_norm(xf, w32, b32), want)
    s, y = ln_mod.fused_add_layer_norm(xf, r.float(), w32, b32)
    assert torch.equal(s, xf + r.float())
    # mixed: stays off the kernel (the stub fails the test otherwise)
    try:
        ln_mod.layer_norm(x, w32, b32)
    except RuntimeError:
        pass  # a framework build without mixed-dtype LayerNorm may refuse


# --------------------------------------------------------------------------
# cross-entropy
# --------------------------------------------------------------------------

@pytest.mark.parametrize("c", kr.CE_CLASSES)
def test_ce_model_inside_every_bound_at_gpu_shapes(c):
    for n in kr.CE_ROWS:
        for family in kr.CE_FAMILIES:
            for dloss in kr.CE_DLOSS:
                logits, target = kr.ce_make_inputs(family, n, c, n)
                assert int(target.min()) >= 0 and int(target.max()) < c
                if n > 1:
                    assert 0 in target.tolist() and c - 1 in target.tolist()
                got = kr.ce_model(logits, target, dloss)
                name = f"model/{family}/{n}x{c}/dloss{dloss}"
                res, ref, _ = _quiet(kr.ce_check, got, logits, target, dloss,
                                     name)
                kr.ce_assert_family(family, logits, target, ref)
                assert res["dlogits"][1] in (0.0, 1.0)


def test_ce_single_row_targets_cover_both_ends():
    assert int(kr.ce_make_inputs("randn", 1, 257, 0)[1]) == 256
    assert int(kr.ce_make_inputs("randn", 1, 257, 1)[1]) == 0


def test_ce_fp64_equals_autograd():
    logits, target = kr.ce_make_inputs("randn", 7, 33, 5)
    ref = kr.ce_fp64(logits, target, 0.37)
    l = logits.double().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(l, target)
    loss.backward(torch.tensor(0.37, dtype=torch.float64))
    assert abs(float(loss.detach()) - float(ref["loss"])) < 1e-13
    assert float((l.grad - ref["dlogits"]).abs().max()) < 1e-15


def _ce_defect_active(defect, family, n, c, dloss):
    """* lse_first_full_blocks needs a partial last block (C > 256,
      C % 256 != 0).  With a +30 peak the rest of the row is e^-30 of the
      sum, below fp32: active only if the peak sits in the dropped tail,
      which the target C - 1 of the last row guarantees for
      `peaked_target` (n > 1) and nothing guarantees for `peaked_other`.
    * grad_n_plus_1 moves the gradient by 1/(N+1).  `peaked_target`'s
      gradient is zero to fp32 resolution (that is the family's point).
    * target_shifted needs a second class.
    * dloss_ignored needs dloss != 1."""
    if defect == "lse_first_full_blocks":
        if c < 256 or c % 256 == 0:
            return False
        if family == "peaked_target":
            return n > 1
        return family != "peaked_other"
    if defect == "grad_n_plus_1":
        return family != "peaked_target" and c > 1
    if defect == "target_shifted":
        return c > 1
    if defect == "dloss_ignored":
        return dloss != 1.0 and family != "peaked_target" and c > 1
    return True


@pytest.mark.parametrize("defect", kr.CE_DEFECTS)
def test_ce_defect_is_rejected(defect):
    for n, c in ((128, 1000), (3, 257), (128, 4099), (3, 8)):
        for family in kr.CE_FAMILIES:
            for dloss in kr.CE_DLOSS:
                if not _ce_defect_active(defect, family, n, c, dloss):
                    continue
                logits, target = kr.ce_make_inputs(family, n, c, 9)
                got = kr.ce_model(logits, target, dloss, defect=defect)
                name = f"{defect}/{family}/{n}x{c}/dloss{dloss}"
                res, ref, _ = _quiet(kr.ce_check, got, logits, target, dloss,
                                     name, False)
                rejected = [t for t, r in res.items() if not r[0]]
                old = kr.ce_old_tolerance_passes(got, ref)
                print(f"defect {name}: new check rejects "
                      f"{rejected or 'NOTHING'}; old tolerances pass "
                      f"{[t for t in old if old[t]] or 'nothing'}"
                      f"{' (ALL: defect invisible)' if all(old.values()) else ''}")
                assert rejected, (name, res)
                with pytest.raises(AssertionError):
                    _quiet(kr.ce_check, got, logits, target, dloss, name)


def test_ce_old_tolerances_accept_what_the_issue_names():
    """128 x 1000 `randn`, dloss = 1: a gradient scaled by 128/129 and an
    lse off by 0.04 both pass the fixed tolerances."""
    logits, target = kr.ce_make_inputs("randn", 128, 1000, 9)
    ref = kr.ce_fp64(logits, target)
    for defect in ("grad_n_plus_1", "lse_off_0.04"):
        old = kr.ce_old_tolerance_passes(
            kr.ce_model(logits, target, defect=defect), ref)
        print(f"old tolerances, {defect}: {old}")
        assert old["dlogits"]
    assert old["loss"] is False  # 0.04 > 0.02: only the loss check sees it


# --------------------------------------------------------------------------
# AdamW
# --------------------------------------------------------------------------

def _adamw_cases():
    for t, state in ((1, "zeros"), (1, "random"), (1000, "random")):
        for wd in (0.0, 0.1):
            for prescale, gs in ((1.0, None), (0.125, 0.37)):
                yield t, state, wd, prescale, gs


@pytest.mark.parametrize("n", kr.ADAMW_SIZES)
def test_adamw_model_inside_every_bound(n):
    for t, state, wd, prescale, gs in _adamw_cases():
        for dt in (torch.float32, torch.bfloat16):
            p, m, v, g = kr.adamw_make_inputs(n, n + t, state, dt, extra=3)
            if state == "random":
                assert bool((m != 0).all()) and bool((v >= 0).all())
            h = kr.adamw_hyper(t, wd, prescale=prescale, grad_scale=gs)
            got = kr.adamw_model(p, m, v, g, h)
            _quiet(kr.adamw_check, got, p, m, v, g, h,
                   f"model/n{n}/t{t}/{state}/wd{wd}/ps{prescale}")


def _adamw_defect_active(defect, t, state, wd, prescale):
    """* decay_after_update differs by update * lr * wd: needs wd != 0.
    * prescale_m_only needs prescale != 1.
    * bias_prev_step has no previous step at t = 1.
    * one_minus_beta2_fp32 puts 1.3e-5 (216 u) on the (1 - beta2) g^2 term
      only: all of v at a real first step (v = 0).  Once v holds history
      of the gradient's own size the term is 1e-3 of v and the defect
      sinks below 3u; the `random` state draws v and g independently per
      element, so among 1e5 elements some have v far below g^2 and it
      shows there too.
    * eps_inside_sqrt is visible where sqrt(v) is not far above eps: the
      inputs span magnitudes down to 1e-4 for that."""
    if defect == "decay_after_update":
        return wd != 0.0
    if defect == "prescale_m_only":
        return prescale != 1.0
    if defect == "bias_prev_step":
        return t > 1
    return True


@pytest.mark.parametrize("defect", kr.ADAMW_DEFECTS)
def test_adamw_defect_is_rejected(defect):
    n = 100003
    for t, state, wd, prescale, gs in _adamw_cases():
        if not _adamw_defect_active(defect, t, state, wd, prescale):
            continue
        p, m, v, g = kr.adamw_make_inputs(n, 11, state)
        h = kr.adamw_hyper(t, wd, prescale=prescale, grad_scale=gs)
        got = kr.adamw_model(p, m, v, g, h, defect)
        name = f"{defect}/t{t}/{state}/wd{wd}/ps{prescale}"
        res, ref = _quiet(kr.adamw_check, got, p, m, v, g, h, name, False)
        rejected = [k for k, r in res.items() if not r[0]]
        old = kr.adamw_old_tolerance_passes(got, ref)
        print(f"defect {name}: new check rejects {rejected or 'NOTHING'}; "
              f"old tolerance on p {'passes' if old else 'fails'}")
        assert rejected, (name, res)


def test_one_minus_beta2_in_fp32_is_what_the_bound_flags():
    """1.f - 0.999f is 1.29e-5 relative below 1 - 0.999: at t = 1 all of v
    carries it, ~20 x the 10u the arithmetic allows."""
    import numpy as np

    rel = 1.0 - float(np.float32(1.0) - np.float32(0.999)) / (1.0 - 0.999)
    assert 1.2e-5 < rel < 1.4e-5
    p, m, v, g = kr.adamw_make_inputs(1023, 2, "zeros")
    h = kr.adamw_hyper(1)
    res, _ = _quiet(kr.adamw_check, kr.adamw_model(
        p, m, v, g, h, "one_minus_beta2_fp32"), p, m, v, g, h, "", False)
    assert not res["v"][0] and res["v"][1] > 10
    assert res["m"][0]


# --------------------------------------------------------------------------
# multi-tensor helpers
# --------------------------------------------------------------------------

def test_small_integer_sums_are_exact_in_fp32():
    for dt in (torch.float32, torch.bfloat16):
        ts = [kr.small_int_tensor(n, n, dt) for n in kr.mt_sizes(65, 1000)]
        exact = sum(int(t.double().pow(2).sum()) for t in ts)
        assert exact < 2 ** 24
        assert float(sum(t.float().pow(2).sum() for t in ts)) == exact
        # one dropped element changes the integer
        assert exact - int(ts[3][5].double() ** 2 + 0.5) <= exact
        total, bound = kr.sqnorm_bound(ts)
        assert total == exact and bound > 0


def test_scale_reference_rounds_once():
    x = torch.randn(1001).to(torch.bfloat16)
    got = kr.scale_reference(x, 1.0 / 3.0)
    assert got.dtype == torch.bfloat16
    import numpy as np

    want = (x.float() * float(np.float32(1.0 / 3.0))).to(torch.bfloat16)
    assert torch.equal(got, want)
    x32 = torch.randn(1001)
    assert torch.equal(kr.scale_reference(x32, 0.5), x32 * 0.5)


def test_margin_is_the_projects():
    assert MARGIN == 2.0
