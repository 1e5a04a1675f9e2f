"""Fused AdamW, mt_sqnorm and mt_scale (csrc/adamw.hip) against fp64 with
per-element bounds written out from the arithmetic
(tests/kernel_reference.py), at the sizes where the vector body, the
scalar tail and the 32-tensor table wrap: tails 0..7, tensors shorter
than one vector, an empty tensor inside a list, and lists of 1, 32, 33
and 65 tensors (the second and third launch of the ``base += kMaxTensors``
loop).  The sums and the scaling are also checked EXACTLY where an
order-independent exact answer exists."""

import numpy as np
import pytest
import torch

from tests import kernel_reference as kr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None


def _dev():
    return torch.device("cuda", 0)


# --------------------------------------------------------------------------
# fused_adamw, one step
# --------------------------------------------------------------------------

def _step_and_check(sizes, seed, t, state, wd, prescale, gs, grad_dtype,
                    mirror_at, name, extra=3):
    """One EXT.fused_adamw call over tensors of ``sizes``; every tensor's
    p, m, v against fp64, every element; mirrors (where ``mirror_at(i)``)
    bit-exact against the returned p."""
    h = kr.adamw_hyper(t, wd, prescale=prescale, grad_scale=gs)
    before, ps, ms, vs, gs_, mirrors = [], [], [], [], [], []
    for i, n in enumerate(sizes):
        p, m, v, g = kr.adamw_make_inputs(n, seed + i, state, grad_dtype,
                                          extra, _dev())
        before.append((p.clone(), m.clone(), v.clone(), g.clone()))
        ps.append(p), ms.append(m), vs.append(v), gs_.append(g)
        mirrors.append(torch.full((n,), 7.0, device=_dev(),
                                  dtype=torch.bfloat16)
                       if mirror_at(i) else None)
    gscale = None if gs is None else torch.tensor(gs, device=_dev())
    EXT.fused_adamw(ps, gs_, ms, vs,
                    mirrors if any(x is not None for x in mirrors) else [],
                    h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"],
                    h["bias_c1"], h["bias_c2"], gscale, prescale)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, n in enumerate(sizes):
        p0, m0, v0, g0 = before[i]
        assert torch.equal(gs_[i], g0), "the gradient was written"
        got = {"p": ps[i], "m": ms[i], "v": vs[i]}
        res, _ = kr.adamw_check(got, p0, m0, v0, g0, h, f"{name}[{i}] n={n}")
        for k in worst:
            worst[k] = max(worst[k], res[k][1])
        if mirrors[i] is not None:
            assert torch.equal(mirrors[i], ps[i].to(torch.bfloat16)), (
                f"{name}[{i}]: mirror != bf16(p)")
    print(f"adamw-worst {name}: " + ", ".join(
        f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


# sizes 1..8 and 1023 walk every tail of the 4-wide body; the empty
# tensor sits inside the list; 100003 takes more than one grid stride
_SIZES = kr.ADAMW_SIZES[:5] + (0,) + kr.ADAMW_SIZES[5:]


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16],
                         ids=["g32", "gbf16"])
@pytest.mark.parametrize("mirrors", [False, True], ids=["nomir", "mir"])
@pytest.mark.parametrize("prescale,gs", [(1.0, None), (0.125, 0.37)],
                         ids=["plain", "scaled"])
@pytest.mark.parametrize("t,state", [(1, "zeros"), (1, "random"),
                                     (1000, "random")])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_fused_adamw_one_step_vs_fp64(wd, t, state, prescale, gs, mirrors,
                                      grad_dtype):
    assert 0 in _SIZES and set(kr.ADAMW_SIZES) <= set(_SIZES)
    _step_and_check(_SIZES, 100 * t, t, state, wd, prescale, gs, grad_dtype,
                    (lambda i: True) if mirrors else (lambda i: False),
                    f"adamw/t{t}/{state}/wd{wd}/ps{prescale}/"
                    f"{'mir' if mirrors else 'nomir'}/"
                    f"{str(grad_dtype)[6:]}")


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16],
                         ids=["g32", "gbf16"])
@pytest.mark.parametrize("count", kr.MT_LIST_LENGTHS)
def test_fused_adamw_list_lengths(count, grad_dtype):
    """32 fills one table, 33 and 65 need a second and a third launch.
    Sizes 0, 1, 2, ...: every tail again, per table slot; a mirror on
    every third tensor only."""
    _step_and_check(kr.mt_sizes(count, 0), 7, 1000, "random", 0.1, 0.125,
                    0.37, grad_dtype, lambda i: i % 3 == 1,
                    f"adamw-list/{count}/{str(grad_dtype)[6:]}")


def test_fused_adamw_step_three_steps_vs_torch_fp64():
    """FusedAdamW.step over 33 parameters (two launches), three steps,
    against torch.optim.AdamW run in float64 on the same gradients; the
    bound is the one-step bound carried along the fp64 trajectory."""
    from vit_10b_fsdp_example_amd.ops import FusedAdamW

    lr, wd, n_par = 1e-2, 0.1, 33
    gen = torch.Generator().manual_seed(3)
    sizes = kr.mt_sizes(n_par, 1000)
    init = [torch.randn(n, generator=gen) for n in sizes]
    params = [torch.nn.Parameter(t.clone().to(_dev())) for t in init]
    ref_params = [torch.nn.Parameter(t.double().to(_dev())) for t in init]
    opt = FusedAdamW(params, lr=lr, weight_decay=wd)
    ref_opt = torch.optim.AdamW(ref_params, lr=lr, weight_decay=wd)
    state = [(p.detach().double().clone(), torch.zeros_like(p).double(),
              torch.zeros_like(p).double()) for p in params]
    bounds = [None] * n_par
    for t in range(1, 4):
        h = kr.adamw_hyper(t, wd, lr=lr)
        grads = [(torch.randn(n, generator=gen)
                  * 10.0 ** (-2 * torch.rand(n, generator=gen))).to(_dev())
                 for n in sizes]
        for p, rp, g in zip(params, ref_params, grads):
            p.grad, rp.grad = g.clone(), g.double()
        opt.step()
        ref_opt.step()
        worst = 0.0
        for i in range(n_par):
            p64, m64, v64 = state[i]
            ref = kr.adamw_fp64(p64, m64, v64, grads[i], h)
            # the reference is torch.optim.AdamW in fp64; the recurrence
            # here (needed for the bound's terms) must agree with it
            assert float((ref["p"] - ref_params[i].detach()).abs().max()
                         ) < 1e-12
            bounds[i] = kr.adamw_bounds(ref, p64, m64, v64, h, bounds[i])
            state[i] = (ref["p"], ref["m"], ref["v"])
            st = opt.state[params[i]]
            for k, got in (("p", params[i].detach()), ("m", st["exp_avg"]),
                           ("v", st["exp_avg_sq"])):
                want = {"p": ref_params[i].detach(), "m": ref["m"],
                        "v": ref["v"]}[k]
                err = (got.double() - want).abs()
                assert bool((err <= bounds[i][k]).all()), (t, i, k)
                worst = max(worst, (err / bounds[i][k]).max().item())
        print(f"adamw-step t={t}: worst err/bound {worst:.3f}")


def test_fused_adamw_refuses_bad_state():
    n = 64
    h = kr.adamw_hyper(1)
    for which in ("exp_avg", "exp_avg_sq"):
        for label in ("dtype", "non-contiguous", "size", "device"):
            p, m, v, g = kr.adamw_make_inputs(n, 1, device=_dev())
            keep = p.clone()
            bad = m if which == "exp_avg" else v
            if label == "dtype":
                bad = bad.to(torch.bfloat16)
            elif label == "non-contiguous":
                bad = torch.stack([bad, bad], 1)[:, 0]
                assert not bad.is_contiguous()
            elif label == "size":
                bad = bad[:n - 4].clone()
            else:
                bad = bad.cpu()
            ms, vs = ([bad], [v]) if which == "exp_avg" else ([m], [bad])
            # behind a good first entry, so that nothing may be stepped
            # before the whole list is checked
            p0, m0, v0, g0 = kr.adamw_make_inputs(n, 2, device=_dev())
            keep0 = p0.clone()
            with pytest.raises(RuntimeError, match=which):
                EXT.fused_adamw([p0, p], [g0, g], [m0] + ms, [v0] + vs, [],
                                h["lr"], h["beta1"], h["beta2"], h["eps"],
                                h["wd"], h["bias_c1"], h["bias_c2"], None, 1.0)
            assert torch.equal(p, keep) and torch.equal(p0, keep0), (
                which, label, "a refused call stepped a parameter")
    p, m, v, g = kr.adamw_make_inputs(n, 1, device=_dev())
    with pytest.raises(RuntimeError, match="one length"):
        EXT.fused_adamw([p], [g], [m], [], [], h["lr"], h["beta1"],
                        h["beta2"], h["eps"], h["wd"], h["bias_c1"],
                        h["bias_c2"], None, 1.0)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------
# mt_sqnorm / mt_scale
# --------------------------------------------------------------------------

def _dtype_at(i, mix):
    if mix == "mixed":
        return torch.bfloat16 if i % 2 else torch.float32
    return {"f32": torch.float32, "bf16": torch.bfloat16}[mix]


def _int_list(count, mix, big):
    """Small-integer tensors of sizes 0, 1, 2, ... (tails 0..7 of both the
    4-wide fp32 and the 8-wide bf16 body, tensors shorter than a vector,
    one empty), optionally with one of 100003 elements in the middle."""
    sizes = kr.mt_sizes(count, 0)
    if big:
        sizes[count // 2] = 100003
    return [kr.small_int_tensor(n, 31 + i, _dtype_at(i, mix), _dev())
            for i, n in enumerate(sizes)]


@pytest.mark.parametrize("mix", ["f32", "bf16", "mixed"])
@pytest.mark.parametrize("count", kr.MT_LIST_LENGTHS)
def test_mt_sqnorm_small_integers_exact(count, mix):
    for big in (False, True):
        ts = _int_list(count, mix, big)
        exact = sum(int(t.double().pow(2).sum().item()) for t in ts)
        assert exact < 2 ** 24
        got = EXT.multi_tensor_sqnorm(ts)
        assert got.dtype == torch.float32 and got.dim() == 0
        assert float(got) == float(exact), (count, mix, big, float(got), exact)


@pytest.mark.parametrize("n", [3, 4, 5, 9, 1023, 100003])
def test_mt_sqnorm_sees_one_dropped_element(n):
    """What a random-data tolerance cannot: the integer sum moves by
    exactly the square of one element, wherever it sits."""
    for dt in (torch.float32, torch.bfloat16):
        t = kr.small_int_tensor(n, n, dt, _dev())
        t[n - 1] = 2.0
        a = float(EXT.multi_tensor_sqnorm([t]))
        t[n - 1] = 0.0
        assert a - float(EXT.multi_tensor_sqnorm([t])) == 4.0


@pytest.mark.parametrize("mix", ["f32", "bf16", "mixed"])
@pytest.mark.parametrize("count", kr.MT_LIST_LENGTHS)
def test_mt_sqnorm_randn_vs_fp64(count, mix):
    gen = torch.Generator().manual_seed(count)
    sizes = kr.mt_sizes(count, 0)
    sizes[count // 2] = 100003
    ts = [torch.randn(n, generator=gen).to(_dtype_at(i, mix)).to(_dev())
          for i, n in enumerate(sizes)]
    total, bound = kr.sqnorm_bound(ts)
    err = abs(float(EXT.multi_tensor_sqnorm(ts)) - total)
    print(f"sqnorm {count}/{mix}: rel err {err / total:.3e}, bound "
          f"{bound / total:.3e}")
    assert err <= bound


@pytest.mark.parametrize("factor", [1.0 / 3.0, 0.5])
@pytest.mark.parametrize("mode", ["immediate", "device_scalar"])
@pytest.mark.parametrize("mix", ["f32", "bf16", "mixed"])
@pytest.mark.parametrize("count", kr.MT_LIST_LENGTHS)
def test_mt_scale_bit_identical(count, mix, mode, factor):
    gen = torch.Generator().manual_seed(count)
    sizes = kr.mt_sizes(count, 0)
    sizes[count // 2] = 100003
    ts = [torch.randn(n, generator=gen).to(_dtype_at(i, mix)).to(_dev())
          for i, n in enumerate(sizes)]
    want = [kr.scale_reference(t, factor) for t in ts]
    if mode == "immediate":
        EXT.multi_tensor_scale(ts, factor)
    else:
        EXT.multi_tensor_scale_tensor(
            ts, torch.tensor(np.float32(factor), device=_dev()))
    for i, (t, w) in enumerate(zip(ts, want)):
        assert t.dtype == w.dtype
        assert torch.equal(t, w), (i, t.numel())


def test_mt_sqnorm_refuses_empty_list():
    with pytest.raises(RuntimeError, match="empty tensor list"):
        EXT.multi_tensor_sqnorm([])
    # an empty TENSOR is fine
    z = torch.empty(0, device=_dev())
    assert float(EXT.multi_tensor_sqnorm([z])) == 0.0
