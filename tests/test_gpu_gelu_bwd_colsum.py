"""_C.gelu_bwd_colsum (csrc/gelu.hip): exact-erf GELU backward with the
column sums of its bf16 result (the fc1 bias gradient) in one pass."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None

SHAPES = [(1, 8), (5, 64), (257, 2048), (1024, 20480)]

# zero crossing of the derivative (~ -0.75), erf saturation, exp underflow
SPECIAL = [0.0, 0.75, -0.75, 10.0, -10.0, 40.0, -40.0]


def _dev():
    return torch.device("cuda", 0)


def _inputs(rows, hid, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(rows, hid, generator=g) * 2.0
    dy = torch.randn(rows, hid, generator=g)
    flat = x.view(-1)
    # every 5th element takes one of the special values in turn
    idx = torch.arange(0, flat.numel(), 5)
    flat[idx] = torch.tensor(SPECIAL)[torch.arange(idx.numel()) % len(SPECIAL)]
    return (dy.to(_dev(), torch.bfloat16), x.to(_dev(), torch.bfloat16))


@pytest.mark.parametrize("rows,hid", SHAPES)
def test_dx_and_colsum(rows, hid):
    dy, x = _inputs(rows, hid)
    dx, colsum = EXT.gelu_bwd_colsum(dy, x)
    assert dx.shape == dy.shape and dx.dtype == torch.bfloat16
    assert colsum.shape == (hid,) and colsum.dtype == torch.bfloat16

    # dx against torch's own kernel on the same tensors: both round an
    # fp32 value to bf16 and the two fp32 values differ by a few fp32
    # ulps, so the results differ by at most one bf16 ulp (2^-7
    # relative); the absolute term covers the cancellation at the zero
    # crossing of the derivative
    ref = torch.ops.aten.gelu_backward(dy, x, approximate="none")
    err = (dx.double() - ref.double()).abs()
    bound = 2.0 ** -7 * ref.double().abs() + 2.0 ** -14 * dy.double().abs().max()
    print(f"dx: max err {err.max().item():.3e}, mismatching elements "
          f"{int((dx != ref).sum())}/{dx.numel()}")
    assert bool((err <= bound).all()), (err - bound).max().item()

    # colsum against the fp64 column sum of OUR dx: one bf16 rounding
    # plus the worst-case fp32 accumulation error over `rows` terms
    dx64 = dx.double()
    cref = dx64.sum(0)
    cerr = (colsum.double() - cref).abs()
    cbound = 2.0 ** -7 * cref.abs() + rows * 2.0 ** -24 * dx64.abs().sum(0)
    print(f"colsum: max err {cerr.max().item():.3e}, min slack "
          f"{(cbound - cerr).min().item():.3e}")
    assert bool((cerr <= cbound).all()), (cerr - cbound).max().item()


def test_leading_dims_flatten():
    """[B, T, hid] input: rows are all leading dims."""
    dy, x = _inputs(6, 64, seed=1)
    dx2, c2 = EXT.gelu_bwd_colsum(dy, x)
    dx3, c3 = EXT.gelu_bwd_colsum(dy.view(2, 3, 64), x.view(2, 3, 64))
    assert dx3.shape == (2, 3, 64)
    assert torch.equal(dx3.view(6, 64), dx2) and torch.equal(c3, c2)


def test_non_finite_inputs_propagate():
    dy, x = _inputs(5, 64, seed=2)
    x[1, 3] = float("nan")
    x[2, 9] = float("inf")     # inf * exp(-inf) = inf * 0
    dy[3, 17] = float("inf")
    dy[4, 40] = float("nan")
    dx, colsum = EXT.gelu_bwd_colsum(dy, x)
    ref = torch.ops.aten.gelu_backward(dy, x, approximate="none")
    assert torch.equal(torch.isnan(dx), torch.isnan(ref))
    assert torch.equal(torch.isinf(dx), torch.isinf(ref))
    for col in (3, 9, 17, 40):
        assert not torch.isfinite(dx[:, col].float()).all()
        assert not torch.isfinite(colsum[col].float())
    finite_cols = torch.isfinite(dx.float()).all(0)
    assert torch.isfinite(colsum.float()[finite_cols]).all()


def test_hid_not_multiple_of_8_refused():
    dy = torch.randn(4, 100, device=_dev(), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        EXT.gelu_bwd_colsum(dy, torch.randn_like(dy))
