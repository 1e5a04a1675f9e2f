"""Single-pass LayerNorm backward (csrc/layernorm.hip
ln_bwd_fused_kernel): dx and the dgamma/dbeta partials from one read of
dy and x, at the shapes where a block-walks-many-rows / thread-owns-
columns structure can go wrong.  Forward and backward against the fp32
torch composition with the tolerances of tests/test_gpu_kernels.py, and
dgamma/dbeta additionally against an fp64 reference computed from the
same bf16 inputs."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-6

SHAPES = [
    (1, 1, 64),      # one row, 8 vectors: most threads idle, rows < blocks
    (4, 7, 64),
    (3, 5, 5120),    # 2.5 vectors per thread, 15 rows
    (2, 3, 8192),    # largest fused instantiation (4 vectors per thread)
    (2, 3, 8200),    # beyond it: the two-kernel path
    (1037, 1024),    # rows not a multiple of the grid
]


def _dev():
    return torch.device("cuda", 0)


def _dwdb_fp64(dy, x):
    """fp64 dgamma/dbeta from bf16 dy and the bf16 normalized input x,
    with per-column error bounds for the kernel's arithmetic.

    The kernel sums n fp32 terms per column (worst-case accumulation
    error n * 2^-24 * sum|term|) and rounds once to bf16 (2^-8 relative).
    Its xhat comes from fp32 statistics accumulated over D elements:
    mean and rstd each carry at most ~2 D 2^-24 relative error for data
    whose |mean| does not exceed its std (randn here, so the variance
    subtraction does not amplify), i.e. |dxhat| <= 4 D 2^-24 (|xhat| + 1).
    """
    d = x.shape[-1]
    dy64 = dy.reshape(-1, d).double()
    x64 = x.reshape(-1, d).double()
    n = x64.shape[0]
    mean = x64.mean(1, keepdim=True)
    var = x64.var(1, unbiased=False, keepdim=True)
    xhat = (x64 - mean) / torch.sqrt(var + EPS)
    dw = (dy64 * xhat).sum(0)
    db = dy64.sum(0)
    u = 2.0 ** -24
    dw_tol = (2.0 ** -8) * dw.abs() + (n + 4 * d) * u * (
        dy64.abs() * (xhat.abs() + 1)).sum(0)
    db_tol = (2.0 ** -8) * db.abs() + n * u * dy64.abs().sum(0)
    return dw, db, dw_tol, db_tol


def _check_dwdb(w_grad, b_grad, dy, x_norm_in):
    dw, db, dw_tol, db_tol = _dwdb_fp64(dy, x_norm_in)
    ew = (w_grad.double() - dw).abs()
    eb = (b_grad.double() - db).abs()
    print(f"dw: max err {ew.max().item():.3e} (min slack "
          f"{(dw_tol - ew).min().item():.3e}); db: max err "
          f"{eb.max().item():.3e} (min slack {(db_tol - eb).min().item():.3e})")
    assert bool((ew <= dw_tol).all()), (ew - dw_tol).max().item()
    assert bool((eb <= db_tol).all()), (eb - db_tol).max().item()


@pytest.mark.parametrize("shape", SHAPES)
def test_layer_norm_fused_bwd(shape):
    from vit_10b_fsdp_example_amd.ops import layer_norm

    torch.manual_seed(0)
    d = shape[-1]
    x = torch.randn(*shape, device=_dev(), dtype=torch.bfloat16)
    w = torch.randn(d, device=_dev(), dtype=torch.bfloat16)
    b = torch.randn(d, device=_dev(), dtype=torch.bfloat16)
    for t in (x, w, b):
        t.requires_grad_(True)
    y = layer_norm(x, w, b, EPS)
    dy = torch.randn_like(y)
    y.backward(dy)

    xf = x.detach().float().requires_grad_(True)
    wf = w.detach().float().requires_grad_(True)
    bf = b.detach().float().requires_grad_(True)
    yf = torch.nn.functional.layer_norm(xf, (d,), wf, bf, EPS)
    yf.backward(dy.float())

    n_rows = int(np.prod(shape[:-1]))
    np.testing.assert_allclose(y.detach().float().cpu(), yf.detach().cpu(),
                               rtol=0.05, atol=0.03)
    np.testing.assert_allclose(x.grad.float().cpu(), xf.grad.cpu(),
                               rtol=0.1, atol=0.05)
    np.testing.assert_allclose(w.grad.float().cpu(), wf.grad.cpu(), rtol=0.05,
                               atol=0.02 * max(1.0, n_rows ** 0.5))
    np.testing.assert_allclose(b.grad.float().cpu(), bf.grad.cpu(), rtol=0.05,
                               atol=0.02 * max(1.0, n_rows ** 0.5))
    _check_dwdb(w.grad, b.grad, dy, x.detach())


@pytest.mark.parametrize("shape", SHAPES)
def test_fused_add_layer_norm_fused_bwd(shape):
    from vit_10b_fsdp_example_amd.ops import fused_add_layer_norm

    torch.manual_seed(4)
    d = shape[-1]
    x = torch.randn(*shape, device=_dev(), dtype=torch.bfloat16)
    r = torch.randn_like(x)
    w = torch.randn(d, device=_dev(), dtype=torch.bfloat16)
    b = torch.randn(d, device=_dev(), dtype=torch.bfloat16)
    for t in (x, r, w, b):
        t.requires_grad_(True)
    s, y = fused_add_layer_norm(x, r, w, b, EPS)
    ds = torch.randn_like(s)
    dy = torch.randn_like(y)
    torch.autograd.backward([s, y], [ds, dy])

    xf = x.detach().float().requires_grad_(True)
    rf = r.detach().float().requires_grad_(True)
    wf = w.detach().float().requires_grad_(True)
    bf = b.detach().float().requires_grad_(True)
    sf = xf + rf
    yf = torch.nn.functional.layer_norm(sf, (d,), wf, bf, EPS)
    torch.autograd.backward([sf, yf], [ds.float(), dy.float()])

    n_rows = int(np.prod(shape[:-1]))
    np.testing.assert_allclose(s.detach().float().cpu(), sf.detach().cpu(),
                               rtol=0.05, atol=0.03)
    np.testing.assert_allclose(y.detach().float().cpu(), yf.detach().cpu(),
                               rtol=0.05, atol=0.05)
    np.testing.assert_allclose(x.grad.float().cpu(), xf.grad.cpu(),
                               rtol=0.1, atol=0.1)
    np.testing.assert_allclose(r.grad.float().cpu(), rf.grad.cpu(),
                               rtol=0.1, atol=0.1)
    # the two input gradients are the same values in distinct buffers
    assert torch.equal(x.grad, r.grad)
    assert x.grad.data_ptr() != r.grad.data_ptr()
    np.testing.assert_allclose(w.grad.float().cpu(), wf.grad.cpu(), rtol=0.05,
                               atol=0.02 * max(1.0, n_rows ** 0.5))
    np.testing.assert_allclose(b.grad.float().cpu(), bf.grad.cpu(), rtol=0.05,
                               atol=0.02 * max(1.0, n_rows ** 0.5))
    # the kernel normalizes its own bf16-rounded sum
    _check_dwdb(w.grad, b.grad, dy, s.detach())
