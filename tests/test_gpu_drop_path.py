"""csrc/drop_path.hip and ops/drop_path.py on the GPU: the per-sample
mask is the hash reference's at column 0 and the element mask is hidden
dropout's, bit for bit; dropped samples are never read (non-finite
values under them do not leak); the fused values sit inside the
rounding-model bound of an fp64 reference; the backward regenerates both
masks; no mask is stored; a dropped sample makes the block a skip
connection; and training under gradient checkpointing reproduces the
masks in the recompute."""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None

from vit_10b_fsdp_example_amd.ops import (  # noqa: E402
    drop_path, drop_path_add, drop_path_add_reference, drop_path_mask,
    hidden_dropout_mask,
)
from vit_10b_fsdp_example_amd.ops.attention import (  # noqa: E402
    _draw_seed, dropout_mask_reference,
)

# [B, T, C]
SHAPES = [
    (1, 1, 8),         # smallest possible
    (3, 5, 64),        # samples shorter than a chunk
    (2, 257, 2048),    # one full block of vectors; chunk edges in a sample
    (5, 3, 2056),      # 257 vectors, a ragged second block
    (8, 64, 20480),    # MLP width, many column blocks
]
P_PATHS = [0.1, 0.5]
P_ELEMS = [0.0, 0.25]
SEEDS = [0, 1234, 2 ** 31 - 2]


def cases(fn):
    for names, values in (("shape", SHAPES), ("p_path", P_PATHS),
                          ("p_elem", P_ELEMS), ("seed", SEEDS)):
        fn = pytest.mark.parametrize(names, values)(fn)
    return fn


def _dev():
    return torch.device("cuda", 0)


def _elem_seed(seed):
    # a second integer per case, independent of the path seed's value
    return seed // 2 + 77


@functools.lru_cache(maxsize=None)
def _inputs(shape, seed=0):
    """(dy, x, res) bf16 on the GPU.  Shared between tests: never
    modified."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return tuple(
        torch.randn(shape, generator=g).to(_dev(), torch.bfloat16)
        for _ in range(3))


@functools.lru_cache(maxsize=None)
def _elem_mask(seed, rows, cols, p):
    return hidden_dropout_mask(seed, rows, cols, p).to(_dev())


def _keep(shape, p_path, seed, p_elem, elem_seed):
    """(keep_sample [B, 1, 1], keep [B, T, C]) on the GPU."""
    B, T, C = shape
    keep_s = drop_path_mask(seed, B, p_path).to(_dev()).reshape(B, 1, 1)
    keep = keep_s.expand(shape)
    if p_elem > 0.0:
        keep = keep & _elem_mask(elem_seed, B * T, C, p_elem).reshape(shape)
    return keep_s, keep


def _rscale32(p_path, p_elem):
    # the kernel's scale: one division in double, rounded to fp32
    return torch.tensor(1.0 / ((1.0 - p_path) * (1.0 - p_elem)),
                        dtype=torch.float32, device=_dev())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _fwd_expected(x, keep, p_path, p_elem):
    scaled = (x.float() * _rscale32(p_path, p_elem)).bfloat16()
    return torch.where(keep, scaled, torch.zeros_like(scaled))


@cases
def test_drop_path_fwd_bit_exact(shape, p_path, p_elem, seed):
    dy, x, _ = _inputs(shape)
    es = _elem_seed(seed)
    _, keep = _keep(shape, p_path, seed, p_elem, es)
    y = EXT.drop_path_fwd(x, shape[0], p_path, seed, p_elem, es)
    assert y.shape == x.shape and y.dtype == torch.bfloat16
    assert torch.equal(_bits(y), _bits(_fwd_expected(x, keep, p_path, p_elem)))
    # its own adjoint: the same call on dy is the backward
    dx = EXT.drop_path_fwd(dy, shape[0], p_path, seed, p_elem, es)
    assert torch.equal(
        _bits(dx), _bits(_fwd_expected(dy, keep, p_path, p_elem)))


def _check_add(out, x, res, keep, ref, rscale):
    assert out.shape == x.shape and out.dtype == torch.bfloat16
    # a dropped sample, or a dropped element, passes x through bitwise
    assert torch.equal(_bits(out)[~keep], _bits(x)[~keep])
    err = (out.double() - ref).abs()
    # one bf16 rounding plus fp32 arithmetic slack (an FMA contraction
    # may move the last fp32 bit): test_dropout_add_fwd's bound
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -23 * (
        x.double().abs() + res.double().abs() * rscale)
    if bool(keep.any()):
        print(f"max err {err[keep].max().item():.3e}, min slack "
              f"{(bound - err)[keep].min().item():.3e}")
        assert bool((err <= bound)[keep].all()), (
            (err - bound)[keep].max().item())
    else:
        print("nothing kept")


@cases
def test_drop_path_add_fwd(shape, p_path, p_elem, seed):
    _, x, res = _inputs(shape)
    es = _elem_seed(seed)
    _, keep = _keep(shape, p_path, seed, p_elem, es)
    out = EXT.drop_path_add_fwd(x, res, shape[0], p_path, seed, p_elem, es)
    ref = drop_path_add_reference(x, res, shape[0], p_path, seed, p_elem, es)
    _check_add(out, x, res, keep, ref,
               1.0 / ((1.0 - p_path) * (1.0 - p_elem)))


def _seed_with_mask(want):
    for seed in range(4096):
        if drop_path_mask(seed, 2, 0.5).tolist() == want:
            return seed
    raise AssertionError(f"no seed below 4096 gives {want}")


@pytest.mark.parametrize("kept", [False, True])
@pytest.mark.parametrize("p_elem", P_ELEMS)
def test_all_dropped_and_all_kept(kept, p_elem):
    shape, p = (2, 257, 2048), 0.5
    dy, x, res = _inputs(shape)
    seed = _seed_with_mask([kept, kept])
    keep_s, keep = _keep(shape, p, seed, p_elem, 9)
    assert bool(keep_s.all()) == kept and bool(keep_s.any()) == kept
    y = EXT.drop_path_fwd(x, 2, p, seed, p_elem, 9)
    assert torch.equal(_bits(y), _bits(_fwd_expected(x, keep, p, p_elem)))
    if not kept:
        assert bool((_bits(y) == 0).all())
    out = EXT.drop_path_add_fwd(x, res, 2, p, seed, p_elem, 9)
    if not kept:
        assert torch.equal(_bits(out), _bits(x))
    _check_add(out, x, res, keep,
               drop_path_add_reference(x, res, 2, p, seed, p_elem, 9),
               1.0 / ((1.0 - p) * (1.0 - p_elem)))


@pytest.mark.parametrize("p_elem", P_ELEMS)
def test_non_finite_dropped_is_skipped_kept_propagates(p_elem):
    shape, p = (3, 5, 64), 0.5
    _, x, _ = _inputs(shape)
    for seed in range(4096):
        m = drop_path_mask(seed, 3, p)
        if 0 < int(m.sum()) < 3:
            break
    keep_s, keep = _keep(shape, p, seed, p_elem, 9)
    bad = torch.full_like(x, float("nan"))
    bad[..., ::2] = float("inf")
    y = EXT.drop_path_fwd(bad, 3, p, seed, p_elem, 9)
    assert bool((_bits(y)[~keep] == 0).all())
    assert not torch.isfinite(y.float()[keep]).any()
    out = EXT.drop_path_add_fwd(x, bad, 3, p, seed, p_elem, 9)
    assert torch.equal(_bits(out)[~keep], _bits(x)[~keep])
    assert not torch.isfinite(out.float()[keep]).any()
    # whole dropped samples: exact zeros, x handed through
    dropped = ~keep_s.reshape(3)
    assert bool(dropped.any())
    assert bool((_bits(y)[dropped] == 0).all())
    assert torch.equal(_bits(out)[dropped], _bits(x)[dropped])


def test_leading_dims_flatten():
    _, x, res = _inputs((2, 3, 64), seed=1)
    for p_elem in P_ELEMS:
        for seed in (0, 1, 2, 3):
            a3 = EXT.drop_path_fwd(x, 2, 0.5, seed, p_elem, 7)
            a2 = EXT.drop_path_fwd(x.view(6, 64), 2, 0.5, seed, p_elem, 7)
            b3 = EXT.drop_path_add_fwd(x, res, 2, 0.5, seed, p_elem, 7)
            b2 = EXT.drop_path_add_fwd(
                x.view(6, 64), res.view(6, 64), 2, 0.5, seed, p_elem, 7)
            assert a3.shape == (2, 3, 64) and a2.shape == (6, 64)
            assert torch.equal(_bits(a3).view(6, 64), _bits(a2))
            assert torch.equal(_bits(b3).view(6, 64), _bits(b2))
    # rows == 0 is an empty tensor
    empty = x[:, :0]
    assert EXT.drop_path_fwd(empty, 2, 0.5, 0, 0.0, 0).shape == (2, 0, 64)


def test_offsets_past_2_31_elements():
    """(65537, 1, 32768) is 2^31 + 32768 elements: the smallest batch at
    this width where a 32-bit element offset wraps.  First row and last
    two rows against the reference."""
    B, C, p, pe, seed, es = 65537, 32768, 0.5, 0.25, 1234, 99
    x = torch.randn(B, 1, C, device=_dev(), dtype=torch.bfloat16)
    y = EXT.drop_path_fwd(x, B, p, seed, pe, es)
    pick = torch.tensor([0, B - 2, B - 1])
    keep_s = drop_path_mask(seed, B, p)
    # both outcomes are among the rows that are looked at
    kept, dropped = [int(torch.nonzero(keep_s == v)[-1]) for v in (True, False)]
    pick = torch.unique(torch.cat([pick, torch.tensor([kept, dropped])]))
    keep = keep_s[pick].reshape(-1, 1, 1) & dropout_mask_reference(
        es, pick, torch.arange(C), pe).reshape(-1, 1, C)
    pick = pick.to(_dev())
    assert torch.equal(
        _bits(y[pick]), _bits(_fwd_expected(x[pick], keep.to(_dev()), p, pe)))
    del x, y
    torch.cuda.empty_cache()


def _stock(t, p_path, p_elem):
    b = F.dropout(t, p_elem, True)
    keep = b.new_empty((t.shape[0],) + (1,) * (t.dim() - 1)).bernoulli_(
        1.0 - p_path)
    return b * keep / (1.0 - p_path)


def test_refusals_and_stock_fallback(monkeypatch):
    monkeypatch.delenv("VITFSDP_NATIVE_DROPOUT", raising=False)
    dev = _dev()
    odd = torch.randn(4, 3, 100, device=dev, dtype=torch.bfloat16)
    f32 = torch.randn(4, 3, 64, device=dev)
    ok = torch.randn(4, 3, 64, device=dev, dtype=torch.bfloat16)
    calls = [
        lambda t, n, pp, pe: EXT.drop_path_fwd(t, n, pp, 1, pe, 2),
        lambda t, n, pp, pe: EXT.drop_path_add_fwd(t, t, n, pp, 1, pe, 2),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="multiple of 8"):
            call(odd, 4, 0.1, 0.0)
        with pytest.raises(RuntimeError, match="bf16 only"):
            call(f32, 4, 0.1, 0.0)
        for pp in (0.0, 1.0, -0.1, 1.5):
            with pytest.raises(RuntimeError,
                               match=r"p_path must be in \(0, 1\)"):
                call(ok, 4, pp, 0.0)
        for pe in (1.0, -0.1, 1.5):
            with pytest.raises(RuntimeError,
                               match=r"p_elem must be in \[0, 1\)"):
                call(ok, 4, 0.1, pe)
        for n in (0, -1, 5, 24):
            with pytest.raises(RuntimeError, match="n_samples must divide"):
                call(ok, n, 0.1, 0.0)
        assert call(ok, 12, 0.1, 0.0).shape == ok.shape
    with pytest.raises(RuntimeError, match="one shape"):
        EXT.drop_path_add_fwd(ok, ok[:2], 2, 0.1, 1, 0.0, 2)

    # the public functions take the stock composition for those inputs
    def same_as_stock(ours, stock):
        torch.manual_seed(3)
        a = ours()
        torch.manual_seed(3)
        assert torch.equal(a, stock())

    inputs = [(odd, 0.5, 0.1), (f32, 0.5, 0.1), (f32, 0.5, 0.0),
              (ok, 0.5, 1.0), (ok[0, 0], 0.5, 0.1)]
    for t, pp, pe in inputs:
        same_as_stock(lambda: drop_path(t, pp, True, p_elem=pe),
                      lambda: _stock(t, pp, pe))
        same_as_stock(lambda: drop_path_add(t, t, pp, True, p_elem=pe),
                      lambda: t + _stock(t, pp, pe))
    monkeypatch.setenv("VITFSDP_NATIVE_DROPOUT", "0")
    same_as_stock(lambda: drop_path(ok, 0.5, True, p_elem=0.1),
                  lambda: _stock(ok, 0.5, 0.1))
    same_as_stock(lambda: drop_path_add(ok, ok, 0.5, True, p_elem=0.1),
                  lambda: ok + _stock(ok, 0.5, 0.1))
    monkeypatch.delenv("VITFSDP_NATIVE_DROPOUT")
    # p_path == 0 and eval are the element-dropout call, seed and all
    assert torch.equal(
        _bits(drop_path(ok, 0.0, True, p_elem=0.25, elem_seed=5)),
        _bits(EXT.dropout_fwd(ok, 0.25, 5)))
    assert torch.equal(
        _bits(drop_path_add(ok, ok, 0.0, True, p_elem=0.25, elem_seed=5)),
        _bits(EXT.dropout_add_fwd(ok, ok, 0.25, 5)))
    assert torch.equal(drop_path(ok, 0.5, False, p_elem=0.25), ok)
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError):
            drop_path(ok, bad, True)
        with pytest.raises(ValueError):
            drop_path_add(ok, ok, bad, True)


@pytest.mark.parametrize("p_elem", P_ELEMS)
def test_autograd_matches_direct_calls(p_elem):
    shape, p, seed, es = (2, 257, 2048), 0.5, 1, 1234
    assert drop_path_mask(seed, 2, p).tolist() in ([True, False],
                                                   [False, True])
    dy, x, res = _inputs(shape)
    args = (2, p, seed, p_elem, es)

    xr = x.clone().requires_grad_(True)
    y = drop_path(xr, p, True, p_elem=p_elem, seed=seed, elem_seed=es)
    assert torch.equal(_bits(y), _bits(EXT.drop_path_fwd(x, *args)))
    (g,) = torch.autograd.grad(y, xr, dy)
    assert torch.equal(_bits(g), _bits(EXT.drop_path_fwd(dy, *args)))

    xr = x.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True)
    out = drop_path_add(xr, rr, p, True, p_elem=p_elem, seed=seed,
                        elem_seed=es)
    assert torch.equal(_bits(out), _bits(EXT.drop_path_add_fwd(x, res, *args)))
    gx, gr = torch.autograd.grad(out, (xr, rr), dy)
    assert torch.equal(_bits(gx), _bits(dy))
    assert torch.equal(_bits(gr), _bits(EXT.drop_path_fwd(dy, *args)))


def test_seed_determinism():
    shape = (8, 64, 20480)
    _, x, res = _inputs(shape)
    # seeds 11 and 12 keep different samples
    assert not torch.equal(drop_path_mask(11, 8, 0.5),
                           drop_path_mask(12, 8, 0.5))
    for fn in (lambda s: drop_path(x, 0.5, True, seed=s),
               lambda s: drop_path_add(x, res, 0.5, True, seed=s),
               lambda s: drop_path(x, 0.5, True, p_elem=0.25, seed=s,
                                   elem_seed=3)):
        assert torch.equal(_bits(fn(11)), _bits(fn(11)))
        assert not torch.equal(_bits(fn(11)), _bits(fn(12)))
    # the default seeds come from the CPU generator: the element seed
    # first, the path seed second, none for a mask that is off
    for p_elem in P_ELEMS:
        torch.manual_seed(5)
        a = drop_path(x, 0.5, True, p_elem=p_elem)
        b = drop_path_add(x, res, 0.5, True, p_elem=p_elem)
        state = torch.get_rng_state()
        torch.manual_seed(5)
        es = _draw_seed() if p_elem > 0.0 else 0
        ps = _draw_seed()
        assert torch.equal(
            _bits(a), _bits(EXT.drop_path_fwd(x, 8, 0.5, ps, p_elem, es)))
        es = _draw_seed() if p_elem > 0.0 else 0
        ps = _draw_seed()
        assert torch.equal(_bits(b), _bits(
            EXT.drop_path_add_fwd(x, res, 8, 0.5, ps, p_elem, es)))
        assert torch.equal(state, torch.get_rng_state())


def _block(**kw):
    from vit_10b_fsdp_example_amd.models.vit import Block

    torch.manual_seed(0)
    return Block(640, 4, **kw).to(_dev(), torch.bfloat16).train()


def _saved_dtypes():
    blk = _block(drop=0.2, drop_path=0.3)
    x = torch.randn(2, 256, 640, device=_dev(), dtype=torch.bfloat16,
                    requires_grad=True)
    dtypes = []

    def pack(t):
        dtypes.append(t.dtype)
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = blk(x)
    out.float().sum().backward()
    assert torch.isfinite(x.grad.float()).all()
    return dtypes


def test_block_stores_no_mask(monkeypatch):
    monkeypatch.delenv("VITFSDP_NATIVE_DROPOUT", raising=False)
    dtypes = _saved_dtypes()
    assert dtypes
    assert torch.bool not in dtypes and torch.uint8 not in dtypes, dtypes
    # the probe does see the stock path's masks
    monkeypatch.setenv("VITFSDP_NATIVE_DROPOUT", "0")
    assert torch.bool in _saved_dtypes()


@pytest.mark.parametrize("deferred", [False, True])
def test_dropped_sample_is_a_skip_connection(deferred, monkeypatch):
    monkeypatch.delenv("VITFSDP_NATIVE_DROPOUT", raising=False)
    B, p = 8, 0.5
    # with drop == 0 the block draws exactly two integers per forward:
    # the attention branch's path seed, then the MLP branch's
    for gen_seed in range(64):
        torch.manual_seed(gen_seed)
        both = ~drop_path_mask(_draw_seed(), B, p) & ~drop_path_mask(
            _draw_seed(), B, p)
        if bool(both.any()) and not bool(both.all()):
            break
    else:
        raise AssertionError("no generator seed drops a sample twice")
    blk = _block(drop=0.0, drop_path=p, deferred_residual=deferred)
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(B, 256, 640, generator=g).to(
        _dev(), torch.bfloat16).requires_grad_(True)
    dout = torch.randn(B, 256, 640, generator=g).to(_dev(), torch.bfloat16)
    torch.manual_seed(gen_seed)
    out = blk(x)
    if deferred:
        hidden, stream = out
        torch.autograd.backward([hidden, stream], [dout, dout])
        assert bool((hidden[both.to(_dev())] == 0).all())
        out = stream + hidden
    else:
        out.backward(dout)
    for b in torch.nonzero(both).flatten().tolist():
        assert torch.equal(out[b], x[b])
        err = (x.grad[b].float() - dout[b].float()).abs()
        # one bf16 ulp is at most 2^-7 of the value
        assert bool((err <= 2.0 ** -7 * dout[b].float().abs()).all())
    kept = torch.nonzero(~both).flatten().tolist()
    assert all(not torch.equal(out[b], x[b]) for b in kept)


def test_drop_path_with_checkpointing():
    """--drop_path_rate under gradient checkpointing, after
    test_hidden_dropout_with_checkpointing: the path seeds come from the
    CPU generator too, so the recompute must regenerate the forward's
    per-sample masks."""
    from vit_10b_fsdp_example_amd.cli import parse_args
    from vit_10b_fsdp_example_amd import dist as xdist
    from vit_10b_fsdp_example_amd.models import build_fsdp_vit_model
    from vit_10b_fsdp_example_amd.ops import CrossEntropyLoss, FusedAdamW
    from vit_10b_fsdp_example_amd.parallel import CommContext

    def build(extra=()):
        CommContext.reset()
        cfg = parse_args([
            "--fake_data", "--image_size", "224", "--patch_size", "14",
            "--embed_dim", "640", "--num_heads", "4", "--num_blocks", "2",
            "--num_classes", "100", "--batch_size", "8",
            "--num_workers", "0", "--mlp_dropout", "0.2",
            "--pos_dropout", "0.1", "--drop_path_rate", "0.3", *extra,
        ])
        device = xdist.init_distributed()
        torch.manual_seed(0)
        model = build_fsdp_vit_model(cfg, device, compute_dtype=torch.bfloat16)
        assert cfg.grad_ckpt == ("--no_grad_ckpt" not in extra)
        x = torch.randn(8, 3, 224, 224, device=device, dtype=torch.bfloat16)
        y = torch.randint(0, 100, (8,), device=device)
        return model, x, y

    def one_step_grads(extra=()):
        model, x, y = build(extra)
        torch.manual_seed(4321)  # governs the per-call dropout seeds
        loss = CrossEntropyLoss()(model(x), y)
        loss.backward()
        grads = [
            u.flat_param._comm_grad.clone() for u in model._all_units()
        ]
        return float(loss.detach()), grads

    def assert_same(a, b, what):
        (l1, g1), (l2, g2) = a, b
        assert abs(l1 - l2) < 5e-3 * max(abs(l1), 1.0), (
            f"{what}: drop_path fwd diverged: {l1} vs {l2}")
        for u, v in zip(g1, g2):
            scale = u.float().abs().max() + 1e-6
            rel = (u.float() - v.float()).abs().max() / scale
            assert float(rel) < 5e-2, f"{what}: mask mismatch: rel {rel}"

    r1 = one_step_grads()
    r2 = one_step_grads()
    r3 = one_step_grads(["--no_grad_ckpt"])
    assert_same(r1, r2, "ckpt vs ckpt")
    assert_same(r1, r3, "ckpt vs no ckpt")

    f1 = one_step_grads(["--fuse_residual"])
    f2 = one_step_grads(["--fuse_residual", "--no_grad_ckpt"])
    assert_same(f1, f2, "fuse_residual, ckpt vs no ckpt")

    # training health over full steps (clip + AdamW included)
    model, x, y = build()
    opt = FusedAdamW(model.parameters(), lr=3e-3, weight_decay=0.1)
    loss_fn = CrossEntropyLoss()
    torch.manual_seed(4321)
    losses = []
    for _ in range(8):
        loss = loss_fn(model(x), y)
        loss.backward()
        model.clip_grad_norm_(1.0, defer_scale=True)
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(float(loss.detach()))
    assert all(v == v and abs(v) != float("inf") for v in losses), losses
    assert min(losses) < losses[0], f"no progress under drop_path: {losses}"
