"""csrc/layer_scale.hip and ops/layer_scale.py on the GPU against fp64
references, within one bf16 rounding plus fp32 arithmetic (u = 2^-24);
autograd, refusals, and the Block and the model with --layer_scale_init."""

import functools

import pytest
import torch

from vit_10b_fsdp_example_amd import dist as xdist
from vit_10b_fsdp_example_amd.cli import parse_args
from vit_10b_fsdp_example_amd.models import Block, build_fsdp_vit_model
from vit_10b_fsdp_example_amd.ops import (
    CrossEntropyLoss, drop_path, drop_path_mask, hidden_dropout, layer_scale,
    layer_scale_add, layer_scale_add_reference, layer_scale_bwd_reference,
    layer_scale_reference,
)
from vit_10b_fsdp_example_amd.ops._extension import ext
from vit_10b_fsdp_example_amd.ops.attention import _draw_seed, dropout_mask_reference
from vit_10b_fsdp_example_amd.parallel import CommContext

pytestmark = pytest.mark.gpu

U, BF = 2.0 ** -24, 2.0 ** -8
SHAPES = [(1, 1, 8), (3, 5, 64), (2, 257, 2048), (5, 3, 2056), (4, 64, 5120)]
PROBS = [(0.0, 0.0), (0.0, 0.25), (0.5, 0.0), (0.5, 0.25)]
ES = 77  # element seed


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """(x, res, dy, branch, gamma) bf16 on the GPU; shared, never modified."""
    g = torch.Generator(device="cpu").manual_seed(0)
    ts = [torch.randn(shape, generator=g) for _ in range(4)]
    ts.append(0.5 + torch.randn(shape[-1], generator=g) * 0.25)
    return tuple(t.to("cuda", torch.bfloat16) for t in ts)


@pytest.mark.parametrize("seed", [26, 28])
@pytest.mark.parametrize("p_path,p_elem", PROBS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_against_fp64(shape, p_path, p_elem, seed):
    x, res, dy, branch, gamma = _inputs(shape)
    args = (shape[0], p_path, seed, p_elem, ES)
    rscale = 1.0 / ((1.0 - p_path) * (1.0 - p_elem))
    keep = layer_scale_reference(torch.ones_like(x), torch.ones_like(gamma), *args) != 0
    if p_path > 0 and shape[0] >= 2:  # samples of both kinds
        m = drop_path_mask(seed, shape[0], p_path)
        assert bool(m.any()) and not bool(m.all())

    y, ref = ext().layer_scale_fwd(x, gamma, *args), layer_scale_reference(x, gamma, *args)
    assert bool((_bits(y)[~keep] == 0).all())
    assert bool(((y.double() - ref).abs() <= (BF + 4 * U) * ref.abs()).all())

    out = ext().layer_scale_add_fwd(x, res, gamma, *args)
    ref = layer_scale_add_reference(x, res, gamma, *args)
    assert torch.equal(_bits(out)[~keep], _bits(x)[~keep])
    bound = BF * ref.abs() + 4 * U * (x.double().abs() + (res.double() * gamma.double()).abs() * rscale)
    assert bool(((out.double() - ref).abs() <= bound)[keep].all())

    db, dg = ext().layer_scale_bwd(dy, branch, gamma, *args)
    ref, dg_ref, terms = layer_scale_bwd_reference(dy, branch, gamma, *args)
    assert bool((_bits(db)[~keep] == 0).all())
    assert bool(((db.double() - ref).abs() <= (BF + 4 * U) * ref.abs()).all())
    bound = BF * dg_ref.abs() + (terms.shape[0] + 3) * U * terms.abs().sum(0)
    err = (dg.double() - dg_ref).abs()
    assert dg.shape == gamma.shape and bool((err <= bound).all())
    assert torch.equal(_bits(dg), _bits(ext().layer_scale_bwd(dy, branch, gamma, *args)[1]))


@pytest.mark.parametrize("p_elem", [0.0, 0.25])
def test_non_finite_under_a_dropped_sample(p_elem):
    shape, args = (3, 5, 64), (3, 0.5, 26, p_elem, ES)
    x, res, dy, branch, gamma = _inputs(shape)
    assert drop_path_mask(26, 3, 0.5).tolist() == [False, True, False]
    for sample, finite in ((0, True), (1, False)):
        bad = res.clone()
        bad[sample, :, ::2] = float("nan")
        bad[sample, :, 1::2] = float("inf")
        y = ext().layer_scale_fwd(bad, gamma, *args)
        out = ext().layer_scale_add_fwd(x, bad, gamma, *args)
        # dbranch does not depend on branch
        db, dg = ext().layer_scale_bwd(dy, bad, gamma, *args)
        assert bool(torch.isfinite(db.float()).all())
        for t in (y, out, dg, *ext().layer_scale_bwd(bad, branch, gamma, *args)):
            assert bool(torch.isfinite(t.float()).all()) == finite
        if finite:
            assert bool((_bits(y)[sample] == 0).all())
            assert torch.equal(_bits(out)[sample], _bits(x)[sample])


def test_offsets_past_2_31_elements():
    # 2^31 + 32768 elements: dbranch of the first and the last two rows
    B, C, p, pe, seed = 65537, 32768, 0.5, 0.25, 26
    dy = torch.randn(B, 1, C, device="cuda", dtype=torch.bfloat16)
    branch = torch.randn(B, 1, C, device="cuda", dtype=torch.bfloat16)
    gamma = _inputs((1, 1, C))[4]
    db, dg = ext().layer_scale_bwd(dy, branch, gamma, B, p, seed, pe, ES)
    keep_s = drop_path_mask(seed, B, p)
    kept, dropped = [int(torch.nonzero(keep_s == v)[-1]) for v in (True, False)]
    pick = torch.unique(torch.tensor([0, B - 2, B - 1, kept, dropped]))
    keep = (keep_s[pick].reshape(-1, 1, 1) & dropout_mask_reference(
        ES, pick, torch.arange(C), pe).reshape(-1, 1, C)).cuda()
    ref = dy[pick.cuda()].double() * gamma.double() / ((1 - p) * (1 - pe))
    ref = torch.where(keep, ref, torch.zeros_like(ref))
    got = db[pick.cuda()]
    assert bool((_bits(got)[~keep] == 0).all())
    assert bool(((got.double() - ref).abs() <= (BF + 4 * U) * ref.abs()).all())
    assert bool(torch.isfinite(dg.float()).all())


@pytest.mark.parametrize("p_path,p_elem", PROBS)
def test_autograd_and_seed_order(p_path, p_elem):
    shape = (2, 257, 2048)
    x, res, dy, _, gamma = _inputs(shape)
    xr, rr, gr = (t.clone().requires_grad_(True) for t in (x, res, gamma))
    torch.manual_seed(5)
    y = layer_scale(rr, gr, True, p_path=p_path, p_elem=p_elem)
    out = layer_scale_add(xr, rr, gr, True, p_path=p_path, p_elem=p_elem)
    state = torch.get_rng_state()
    torch.manual_seed(5)
    for got, fwd, ins in ((y, ext().layer_scale_fwd, (rr, gr)),
                          (out, ext().layer_scale_add_fwd, (xr, rr, gr))):
        # element seed first, path seed second, none for a mask that is off
        es = _draw_seed() if p_elem > 0 else 0
        args = (2, p_path, _draw_seed() if p_path > 0 else 0, p_elem, es)
        assert torch.equal(_bits(got), _bits(fwd(*[t.detach() for t in ins], *args)))
        grads = torch.autograd.grad(got, ins, dy)
        want = ext().layer_scale_bwd(dy, res, gamma, *args)
        for a, b in zip(grads[-2:], want):
            assert torch.equal(_bits(a), _bits(b))
        if len(ins) == 3:
            assert torch.equal(_bits(grads[0]), _bits(dy))
    assert torch.equal(state, torch.get_rng_state())
    # eval: the pure scale, no draw
    y = layer_scale(res, gamma, False, p_path=p_path, p_elem=p_elem)
    assert torch.equal(state, torch.get_rng_state())
    assert torch.equal(_bits(y), _bits(ext().layer_scale_fwd(res, gamma, 2, 0.0, 0, 0.0, 0)))


def test_refusals_and_composition_route(monkeypatch):
    ok, _, _, _, gamma = _inputs((3, 5, 64))
    cases = [  # (x, other, gamma, n_samples, p_path, p_elem), message
        ((ok.transpose(0, 1), ok.transpose(0, 1), gamma, 5, 0, 0), "must be a contiguous GPU tensor"),
        ((ok.float(), ok.float(), gamma, 3, 0, 0), "bf16 only"),
        ((ok.cpu(), ok.cpu(), gamma, 3, 0, 0), "contiguous GPU tensor"),
        ((ok[..., :12].contiguous(),) * 2 + (gamma[:12], 3, 0, 0), "multiple of 8"),
        ((ok, ok, gamma.float(), 3, 0, 0), "bf16 only, gamma"),
        ((ok, ok, gamma.cpu(), 3, 0, 0), "gamma must be a contiguous GPU"),
        ((ok, ok, gamma[:56], 3, 0, 0), r"gamma must have shape \[64\]"),
        ((ok, ok, gamma, 4, 0, 0), "n_samples must divide"),
        ((ok, ok, gamma, 3, 1.0, 0), r"p_path must be in \[0, 1\)"),
        ((ok, ok, gamma, 3, 0, -0.1), r"p_elem must be in \[0, 1\)"),
    ]
    for (a, b, g, n, pp, pe), msg in cases:
        for fn, ins in ((ext().layer_scale_fwd, (a,)),
                        (ext().layer_scale_add_fwd, (a, b)),
                        (ext().layer_scale_bwd, (a, b))):
            with pytest.raises(RuntimeError, match=msg):
                fn(*ins, g, n, pp, 1, pe, 2)
    for fn in (ext().layer_scale_add_fwd, ext().layer_scale_bwd):
        with pytest.raises(RuntimeError, match="one shape"):
            fn(ok, ok[:2], gamma, 1, 0.0, 1, 0.0, 2)
    db, dg = ext().layer_scale_bwd(ok[:, :0], ok[:, :0], gamma, 3, 0.5, 1, 0, 2)
    assert db.shape == (3, 0, 64) and bool((_bits(dg) == 0).all())

    monkeypatch.setenv("VITFSDP_NATIVE_DROPOUT", "0")
    torch.manual_seed(3)
    a = layer_scale(ok, gamma, True, p_path=0.5, p_elem=0.25)
    b = layer_scale_add(ok, ok, gamma, True, p_path=0.5, p_elem=0.25)
    torch.manual_seed(3)
    comp = lambda: drop_path(hidden_dropout(ok, 0.25, True) * gamma, 0.5, True)
    assert torch.equal(a, comp()) and torch.equal(b, ok + comp())


def _assert_same(a, b, what):  # test_drop_path_with_checkpointing's bounds
    (l1, g1), (l2, g2) = a, b
    assert abs(l1 - l2) < 5e-3 * max(abs(l1), 1.0), f"{what}: {l1} vs {l2}"
    for u, v in zip(g1, g2):
        rel = (u.float() - v.float()).abs().max() / (u.float().abs().max() + 1e-6)
        assert float(rel) < 5e-2, f"{what}: rel {rel}"


@pytest.mark.parametrize("deferred", [False, True])
def test_block(deferred, monkeypatch):
    g = torch.Generator(device="cpu").manual_seed(1)
    x, dout = (torch.randn(2, 256, 640, generator=g).to("cuda", torch.bfloat16) for _ in range(2))

    def run(**kw):
        torch.manual_seed(0)
        blk = Block(640, 4, layer_scale_init=0.1, deferred_residual=deferred, **kw).to("cuda", torch.bfloat16).train()
        xr = x.clone().requires_grad_(True)
        out = blk(xr)
        out = out[0] + out[1] if deferred else out
        out.backward(dout)
        grads = [xr.grad] + [p.grad for p in blk.parameters()]
        return blk, (float(out.detach().float().square().mean()), grads)

    monkeypatch.delenv("VITFSDP_NATIVE_DROPOUT", raising=False)
    blk, _ = run(drop=0.2, drop_path=0.3)
    for grad in (blk.ls1.gamma.grad, blk.ls2.gamma.grad):
        assert bool(torch.isfinite(grad.float()).all() and (grad != 0).any())
    _, native = run()  # drop = drop_path = 0: no randomness left
    monkeypatch.setenv("VITFSDP_NATIVE_DROPOUT", "0")
    _assert_same(native, run()[1], "native vs composition")


def test_layer_scale_with_checkpointing():
    def one_step_grads(extra=()):
        CommContext.reset()
        cfg = parse_args([
            "--fake_data", "--image_size", "224", "--patch_size", "14",
            "--embed_dim", "640", "--num_heads", "4", "--num_blocks", "2",
            "--num_classes", "100", "--batch_size", "8", "--num_workers", "0",
            "--mlp_dropout", "0.2", "--drop_path_rate", "0.3",
            "--layer_scale_init", "1e-2", *extra,
        ])
        device = xdist.init_distributed()
        torch.manual_seed(0)
        model = build_fsdp_vit_model(cfg, device, compute_dtype=torch.bfloat16)
        x = torch.randn(8, 3, 224, 224, device=device, dtype=torch.bfloat16)
        y = torch.randint(0, 100, (8,), device=device)
        torch.manual_seed(4321)  # governs the per-call dropout seeds
        loss = CrossEntropyLoss()(model(x), y)
        loss.backward()
        return float(loss.detach()), [u.flat_param._comm_grad.clone() for u in model._all_units()]

    _assert_same(one_step_grads(), one_step_grads(["--no_grad_ckpt"]), "ckpt vs no ckpt")
