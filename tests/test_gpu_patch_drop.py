"""csrc/patch_drop.hip and ops/patch_drop.py on the GPU: the plan against
its CPU reference, the embed kernels against torch's add, _C.dropout_fwd
and fp64, the argument checks, and a training step at an odd kept count."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from vit_10b_fsdp_example_amd.ops import _extension

    EXT = _extension.ext()
else:
    EXT = None

from vit_10b_fsdp_example_amd.ops import (  # noqa: E402
    hidden_dropout_reference, patch_drop_embed, patch_drop_embed_reference,
    patch_drop_plan_reference,
)

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
# one vector; 257 vectors, across a 2048-column chunk edge
WIDTHS = [8, 2056]
PS = [0.0, 0.3]


def _rand(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV, BF)


def _plan(seed, B, T, K):
    return tuple(t.to(DEV) for t in patch_drop_plan_reference(seed, B, T, K))


def _dpos_bound_ok(dpos, terms, idx, T, ref=None):
    """|dpos - ref| <= 2^-8 |ref| + B 2^-23 sum_b |term_b| per element,
    ref = the fp64 sum of terms [B, K, E] into their tokens."""
    B, K, E = terms.shape
    flat = idx.long().reshape(-1)
    mag = torch.zeros(T, E, dtype=torch.float64, device=DEV)
    mag.index_add_(0, flat, terms.abs().reshape(-1, E))
    if ref is None:
        ref = torch.zeros_like(mag).index_add_(0, flat, terms.reshape(-1, E))
    err = (dpos.double().reshape(T, E) - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + B * 2.0 ** -23 * mag
    print(f"dpos: worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    return bool((err <= bound).all())


@pytest.mark.parametrize("seed", [0, 2 ** 31 - 2])
@pytest.mark.parametrize("B,T,K", [
    (3, 16, 1), (3, 16, 15),   # the edge counts
    (2, 64, 64),               # keep all
    (2, 257, 100),             # two tokens per thread
    (2, 1024, 512),            # the cap
])
def test_plan_equals_reference(B, T, K, seed):
    idx, inv = EXT.patch_drop_plan(seed, B, T, K)
    ref_idx, ref_inv = patch_drop_plan_reference(seed, B, T, K)
    assert idx.dtype == inv.dtype == torch.int32
    assert torch.equal(idx.cpu(), ref_idx) and torch.equal(inv.cpu(), ref_inv)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("E", WIDTHS)
def test_embed_fwd_bit_exact(E, p):
    B, T, K, seed = 3, 16, 5, 99
    idx, _ = _plan(7, B, T, K)
    proj, pos = _rand(B, K, E), _rand(T, E, seed=1)
    want = proj + pos[idx.long()]
    if p > 0:
        want = EXT.dropout_fwd(want, p, seed)
    assert torch.equal(EXT.patch_drop_embed_fwd(proj, pos, idx, p, seed), want)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,E", [(3, 8), (3, 2056), (5, 64)])
def test_embed_bwd(B, E, p):
    T, K, seed = 16, 5, 99
    for plan_seed in range(64):
        idx, inv = patch_drop_plan_reference(plan_seed, B, T, K)
        never = torch.nonzero((inv < 0).all(0)).flatten()
        if never.numel():
            break
    else:
        raise AssertionError("no plan seed leaves a token unkept")
    idx, inv = idx.to(DEV), inv.to(DEV)
    dy = _rand(B, K, E, seed=2)
    dproj, dpos = EXT.patch_drop_embed_bwd(dy, inv, T, p, seed)
    if p > 0:
        assert torch.equal(dproj, EXT.dropout_fwd(dy, p, seed))
        terms = hidden_dropout_reference(dy, p, seed)
    else:
        assert dproj.data_ptr() == dy.data_ptr()
        terms = dy.double()
    assert dpos.shape == (T, E) and dpos.dtype == BF
    assert _dpos_bound_ok(dpos, terms, idx, T)
    assert bool((dpos[never.to(DEV)] == 0).all())


# the plan takes no tensors: only the two counts can be wrong
@pytest.mark.parametrize("entry,bad", [
    (entry, bad)
    for entry in ("patch_drop_plan", "patch_drop_embed_fwd",
                  "patch_drop_embed_bwd")
    for bad in ("fp32", "width", "T=1025", "K>T", "int64")
    if entry != "patch_drop_plan" or bad in ("T=1025", "K>T")])
def test_argument_errors(entry, bad):
    B = 2
    T = 1025 if bad == "T=1025" else 16
    K = T + 1 if bad == "K>T" else 5
    E = 12 if bad == "width" else 16
    itype = torch.int64 if bad == "int64" else torch.int32
    proj = torch.zeros(B, K, E, device=DEV,
                       dtype=torch.float32 if bad == "fp32" else BF)
    pos = torch.zeros(T, E, device=DEV, dtype=BF)
    idx = torch.zeros(B, K, device=DEV, dtype=itype)
    inv = torch.zeros(B, T, device=DEV, dtype=itype)
    with pytest.raises(RuntimeError, match=entry):
        if entry == "patch_drop_plan":
            EXT.patch_drop_plan(1, B, T, K)
        elif entry == "patch_drop_embed_fwd":
            EXT.patch_drop_embed_fwd(proj, pos, idx, 0.3, 1)
        else:
            EXT.patch_drop_embed_bwd(proj, inv, T, 0.3, 1)


def test_autograd_op():
    B, T, K, E, p, seed = 3, 16, 5, 64, 0.3, 99
    idx, inv = _plan(7, B, T, K)
    proj = _rand(B, K, E).requires_grad_(True)
    pos = _rand(1, T, E, seed=1).requires_grad_(True)
    dy = _rand(B, K, E, seed=2)
    out = patch_drop_embed(proj, pos, idx, inv, p, True, seed=seed)
    assert torch.equal(out, EXT.patch_drop_embed_fwd(
        proj.detach(), pos.detach()[0], idx, p, seed))
    out.backward(dy)
    assert pos.grad.shape == (1, T, E)

    proj64 = proj.detach().double().requires_grad_(True)
    pos64 = pos.detach().double().requires_grad_(True)
    patch_drop_embed_reference(proj64, pos64, idx, p, seed).backward(
        dy.double())
    # dproj: one fp32 product, one bf16 rounding
    err = (proj.grad.double() - proj64.grad).abs()
    assert bool((err <= (2.0 ** -8 + 2.0 ** -23) * proj64.grad.abs()).all())
    # pos64.grad is the sum of proj64.grad's rows into their tokens
    assert _dpos_bound_ok(pos.grad, proj64.grad, idx, T, ref=pos64.grad[0])


def test_training_step_at_an_odd_kept_count():
    """Built like test_drop_path_with_checkpointing: T = 256, K = 179, an
    odd row count for every GEMM route and for the attention.

    A second run repeats the first bit for bit in the logits and in every
    communicated gradient.  The loss is held to the order of its sum
    instead: csrc/cross_entropy.hip adds the 8 per-row terms, all
    positive, with fp32 atomics in any order, and two orders of n terms
    differ by at most 2 (n - 1) 2^-24 of their sum.  Measured: gradients
    equal, losses 4.5527143478 and 4.5527148247, one fp32 ulp apart."""
    from vit_10b_fsdp_example_amd.cli import parse_args
    from vit_10b_fsdp_example_amd import dist as xdist
    from vit_10b_fsdp_example_amd.models import build_fsdp_vit_model
    from vit_10b_fsdp_example_amd.models.vit import Block
    from vit_10b_fsdp_example_amd.ops import CrossEntropyLoss
    from vit_10b_fsdp_example_amd.parallel import CommContext

    def one_step_grads(extra=()):
        CommContext.reset()
        cfg = parse_args([
            "--fake_data", "--image_size", "224", "--patch_size", "14",
            "--embed_dim", "640", "--num_heads", "4", "--num_blocks", "2",
            "--num_classes", "100", "--batch_size", "8",
            "--num_workers", "0", "--patch_drop_rate", "0.3",
            "--pos_dropout", "0.1", *extra,
        ])
        device = xdist.init_distributed()
        torch.manual_seed(0)
        model = build_fsdp_vit_model(cfg, device, compute_dtype=BF)
        assert cfg.grad_ckpt == ("--no_grad_ckpt" not in extra)
        x = torch.randn(8, 3, 224, 224, device=device, dtype=BF)
        y = torch.randint(0, 100, (8,), device=device)
        tokens = []
        block0 = next(m for m in model.modules() if isinstance(m, Block))
        block0.norm1.register_forward_pre_hook(
            lambda mod, args: tokens.append(args[0].shape[1]))
        torch.manual_seed(4321)  # governs the plan and dropout seeds
        logits = model(x)
        loss = CrossEntropyLoss()(logits, y)
        loss.backward()
        assert tokens and set(tokens) == {179}, tokens
        grads = [u.flat_param._comm_grad.clone() for u in model._all_units()]
        return float(loss.detach()), grads, logits.detach()

    (l1, g1, y1), (l2, g2, y2) = one_step_grads(), one_step_grads()
    l3, g3, _ = one_step_grads(["--no_grad_ckpt"])
    print(f"losses {l1!r} {l2!r} {l3!r}")
    assert torch.equal(y1, y2), "second run differs"
    assert all(torch.equal(u, v) for u, v in zip(g1, g2)), "second run differs"
    assert abs(l1 - l2) <= 2 * 7 * 2.0 ** -24 * abs(l1)
    # checkpointing: that test's tolerances
    assert abs(l1 - l3) < 5e-3 * max(abs(l1), 1.0), f"{l1} vs {l3}"
    for u, v in zip(g1, g3):
        rel = (u.float() - v.float()).abs().max() / (u.float().abs().max() + 1e-6)
        assert float(rel) < 5e-2, f"ckpt vs no ckpt: mask mismatch: rel {rel}"
