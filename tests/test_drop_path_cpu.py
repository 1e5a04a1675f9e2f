"""Stochastic depth (--drop_path_rate) away from the GPU: the flag, the
linear ramp over depth, no new state, no change at rate 0 (values and
RNG consumption), the stock per-sample composition, the statistics of
the hash mask at column 0, and the trainer end to end."""

import glob
import math
import os
import re

import pytest
import torch

from test_cli import REFERENCE_DEFAULTS
from vit_10b_fsdp_example_amd.cli import parse_args
from vit_10b_fsdp_example_amd.models.vit import Block, FSDPViTModel
from vit_10b_fsdp_example_amd.ops import (
    drop_path, drop_path_add, drop_path_mask,
)


def test_cli_flag():
    cfg = parse_args([])
    assert cfg.drop_path_rate == 0.0
    for key, val in REFERENCE_DEFAULTS.items():
        assert getattr(cfg, key) == val, key
    assert len(REFERENCE_DEFAULTS) == 29
    assert parse_args(["--drop_path_rate", "0.3"]).drop_path_rate == 0.3
    for bad in ("1.0", "-0.1"):
        with pytest.raises(SystemExit):
            parse_args(["--drop_path_rate", bad])


def _model(rate, num_blocks=4):
    return FSDPViTModel(
        image_size=16, patch_size=4, embed_dim=32, num_heads=2,
        num_blocks=num_blocks, mlp_ratio=4.0, pos_dropout=0.0,
        mlp_dropout=0.1, att_dropout=0.0, num_classes=5,
        grad_ckpt_wrap=lambda m: m, fsdp_wrap=lambda m: m,
        drop_path_rate=rate,
    )


def test_linear_ramp_over_depth():
    rates = [blk.drop_path for blk in _model(0.3).blocks]
    for got, want in zip(rates, [0.0, 0.1, 0.2, 0.3]):
        assert abs(got - want) <= 1e-12, rates
    assert rates[0] == 0.0
    assert [blk.drop_path for blk in _model(0.3, num_blocks=1).blocks] == [0.0]
    assert "drop_path=" in repr(_model(0.3).blocks[3])
    with pytest.raises(ValueError):
        Block(32, 2, drop_path=1.0)
    with pytest.raises(ValueError):
        Block(32, 2, drop_path=-0.1)


def test_build_reads_the_flag():
    from vit_10b_fsdp_example_amd.models import build_fsdp_vit_model
    from vit_10b_fsdp_example_amd.parallel import CommContext

    for extra, want in (([], [0.0, 0.0, 0.0]),
                        (["--drop_path_rate", "0.2"], [0.0, 0.1, 0.2]),
                        (["--drop_path_rate", "0.2", "--fuse_residual"],
                         [0.0, 0.1, 0.2])):
        CommContext.reset()
        cfg = parse_args([
            "--image_size", "16", "--patch_size", "4", "--embed_dim", "32",
            "--num_heads", "2", "--num_blocks", "3", "--num_classes", "5",
            *extra,
        ])
        model = build_fsdp_vit_model(cfg, torch.device("cpu"))
        rates = [m.drop_path for m in model.modules() if isinstance(m, Block)]
        assert len(rates) == 3
        for got, w in zip(rates, want):
            assert abs(got - w) <= 1e-12, rates


def test_state_dict_keys_do_not_depend_on_drop_path():
    assert list(_model(0.3).state_dict()) == list(_model(0.0).state_dict())
    assert not list(_model(0.3).buffers())


@pytest.mark.parametrize("deferred", [False, True])
def test_rate_zero_changes_nothing(deferred):
    def run(**kw):
        torch.manual_seed(0)
        blk = Block(32, 2, drop=0.2, deferred_residual=deferred, **kw).train()
        x = torch.randn(3, 9, 32, requires_grad=True)
        torch.manual_seed(11)
        out = blk(x)
        outs = list(out) if deferred else [out]
        sum(o.sum() for o in outs).backward()
        grads = [x.grad] + [p.grad for p in blk.parameters()]
        return outs, grads, torch.get_rng_state()

    o1, g1, s1 = run()
    o2, g2, s2 = run(drop_path=0.0)
    assert torch.equal(s1, s2)
    assert len(o1) == len(o2) and len(g1) == len(g2)
    for a, b in zip(o1 + g1, o2 + g2):
        assert torch.equal(a, b)


def _mixed_keep(B, p, seed):
    """The keep tensor the stock composition draws first under
    torch.manual_seed(seed) (p_elem == 0 draws nothing before it)."""
    torch.manual_seed(seed)
    return torch.empty(B, 1, 1).bernoulli_(1.0 - p).reshape(B) != 0


def test_stock_composition_is_per_sample():
    B, p, seed = 6, 0.5, 3
    keep = _mixed_keep(B, p, seed)
    assert 0 < int(keep.sum()) < B, "pick a generator seed with a mixed mask"
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 5, 24, generator=g)
    res = torch.randn(B, 5, 24, generator=g).requires_grad_(True)

    torch.manual_seed(seed)
    y = drop_path(x, p, True)
    torch.manual_seed(seed)
    out = drop_path_add(x, res, p, True)
    (dres,) = torch.autograd.grad(out.sum(), res)
    for b in range(B):
        if keep[b]:
            assert torch.equal(y[b], x[b] / (1.0 - p))
            assert torch.equal(out[b], x[b] + res[b] / (1.0 - p))
            assert torch.equal(dres[b], torch.full_like(dres[b], 1 / (1 - p)))
        else:
            assert torch.equal(y[b], torch.zeros_like(x[b]))
            assert torch.equal(out[b], x[b])
            assert torch.equal(dres[b], torch.zeros_like(dres[b]))

    # eval, and rate 0, are the identity and draw nothing
    torch.manual_seed(seed)
    state = torch.get_rng_state()
    assert torch.equal(drop_path(x, p, False), x)
    assert torch.equal(drop_path_add(x, res, p, False), x + res)
    assert torch.equal(drop_path(x, 0.0, True), x)
    assert torch.equal(drop_path_add(x, res, 0.0, True), x + res)
    assert torch.equal(state, torch.get_rng_state())

    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            drop_path(x, bad, True)
        with pytest.raises(ValueError):
            drop_path_add(x, res, bad, True)


@pytest.mark.parametrize("p", [0.05, 0.1, 0.25, 0.5])
def test_mask_reference_statistics(p):
    """Conditions on the hash at column 0, not measurements: a Bernoulli
    mask of these sizes stays inside them with overwhelming probability."""
    B, n_seeds = 64, 4096
    keep = torch.stack(
        [drop_path_mask(s, B, p) for s in range(n_seeds)]).double()
    assert keep.shape == (n_seeds, B)

    def sigmas(rate, n):
        return abs(rate - (1.0 - p)) / math.sqrt(p * (1.0 - p) / n)

    overall = sigmas(keep.mean().item(), B * n_seeds)
    per_sample = max(sigmas(v, n_seeds) for v in keep.mean(0).tolist())
    print(f"p={p}: overall {overall:.2f} sigma, worst sample index "
          f"{per_sample:.2f}")
    assert overall <= 4.0
    assert per_sample <= 4.5


def test_train_e2e_tiny_with_drop_path(tmp_path, capsys):
    from vit_10b_fsdp_example_amd.train import main
    from vit_10b_fsdp_example_amd.parallel import CommContext
    import vit_10b_fsdp_example_amd.data.datasets as ds

    CommContext.reset()
    cfg = parse_args([
        "--fake_data", "--image_size", "16", "--patch_size", "4",
        "--embed_dim", "32", "--num_heads", "2", "--num_blocks", "2",
        "--num_classes", "10", "--batch_size", "4", "--num_workers", "0",
        "--num_epochs", "1", "--ckpt_epoch_interval", "1",
        "--test_epoch_interval", "1", "--log_step_interval", "1",
        "--warmup_steps", "2", "--max_steps_per_epoch", "3",
        "--drop_path_rate", "0.2", "--mlp_dropout", "0.1",
        "--ckpt_dir", str(tmp_path),
    ])
    orig_train, orig_val = ds.IMAGENET_TRAIN_LEN, ds.IMAGENET_VAL_LEN
    ds.IMAGENET_TRAIN_LEN, ds.IMAGENET_VAL_LEN = 16, 8
    try:
        main(cfg)
    finally:
        ds.IMAGENET_TRAIN_LEN, ds.IMAGENET_VAL_LEN = orig_train, orig_val

    out = capsys.readouterr().out
    assert "'drop_path_rate': 0.2" in out
    assert "training begins" in out and "training completed" in out
    losses = [float(v) for v in re.findall(r"loss: (\S+),", out)]
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses), out
    assert re.search(r"accuracy on val: \d", out)
    assert glob.glob(os.path.join(str(tmp_path), "epoch_1_rank_0.ckpt"))
