#!/usr/bin/env python3
"""Patch dropout at the ViT-10B per-GPU front-end shape (B = 128, T = 256,
E = 5120, rate 0.25 and 0.5): the three kernels of csrc/patch_drop.hip
against the stock composition they replace (rand / argsort / sort for the
plan; indexing, add and hidden_dropout for the embed; autograd's
index_put for its backward), and one training step of a small model at
rate 0, 0.25 and 0.5.

The two sides of a comparison are timed in ALTERNATING series in one
process, --reps windows of at least 1 s each per side; the median is
printed with the spread (min .. max) of the windows.  Run on an MI355X:

    python benchmarks/bench_patch_drop.py
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_tail import timed  # noqa: E402


def alternate(name, sides, reps):
    """Time each callable of ``sides`` (label -> fn) in turn, reps times;
    print median and spread per side; return the medians."""
    series = {label: [] for label in sides}
    for _ in range(reps):
        for label, fn in sides.items():
            series[label].append(timed(fn))
    med = {k: statistics.median(v) for k, v in series.items()}
    for label, v in series.items():
        print(f"{name:<34s} {label:<7s} {med[label]:9.4f} ms  "
              f"({min(v):.4f} .. {max(v):.4f})", flush=True)
    if len(med) == 2:
        a, b = med.values()
        print(f"{'':<34s} ratio   {a / b:9.3f}", flush=True)
    return med


def step_ms(args, torch, rate):
    """One training step (forward, backward, clip, AdamW) of the small
    model at patch_drop_rate = rate."""
    from vit_10b_fsdp_example_amd import dist as xdist
    from vit_10b_fsdp_example_amd.cli import parse_args
    from vit_10b_fsdp_example_amd.models import build_fsdp_vit_model
    from vit_10b_fsdp_example_amd.ops import CrossEntropyLoss, FusedAdamW
    from vit_10b_fsdp_example_amd.parallel import CommContext

    CommContext.reset()
    cfg = parse_args([
        "--fake_data", "--embed_dim", str(args.step_embed), "--num_heads",
        str(args.step_heads), "--num_blocks", str(args.step_blocks),
        "--batch_size", str(args.step_batch), "--num_workers", "0",
        "--patch_drop_rate", str(rate),
    ])
    device = xdist.init_distributed()
    torch.manual_seed(0)
    model = build_fsdp_vit_model(cfg, device, compute_dtype=torch.bfloat16)
    loss_fn = CrossEntropyLoss()
    opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.1)
    x = torch.randn(args.step_batch, 3, 224, 224, device=device,
                    dtype=torch.bfloat16)
    y = torch.randint(0, 1000, (args.step_batch,), device=device)

    def step():
        loss_fn(model(x), y).backward()
        model.clip_grad_norm_(1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--embed", type=int, default=5120)
    ap.add_argument("--p_elem", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step_embed", type=int, default=1280)
    ap.add_argument("--step_heads", type=int, default=8)
    ap.add_argument("--step_blocks", type=int, default=4)
    ap.add_argument("--step_batch", type=int, default=64)
    ap.add_argument("--skip_step", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(
        os.path.dirname(os.path.abspath(__file__))))

    import torch
    from vit_10b_fsdp_example_amd.ops import (
        patch_drop_embed, patch_drop_plan,
    )

    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    B, T, E = args.batch, args.tokens, args.embed

    def both(fn):
        """fn on the native path and on the stock composition."""
        def stock():
            os.environ["VITFSDP_NATIVE_DROPOUT"] = "0"
            try:
                return fn()
            finally:
                del os.environ["VITFSDP_NATIVE_DROPOUT"]
        return {"native": fn, "stock": stock}

    for rate in (0.25, 0.5):
        K = max(1, int(T * (1.0 - rate)))
        print(f"--- rate {rate}: B={B} T={T} K={K} E={E}", flush=True)
        alternate("plan", both(lambda: patch_drop_plan(B, T, K, dev)),
                  args.reps)
        idx, inv = patch_drop_plan(B, T, K, dev, seed=1)
        proj = torch.randn(B, K, E, device=dev, dtype=torch.bfloat16,
                           requires_grad=True)
        pos = torch.randn(1, T, E, device=dev, dtype=torch.bfloat16,
                          requires_grad=True)
        dy = torch.randn(B, K, E, device=dev, dtype=torch.bfloat16)
        for p in (0.0, args.p_elem):
            sides = both(
                lambda: patch_drop_embed(proj, pos, idx, inv, p, True))
            alternate(f"embed fwd p={p}", sides, args.reps)
            # the backward alone, on a graph built once per side
            outs = {label: fn() for label, fn in sides.items()}
            alternate(f"embed bwd p={p}", {
                label: (lambda out=out: torch.autograd.grad(
                    out, (proj, pos), dy, retain_graph=True))
                for label, out in outs.items()}, args.reps)
            del outs
        del proj, pos, dy
        torch.cuda.empty_cache()

    if not args.skip_step:
        print(f"--- training step: embed {args.step_embed}, "
              f"{args.step_blocks} blocks, batch {args.step_batch}",
              flush=True)
        for rate in (0.0, 0.25, 0.5):
            step = step_ms(args, torch, rate)
            alternate(f"step rate={rate}", {"native": step}, args.reps)
            del step
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
