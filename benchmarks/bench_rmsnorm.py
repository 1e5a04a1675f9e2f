#!/usr/bin/env python3
"""--norm_type rmsnorm at the ViT-10B per-GPU activation shape
((32768, 5120) bf16): the four entry points of csrc/rmsnorm.hip against

* the stock composition (ops.rms_norm / ops.fused_add_rms_norm with
  VITFSDP_NATIVE_RMSNORM=0, forward and autograd's backward), and
* layernorm_fwd / layernorm_add_fwd / layernorm_bwd / layernorm_add_bwd of
  the same build on the same tensors: the yardstick, since they move the
  same bytes with more arithmetic,

and one Block forward+backward with the flag at either value under the
training step's dispatch mode.

Everything runs in one process, in --series alternating series, every
timing window at least --window s.  Printed per entry: each series' ms,
the spread (max - min) / min between series, and TB/s of the best series
over the bytes the op must move (the [rows, D] tensors it reads and
writes once; statistics, gamma and the backward's fp32 partials are not
part of that minimum).  Run on an MI355X:

    python benchmarks/bench_rmsnorm.py
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_tail import timed  # noqa: E402


def stock(fn):
    """fn with the native route switched off: the stock composition."""
    def run():
        os.environ["VITFSDP_NATIVE_RMSNORM"] = "0"
        try:
            return fn()
        finally:
            del os.environ["VITFSDP_NATIVE_RMSNORM"]
    return run


def block_step(args, torch, norm_type):
    """One Block forward+backward at [batch, tokens, E]."""
    from vit_10b_fsdp_example_amd.models.vit import Block

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    blk = Block(args.embed, args.heads, norm_type=norm_type).to(
        dev, torch.bfloat16)
    blk.train()
    x = torch.randn(args.batch, args.tokens, args.embed, device=dev,
                    dtype=torch.bfloat16, requires_grad=True)
    dout = torch.randn_like(x)

    def step():
        blk(x).backward(dout)

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--embed", type=int, default=5120)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--skip_block", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(
        os.path.dirname(os.path.abspath(__file__))))

    import torch
    import vit_10b_fsdp_example_amd._C as C
    from vit_10b_fsdp_example_amd.ops import fused_add_rms_norm, rms_norm
    from vit_10b_fsdp_example_amd.ops.linear import gemm_dispatch_context

    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    rows, d, eps = args.batch * args.tokens, args.embed, 1e-6
    act = rows * d * 2  # bytes of one bf16 [rows, D] tensor
    x = torch.randn(rows, d, device=dev, dtype=torch.bfloat16)
    res = 0.5 * torch.randn_like(x)
    dy, dsum = torch.randn_like(x), torch.randn_like(x)
    w = (1 + 0.5 * torch.randn(d, device=dev)).bfloat16()
    b = (0.1 * torch.randn(d, device=dev)).bfloat16()
    _, rstd = C.rmsnorm_fwd(x, w, eps)
    _, mean, ln_rstd = C.layernorm_fwd(x, w, b, eps)

    # the composition: autograd graphs built once, backward retained
    xr, rr, wr = (t.clone().requires_grad_(True) for t in (x, res, w))
    y_c = stock(lambda: rms_norm(xr, wr, eps))()
    s_c, ya_c = stock(lambda: fused_add_rms_norm(xr, rr, wr, eps))()

    # name -> (fn, bytes the op must move), grouped as (ours, LN, stock)
    entries = {
        "rmsnorm_fwd": (lambda: C.rmsnorm_fwd(x, w, eps), 2 * act),
        "layernorm_fwd": (lambda: C.layernorm_fwd(x, w, b, eps), 2 * act),
        "stock fwd": (stock(lambda: rms_norm(x, w, eps)), 2 * act),
        "rmsnorm_add_fwd": (
            lambda: C.rmsnorm_add_fwd(x, res, w, eps), 4 * act),
        "layernorm_add_fwd": (
            lambda: C.layernorm_add_fwd(x, res, w, b, eps), 4 * act),
        "stock add fwd": (
            stock(lambda: fused_add_rms_norm(x, res, w, eps)), 4 * act),
        "rmsnorm_bwd": (lambda: C.rmsnorm_bwd(dy, x, w, rstd), 3 * act),
        "layernorm_bwd": (
            lambda: C.layernorm_bwd(dy, x, w, mean, ln_rstd), 3 * act),
        "stock bwd": (lambda: torch.autograd.grad(
            y_c, (xr, wr), dy, retain_graph=True), 3 * act),
        "rmsnorm_add_bwd": (
            lambda: C.rmsnorm_add_bwd(dy, dsum, x, w, rstd), 5 * act),
        "layernorm_add_bwd": (
            lambda: C.layernorm_add_bwd(dy, dsum, x, w, mean, ln_rstd),
            5 * act),
        "stock add bwd": (lambda: torch.autograd.grad(
            (s_c, ya_c), (xr, rr, wr), (dsum, dy), retain_graph=True),
            5 * act),
    }
    if not args.skip_block:
        for norm_type in ("layernorm", "rmsnorm"):
            entries[f"Block fwd+bwd norm_type={norm_type}"] = (
                block_step(args, torch, norm_type), 0)

    ms = {name: [] for name in entries}
    for s in range(args.series):
        for name, (fn, nbytes) in entries.items():
            if nbytes:
                ms[name].append(timed(fn, args.window))
            else:  # the Block, under the training step's dispatch mode
                with gemm_dispatch_context():
                    ms[name].append(timed(fn, args.window))
        print(f"series {s + 1} of {args.series} done", flush=True)

    def spread(name):
        return (max(ms[name]) - min(ms[name])) / min(ms[name])

    for name, (_, nbytes) in entries.items():
        best = min(ms[name])
        series = " ".join(f"{v:7.3f}" for v in ms[name])
        tbs = f"{nbytes / best / 1e9:5.2f} TB/s" if nbytes else ""
        print(f"{name:<36s} {series} ms  spread {100 * spread(name):4.1f} %  "
              f"{tbs}", flush=True)

    n_part = min(rows, 768)
    print(f"rmsnorm_bwd partials: {n_part} x {d} fp32, "
          f"{2 * n_part * d * 4 / 1e6:.1f} MB written and read "
          f"(LayerNorm's: twice that)")
    for op in ("fwd", "add_fwd", "bwd", "add_bwd"):
        ours, ln = f"rmsnorm_{op}", f"layernorm_{op}"
        theirs = "stock " + op.replace("_", " ")
        print(f"{ours}: {min(ms[ours]) / min(ms[ln]):.3f} x {ln} (best "
              f"series each; its spread {100 * spread(ln):.1f} %, ours "
              f"{100 * spread(ours):.1f} %); worst {max(ms[ours]):.3f} ms "
              f"against the composition's best {min(ms[theirs]):.3f} ms")


if __name__ == "__main__":
    main()
