#!/usr/bin/env python3
"""Hidden dropout at the ViT-10B per-GPU shapes (32768 rows, E = 5120,
hid = 20480, p = 0.1): each op of csrc/dropout.hip, forward and
backward, next to the stock torch composition it replaces; the
GELU+dropout backward together with fc1's bias sums and dx^T, as two
passes and as the one pass of gelu_dropout_bwd_colsum(_t)
(``--only_gelu_bwd`` runs just these and the Block time); and the peak
memory and the time of one Block forward+backward with hidden dropout
on.  Prints ms
per call and effective TB/s, where the bytes are the MINIMUM traffic of
the op (each input read once, each output written once; no mask), so
the stock path's extra passes and its mask show up as lost bandwidth.
Every timing window is at least 1 s.  Run on an MI355X:

    python benchmarks/bench_dropout.py
    python benchmarks/bench_dropout.py --root /path/to/another/checkout

``--root`` imports the package (and its built _C) from another checkout,
so two builds can be compared in one session; entries a build does not
have are reported as absent.
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_tail import report, timed  # noqa: E402


def block_peak_mb(args, torch):
    """Peak allocation above the resident state of one Block
    forward+backward at [rows/tokens, tokens, E] with drop = p."""
    from vit_10b_fsdp_example_amd.models.vit import Block

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    blk = Block(args.embed, args.heads, drop=args.p).to(dev, torch.bfloat16)
    blk.train()
    x = torch.randn(args.rows // args.tokens, args.tokens, args.embed,
                    device=dev, dtype=torch.bfloat16, requires_grad=True)
    peaks = []
    for _ in range(2):  # first pass warms the GEMM workspaces
        blk.zero_grad(set_to_none=True)
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = blk(x)
        out.backward(out.detach())
        torch.cuda.synchronize()
        peaks.append((torch.cuda.max_memory_allocated() - base) / 1e6)
        del out
    return peaks[-1]


def block_ms(args, torch):
    """ms of one Block forward+backward at [rows/tokens, tokens, E] with
    drop = p, under the training step's dispatch mode."""
    from vit_10b_fsdp_example_amd.models.vit import Block
    from vit_10b_fsdp_example_amd.ops.linear import gemm_dispatch_context

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    blk = Block(args.embed, args.heads, drop=args.p).to(dev, torch.bfloat16)
    blk.train()
    x = torch.randn(args.rows // args.tokens, args.tokens, args.embed,
                    device=dev, dtype=torch.bfloat16, requires_grad=True)
    dout = torch.randn_like(x)

    def step():
        out = blk(x)
        out.backward(dout)

    with gemm_dispatch_context() as mode:
        ms = timed(step)
    routed = {k: v for k, v in (vars(mode) if mode else {}).items()
              if k in ("dgelu_drop_hits", "dbias_hits", "tn_hits")}
    print(f"Block fwd+bwd, drop={args.p}, {type(mode).__name__}: "
          f"{ms:8.3f} ms  (routed in all: {routed})", flush=True)


def gelu_bwd_with_sums(args, torch, C):
    """The backward of dropout(gelu(x)) at [rows, hid] together with what
    fc1's gradients need of its result: the column sums (bias gradient)
    and, on the TN weight-gradient route, dx^T.  As two passes, and as
    the one pass of gelu_dropout_bwd_colsum(_t)."""
    dev = torch.device("cuda", 0)
    n, hid, p = args.rows, args.hidden, args.p
    big = n * hid * 2
    pre = torch.randn(n, hid, device=dev, dtype=torch.bfloat16)
    g = torch.randn_like(pre)
    if not hasattr(C, "gelu_dropout_bwd"):
        print("gelu_dropout_bwd: not in this build")
        return

    def bwd_then_sum():
        return C.gelu_dropout_bwd(g, pre, p, 1234).sum(0)

    def bwd_then_transpose_colsum():
        return C.transpose_colsum(C.gelu_dropout_bwd(g, pre, p, 1234))

    report("gelu_dropout_bwd + sum(0)", timed(bwd_then_sum), 3 * big)
    if hasattr(C, "gelu_dropout_bwd_colsum"):
        report("gelu_dropout_bwd_colsum (dx, colsum)", timed(
            lambda: C.gelu_dropout_bwd_colsum(g, pre, p, 1234)), 3 * big)
    else:
        print("gelu_dropout_bwd_colsum: not in this build")
    report("gelu_dropout_bwd + transpose_colsum",
           timed(bwd_then_transpose_colsum), 4 * big)
    if hasattr(C, "gelu_dropout_bwd_colsum_t"):
        report("gelu_dropout_bwd_colsum_t (dx, colsum, dx^T)", timed(
            lambda: C.gelu_dropout_bwd_colsum_t(g, pre, p, 1234)), 4 * big)
    else:
        print("gelu_dropout_bwd_colsum_t: not in this build")
    del pre, g
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(
        os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--embed", type=int, default=5120)
    ap.add_argument("--hidden", type=int, default=20480)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--skip_block", action="store_true")
    ap.add_argument("--only_gelu_bwd", action="store_true",
                    help="only the GELU+dropout backward with its sums and "
                         "transpose, as two passes and as one")
    args = ap.parse_args()
    sys.path.insert(0, args.root)

    import torch
    import torch.nn.functional as F
    import vit_10b_fsdp_example_amd._C as C

    assert torch.cuda.is_available()
    print(f"[bench_dropout] package root {args.root}")
    if args.only_gelu_bwd:
        gelu_bwd_with_sums(args, torch, C)
        if not args.skip_block:
            block_ms(args, torch)
        return
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    torch.manual_seed(0)
    n, e, hid, p = args.rows, args.embed, args.hidden, args.p
    act = n * e * 2    # bytes of one [rows, E] bf16 tensor
    big = n * hid * 2  # ... and of one [rows, hid]
    native = hasattr(C, "dropout_fwd")
    if not native:
        print("dropout_fwd, dropout_add_fwd, gelu_dropout_fwd/bwd: "
              "not in this build")

    # ---- [rows, E]: projection / pos-embed dropout, MLP residual add ---
    x = torch.randn(n, e, device=dev, dtype=bf)
    res = torch.randn_like(x)
    dy = torch.randn_like(x)

    report("stock dropout fwd", timed(lambda: F.dropout(x, p, True)), 2 * act)
    xr = x.clone().requires_grad_(True)
    y = F.dropout(xr, p, True)
    report("stock dropout bwd", timed(
        lambda: torch.autograd.grad(y, xr, dy, retain_graph=True)), 2 * act)
    del y
    report("stock x + dropout(res) fwd",
           timed(lambda: x + F.dropout(res, p, True)), 3 * act)
    if native:
        # the backward of dropout and of dropout_add's res is this call
        report("dropout_fwd (= its backward)",
               timed(lambda: C.dropout_fwd(x, p, 1234)), 2 * act)
        report("dropout_add_fwd",
               timed(lambda: C.dropout_add_fwd(x, res, p, 1234)), 3 * act)
    del x, res, dy, xr

    # ---- [rows, hid]: fc1 -> GELU -> dropout ---------------------------
    pre = torch.randn(n, hid, device=dev, dtype=bf)
    g = torch.randn_like(pre)
    report("stock dropout(gelu(x)) fwd",
           timed(lambda: F.dropout(F.gelu(pre), p, True)), 2 * big)
    pr = pre.clone().requires_grad_(True)
    y = F.dropout(F.gelu(pr), p, True)
    report("stock dropout(gelu(x)) bwd", timed(
        lambda: torch.autograd.grad(y, pr, g, retain_graph=True)), 3 * big)
    del y, pr
    if native:
        report("gelu_dropout_fwd",
               timed(lambda: C.gelu_dropout_fwd(pre, p, 1234)), 2 * big)
        report("gelu_dropout_bwd",
               timed(lambda: C.gelu_dropout_bwd(g, pre, p, 1234)), 3 * big)
    del pre, g
    torch.cuda.empty_cache()

    gelu_bwd_with_sums(args, torch, C)

    if not args.skip_block:
        mb = block_peak_mb(args, torch)
        print(f"Block fwd+bwd peak above resident, drop={p}: {mb:.0f} MB",
              flush=True)
        block_ms(args, torch)


if __name__ == "__main__":
    main()
