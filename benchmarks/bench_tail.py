#!/usr/bin/env python3
"""Memory-bound backward tail at the ViT-10B per-GPU shapes (32768 rows,
E = 5120, hid = 20480, 32 heads of 160): LayerNorm backward (plain and
fused-add), the attention backward's row dot, and GELU backward plus
the fc1 bias gradient.  Prints ms per call and effective TB/s, where
the bytes are the MINIMUM traffic of the op (each input read once, each
output written once), so a redundant pass shows up as lost bandwidth.
Every timing window is at least 1 s.  Run on an MI355X:

    python benchmarks/bench_tail.py
    python benchmarks/bench_tail.py --root /path/to/another/checkout

``--root`` imports the package (and its built _C) from another checkout,
so two builds can be compared in one session; entries a build does not
have are reported as absent.
"""

import argparse
import os
import sys
import time


def timed(fn, min_window=1.0):
    """ms per call over a window of at least ``min_window`` seconds."""
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.time()
    fn()
    torch.cuda.synchronize()
    one = max(time.time() - t0, 1e-5)
    iters = max(5, int(1.2 * min_window / one) + 1)
    while True:
        start, stop = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        ms = start.elapsed_time(stop)
        if ms >= 1e3 * min_window:
            return ms / iters
        iters *= 2


def report(name, ms, nbytes):
    print(f"{name:<44s} {ms:8.3f} ms  {nbytes / ms / 1e9:6.2f} TB/s "
          f"({nbytes / 1e6:.0f} MB min)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(
        os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--embed", type=int, default=5120)
    ap.add_argument("--hidden", type=int, default=20480)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=256)
    args = ap.parse_args()
    sys.path.insert(0, args.root)

    import torch
    import vit_10b_fsdp_example_amd._C as C

    assert torch.cuda.is_available()
    print(f"[bench_tail] package root {args.root}")
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    torch.manual_seed(0)
    n, e, hid = args.rows, args.embed, args.hidden
    act = n * e * 2  # bytes of one [rows, E] bf16 tensor

    # ---- LayerNorm backward -------------------------------------------
    x = torch.randn(n, e, device=dev, dtype=bf)
    dy = torch.randn_like(x)
    w = torch.randn(e, device=dev, dtype=bf)
    b = torch.randn(e, device=dev, dtype=bf)
    _, mean, rstd = C.layernorm_fwd(x, w, b, 1e-6)
    report("layernorm_bwd (dx, dw, db)",
           timed(lambda: C.layernorm_bwd(dy, x, w, mean, rstd)), 3 * act)
    dsum = torch.randn_like(x)
    report("layernorm_add_bwd (dx1, dx2, dw, db)",
           timed(lambda: C.layernorm_add_bwd(dy, dsum, x, w, mean, rstd)),
           5 * act)
    del dsum

    # ---- attention backward row dot -----------------------------------
    h, t = args.heads, args.tokens
    d = e // h
    bsz = n // t
    if hasattr(C, "fmha_rowdot"):
        do4 = dy.view(bsz, h, t, d)
        o4 = x.view(bsz, h, t, d)
        report("fmha_rowdot [B,H,T,D]",
               timed(lambda: C.fmha_rowdot(do4, o4)), 2 * act)
    else:
        print("fmha_rowdot: not exposed by this build (see the kernel trace)")
    qkv = torch.randn(bsz, t, 3, h, d, device=dev, dtype=bf)
    o, lse = C.fmha_fwd_qkv(qkv, h, d ** -0.5)
    do = dy.view(bsz, t, e)
    # whole backward (row dot + dq + dkv kernels): q, k, v, o, dO in,
    # dqkv out; the row dot is the only memory-bound part of it
    report("fmha_bwd_qkv (rowdot + dq + dkv)",
           timed(lambda: C.fmha_bwd_qkv(do, qkv, o, lse, h, d ** -0.5)),
           8 * act)
    del qkv, o, lse, x, dy

    # ---- GELU backward + fc1 bias gradient ----------------------------
    pre = torch.randn(n, hid, device=dev, dtype=bf)
    g = torch.randn_like(pre)
    big = n * hid * 2

    def stock():
        dx = torch.ops.aten.gelu_backward(g, pre, approximate="none")
        return dx, dx.sum(0, keepdim=True)

    report("aten.gelu_backward + sum(0)", timed(stock), 3 * big)
    report("aten.gelu_backward alone", timed(
        lambda: torch.ops.aten.gelu_backward(g, pre, approximate="none")),
        3 * big)
    if hasattr(C, "gelu_bwd_colsum"):
        report("gelu_bwd_colsum (dx, colsum)",
               timed(lambda: C.gelu_bwd_colsum(g, pre)), 3 * big)
    else:
        print("gelu_bwd_colsum: not in this build")


if __name__ == "__main__":
    main()
