#!/usr/bin/env python3
"""--qk_norm at the ViT-10B per-GPU shape ([128, 256, 3, 32, 160], i.e.
(B*T, H, D) = (32768, 32, 160)):

1. the two kernels of csrc/qk_norm.hip against the stock composition on
   the same tensors (F.layer_norm on the strided q and k views + stack,
   and autograd's backward of exactly that);
2. the bandwidth each kernel reaches over its MINIMUM traffic: with
   A = bytes of one [B*T, H, D] slice, the forward reads 3 A and writes
   3 A (v is copied), the backward reads dq, dk, q, k (4 A) and writes
   dq, dk (2 A); statistics and partials are below 1 % of that;
3. one Block forward+backward with the flag off and on, under the
   training step's dispatch mode, alternating so that clock drift hits
   both alike.

Every figure is the median of --repeats windows of at least --window
seconds each, with the spread (max - min) / median of the series next to
it.  Run on an MI355X:

    python benchmarks/bench_qk_norm.py

--type rmsnorm does the same for --qk_norm_type rmsnorm
(csrc/qk_rmsnorm.hip), at that shape and at (128, 256, 16, 80), a head dim
that two lanes per row serve: the two kernels against the composition
(fp32 statistics on the strided q and k views + stack) and, where they
exist for the head dim, against the LayerNorm kernels, which move the same
bytes; then one Block forward+backward with the backward's second norm
forward (VITFSDP_QK_NORM_RECOMPUTE) on and off, and the bytes each setting
saves for the backward.  The candidates of a comparison alternate window
by window.

    python benchmarks/bench_qk_norm.py --type rmsnorm
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_tail import timed  # noqa: E402


def series(fn, args):
    return [timed(fn, args.window) for _ in range(args.repeats)]


def show(name, ms_series, nbytes=None):
    med = statistics.median(ms_series)
    spread = (max(ms_series) - min(ms_series)) / med
    rate = f"  {nbytes / med / 1e9:5.2f} TB/s" if nbytes else ""
    print(f"{name:<40s} {med:8.3f} ms  spread {100 * spread:4.1f} %{rate}  "
          f"[{' '.join(f'{v:.3f}' for v in ms_series)}]", flush=True)
    return med


def kernels(args, torch, C):
    import torch.nn.functional as F

    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    B, T, H, D = args.batch, args.tokens, args.heads, args.embed // args.heads
    a = B * T * H * D * 2  # bytes of one slice
    qkv = torch.randn(B, T, 3, H, D, device=dev, dtype=bf, requires_grad=True)
    dout = torch.randn(B, T, 3, H, D, device=dev, dtype=bf)
    params = [torch.randn(D, device=dev, dtype=bf, requires_grad=True)
              for _ in range(4)]
    wq, bq, wk, bk = params
    eps = 1e-6

    def stock():
        q, k, v = qkv.unbind(2)
        return torch.stack((F.layer_norm(q, (D,), wq, bq, eps),
                            F.layer_norm(k, (D,), wk, bk, eps), v), dim=2)

    with torch.no_grad():
        ours = show("qk_norm_fwd", series(
            lambda: C.qk_norm_fwd(qkv, wq, bq, wk, bk, eps), args), 6 * a)
        theirs = show("stock forward (2 LN + stack)", series(stock, args))
    print(f"    kernel / stock: {ours / theirs:.3f}", flush=True)

    _, mean, rstd = C.qk_norm_fwd(qkv.detach(), wq, bq, wk, bk, eps)
    work = dout.clone()  # overwritten in place; the values do not matter
    with torch.no_grad():
        ours = show("qk_norm_bwd (+ final sum)", series(
            lambda: C.qk_norm_bwd(work, qkv, wq, wk, mean, rstd), args), 6 * a)
    out = stock()
    theirs = show("stock backward (autograd)", series(
        lambda: torch.autograd.grad(out, [qkv] + params, dout,
                                    retain_graph=True), args))
    print(f"    kernel / stock: {ours / theirs:.3f}", flush=True)


def alternating(fns, args):
    """{name: series}: one window of each candidate per round"""
    ms = {name: [] for name in fns}
    for _ in range(args.repeats):
        for name, fn in fns.items():
            ms[name].append(timed(fn, args.window))
    return ms


def rms_kernels(args, torch, C, heads, D):
    from vit_10b_fsdp_example_amd.ops.attention import QK_NORM_HEAD_DIMS
    from vit_10b_fsdp_example_amd.ops.rmsnorm import _composition

    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    B, T, eps = args.batch, args.tokens, 1e-6
    a = B * T * heads * D * 2  # bytes of one slice
    print(f"(B, T, H, D) = ({B}, {T}, {heads}, {D})", flush=True)
    qkv = torch.randn(B, T, 3, heads, D, device=dev, dtype=bf,
                      requires_grad=True)
    dout = torch.randn(B, T, 3, heads, D, device=dev, dtype=bf)
    wq, bq, wk, bk = (torch.randn(D, device=dev, dtype=bf, requires_grad=True)
                      for _ in range(4))
    work = dout.clone()  # overwritten in place; the values do not matter
    layernorm = D in QK_NORM_HEAD_DIMS

    def stock():
        q, k, v = qkv.unbind(2)
        return torch.stack((_composition(q, wq, eps),
                            _composition(k, wk, eps), v), dim=2)

    fwd = {"qk_rmsnorm_fwd": lambda: C.qk_rmsnorm_fwd(qkv, wq, wk, eps)}
    _, rstd = C.qk_rmsnorm_fwd(qkv.detach(), wq, wk, eps)
    bwd = {"qk_rmsnorm_bwd (+ final sum)":
           lambda: C.qk_rmsnorm_bwd(work, qkv, wq, wk, rstd)}
    if layernorm:
        fwd["qk_norm_fwd"] = lambda: C.qk_norm_fwd(qkv, wq, bq, wk, bk, eps)
        _, mean, ln_rstd = C.qk_norm_fwd(qkv.detach(), wq, bq, wk, bk, eps)
        bwd["qk_norm_bwd (+ final sum)"] = lambda: C.qk_norm_bwd(
            work, qkv, wq, wk, mean, ln_rstd)
    else:
        print(f"    no LayerNorm kernels at D = {D}", flush=True)
    fwd["composition forward"] = stock
    out = stock()
    bwd["composition backward (autograd)"] = lambda: torch.autograd.grad(
        out, [qkv, wq, wk], dout, retain_graph=True)
    for fns in (fwd, bwd):
        with torch.no_grad():
            kernel_ms = alternating(
                {k: f for k, f in fns.items() if "composition" not in k}, args)
        med = {k: show(k, v, 6 * a) for k, v in kernel_ms.items()}
        comp = [k for k in fns if "composition" in k][0]
        med[comp] = show(comp, series(fns[comp], args))
        ours = med[next(iter(fns))]
        for k, v in list(med.items())[1:]:
            print(f"    rmsnorm kernel / {k}: {ours / v:.3f}", flush=True)


def rms_block(args, torch):
    from vit_10b_fsdp_example_amd.models.vit import Block
    from vit_10b_fsdp_example_amd.ops.linear import gemm_dispatch_context

    dev = torch.device("cuda", 0)
    x = torch.randn(args.batch, args.tokens, args.embed, device=dev,
                    dtype=torch.bfloat16, requires_grad=True)
    dy = torch.randn_like(x)
    torch.manual_seed(0)
    blk = Block(args.embed, args.heads, qk_norm=True,
                qk_norm_type="rmsnorm").to(dev, torch.bfloat16).train()
    settings = {"recompute on": "1", "recompute off": "0"}
    ms, saved = {k: [] for k in settings}, {}
    with gemm_dispatch_context() as mode:
        for name, value in settings.items():
            os.environ["VITFSDP_QK_NORM_RECOMPUTE"] = value
            sizes = {}  # by storage: a tensor saved twice counts once

            def pack(t):
                store = t.untyped_storage()
                sizes[store.data_ptr()] = store.nbytes()
                return t

            with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
                blk(x).backward(dy)
            saved[name] = sum(sizes.values())
        for _ in range(args.repeats):
            for name, value in settings.items():
                os.environ["VITFSDP_QK_NORM_RECOMPUTE"] = value
                ms[name].append(timed(lambda: blk(x).backward(dy),
                                      args.window))
    print(f"Block forward+backward, qk_norm_type rmsnorm, under "
          f"{type(mode).__name__}:")
    on = show("  recompute on", ms["recompute on"])
    off = show("  recompute off", ms["recompute off"])
    print(f"    on - off: {on - off:+.3f} ms ({100 * (on / off - 1):+.2f} %)")
    for name, nbytes in saved.items():
        print(f"    saved for the backward, {name}: {nbytes / 2**20:.1f} MiB")
    print(f"    off - on: "
          f"{(saved['recompute off'] - saved['recompute on']) / 2**20:.1f} "
          f"MiB per block", flush=True)


def block(args, torch):
    from vit_10b_fsdp_example_amd.models.vit import Block
    from vit_10b_fsdp_example_amd.ops.linear import gemm_dispatch_context

    dev = torch.device("cuda", 0)
    x = torch.randn(args.batch, args.tokens, args.embed, device=dev,
                    dtype=torch.bfloat16, requires_grad=True)
    dy = torch.randn_like(x)
    steps, ms = {}, {False: [], True: []}
    for flag in (False, True):
        torch.manual_seed(0)
        blk = Block(args.embed, args.heads, qk_norm=flag).to(
            dev, torch.bfloat16).train()
        steps[flag] = lambda blk=blk: blk(x).backward(dy)
    with gemm_dispatch_context() as mode:
        for _ in range(args.repeats):
            for flag in (False, True):
                ms[flag].append(timed(steps[flag], args.window))
    print(f"Block forward+backward under {type(mode).__name__}:")
    off = show("  qk_norm off", ms[False])
    on = show("  qk_norm on", ms[True])
    print(f"    on - off: {on - off:+.3f} ms ({100 * (on / off - 1):+.2f} %)",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--embed", type=int, default=5120)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--skip_block", action="store_true")
    ap.add_argument("--type", choices=("layernorm", "rmsnorm"),
                    default="layernorm")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(
        os.path.dirname(os.path.abspath(__file__))))

    import torch
    import vit_10b_fsdp_example_amd._C as C

    assert torch.cuda.is_available()
    torch.manual_seed(0)
    if args.type == "rmsnorm":
        rms_kernels(args, torch, C, args.heads, args.embed // args.heads)
        torch.cuda.empty_cache()
        rms_kernels(args, torch, C, args.heads // 2,
                    args.embed // args.heads // 2)
        torch.cuda.empty_cache()
        if not args.skip_block:
            rms_block(args, torch)
        return
    kernels(args, torch, C)
    torch.cuda.empty_cache()
    if not args.skip_block:
        block(args, torch)


if __name__ == "__main__":
    main()
