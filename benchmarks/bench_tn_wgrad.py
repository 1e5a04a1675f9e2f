#!/usr/bin/env python3
"""Weight gradient dW[out, in] = dY^T X as a library TN GEMM on
transposed operands, against today's path, at the four ViT-10B shapes
(K = 32768 tokens).  Per shape:

  (a) today: the NT GEMM (`lt_gemm(dy.t(), x, tuned index)` for fc1/fc2,
      `_C.wgrad_gemm` for qkv/proj) plus `dy.sum(0)` for the bias;
  (b) the TN GEMM alone, `lt_gemm(dyT, xT.t(), idx)`, for the library
      heuristic (-1) and every index in ``--indices`` (default: the T,N
      rows of tuned/lt_algos_gfx950.json, all of which have run on
      MI355X; an index that does not validate falls back to the
      heuristic inside lt_gemm);
  (c) the whole new path: `transpose_colsum(dy)` + `transpose2d(x)` +
      the best GEMM of (b).

Method as in bench_wgemm.py: 4 rotating operand sets (past the 256 MB
L3), every timing window at least 1 s; ms per call and TF/s.  The
transposes are also reported in TB/s (one read + one write) next to
`dropout_fwd` on the same tensor as the streaming yardstick.

    python benchmarks/bench_tn_wgrad.py
    python benchmarks/bench_tn_wgrad.py --root /path/to/another/checkout

Last, at [tokens, 20480]: `gelu_bwd_colsum`, the same followed by
`transpose2d(dx)`, and `gelu_bwd_colsum_t`, which writes dx^T itself.

``--root`` imports the package (and its built _C) from another checkout;
a build without the transpose kernels reports (a) and (b) only.
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_tail import timed  # noqa: E402

# name: (out, in); dy is [K, out], x is [K, in]
SHAPES = {
    "qkv": (15360, 5120),
    "proj": (5120, 5120),
    "fc1": (20480, 5120),
    "fc2": (5120, 20480),
}
NATIVE_NT = ("qkv", "proj")  # shapes today's step runs on csrc/wgemm.hip


def rotating(fn, sets):
    """Call fn on the next of the operand sets each time."""
    state = {"i": 0}

    def call():
        s = sets[state["i"] % len(sets)]
        state["i"] += 1
        return fn(*s)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(
        os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--shapes", default="qkv,proj,fc1,fc2")
    ap.add_argument("--indices", default=None,
                    help="comma-separated library indices for (b)")
    ap.add_argument("--window", type=float, default=1.0)
    args = ap.parse_args()
    sys.path.insert(0, args.root)

    import torch
    import vit_10b_fsdp_example_amd._C as C
    from vit_10b_fsdp_example_amd.tuning import lt_algo_table

    assert torch.cuda.is_available()
    print(f"[bench_tn_wgrad] package root {args.root}")
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    table = lt_algo_table()
    if args.indices is None:
        cand = sorted({v for k, v in table.items() if k[:2] == ("T", "N")})
    else:
        cand = [int(s) for s in args.indices.split(",") if s]
    have_tr = hasattr(C, "transpose2d")
    K = args.tokens
    win = args.window

    for name in [s for s in args.shapes.split(",") if s]:
        out, inn = SHAPES[name]
        fl = 2.0 * K * out * inn
        torch.manual_seed(0)
        sets = [(torch.randn(K, out, device=dev, dtype=bf),
                 torch.randn(K, inn, device=dev, dtype=bf)) for _ in range(4)]
        print(f"--- {name}: dW [{out}, {inn}], K = {K}", flush=True)

        def line(tag, ms, extra=""):
            print(f"{name:5s} {tag:<34s} {ms:8.3f} ms {fl / ms / 1e9:7.0f} TF/s"
                  f" {extra}", flush=True)

        # (a) today's path
        if name in NATIVE_NT:
            nt = rotating(lambda dy, x: C.wgrad_gemm(dy, x, False), sets)
            tag = "(a) wgrad_gemm NT"
        else:
            idx_nt = table.get(("N", "T", inn, out, K), -1)
            nt = rotating(lambda dy, x: C.lt_gemm(dy.t(), x, idx_nt), sets)
            tag = f"(a) library NT idx {idx_nt}"
        a_gemm = timed(nt, win)
        a_sum = timed(rotating(lambda dy, x: dy.sum(0), sets), win)
        line(tag, a_gemm)
        line("(a) dy.sum(0)", a_sum)
        line("(a) total", a_gemm + a_sum)

        # (b) TN GEMM alone on pre-transposed operands
        tsets = [(dy.t().contiguous(), x.t().contiguous()) for dy, x in sets]
        ref = sets[0][0].float().t() @ sets[0][1].float()
        best = None
        for idx in [-1] + cand:
            got = C.lt_gemm(tsets[0][0], tsets[0][1].t(), idx)
            rel = ((got.float() - ref).abs().max() / ref.abs().max()).item()
            ms = timed(rotating(
                lambda dyT, xT, i=idx: C.lt_gemm(dyT, xT.t(), i), tsets), win)
            line(f"(b) library TN idx {idx}", ms, f"rel_err {rel:.4f}")
            if best is None or ms < best[1]:
                best = (idx, ms)
        del ref, got
        print(f"{name:5s} (b) best idx {best[0]} {best[1]:.3f} ms "
              f"key T,N,{inn},{out},{K}", flush=True)

        if not have_tr:
            print(f"{name:5s} (c) transpose kernels: not in this build")
            del sets, tsets
            torch.cuda.empty_cache()
            continue

        # (c) transposes + best (b)
        dy0, x0 = sets[0]
        assert torch.equal(C.transpose2d(x0), tsets[0][1])
        dyT0, cs0 = C.transpose_colsum(dy0)
        assert torch.equal(dyT0, tsets[0][0])
        cs_err = (cs0.double() - dy0.double().sum(0)).abs().max().item()
        del dyT0, tsets
        torch.cuda.empty_cache()
        by_dy, by_x = 2 * K * out * 2, 2 * K * inn * 2
        t_dy = timed(rotating(lambda dy, x: C.transpose_colsum(dy), sets), win)
        t_dy0 = timed(rotating(lambda dy, x: C.transpose2d(dy), sets), win)
        t_x = timed(rotating(lambda dy, x: C.transpose2d(x), sets), win)
        d_dy = timed(rotating(lambda dy, x: C.dropout_fwd(dy, 0.1, 1), sets),
                     win)
        d_x = timed(rotating(lambda dy, x: C.dropout_fwd(x, 0.1, 1), sets), win)
        print(f"{name:5s} transpose_colsum(dy [{K},{out}]) {t_dy:7.3f} ms "
              f"{by_dy / t_dy / 1e9:5.2f} TB/s | transpose2d(dy) {t_dy0:7.3f} "
              f"ms {by_dy / t_dy0 / 1e9:5.2f} TB/s | dropout_fwd {d_dy:7.3f} ms"
              f" {by_dy / d_dy / 1e9:5.2f} TB/s | colsum max err {cs_err:.3g}",
              flush=True)
        print(f"{name:5s} transpose2d(x [{K},{inn}]) {t_x:7.3f} ms "
              f"{by_x / t_x / 1e9:5.2f} TB/s | dropout_fwd {d_x:7.3f} ms "
              f"{by_x / d_x / 1e9:5.2f} TB/s", flush=True)

        def new_path(dy, x, i=best[0]):
            dyT, colsum = C.transpose_colsum(dy)
            xT = C.transpose2d(x)
            return C.lt_gemm(dyT, xT.t(), i), colsum

        c_ms = timed(rotating(new_path, sets), win)
        line(f"(c) transposes + TN idx {best[0]}", c_ms,
             f"vs (a) total {a_gemm + a_sum:.3f} ms, "
             f"vs (a) GEMM alone {a_gemm:.3f} ms")
        del sets, dy0, x0
        torch.cuda.empty_cache()

    # fc1's dy^T: a third output of the GELU backward, or a transpose of
    # its result afterwards
    hid = SHAPES["fc1"][0]
    if hasattr(C, "gelu_bwd_colsum_t"):
        gsets = [(torch.randn(K, hid, device=dev, dtype=bf),
                  torch.randn(K, hid, device=dev, dtype=bf)) for _ in range(4)]
        dx0, cs0 = C.gelu_bwd_colsum(*gsets[0])
        dx1, cs1, dxt1 = C.gelu_bwd_colsum_t(*gsets[0])
        assert torch.equal(dx0, dx1) and torch.equal(cs0, cs1)
        assert torch.equal(dxt1, C.transpose2d(dx0))
        del dx0, cs0, dx1, cs1, dxt1

        def two_pass(g, pre):
            dx, cs = C.gelu_bwd_colsum(g, pre)
            return dx, cs, C.transpose2d(dx)

        print(f"--- GELU backward at [{K}, {hid}]", flush=True)
        for rep in range(2):  # alternate, twice
            for tag, fn in (
                    ("gelu_bwd_colsum", lambda g, pre: C.gelu_bwd_colsum(g, pre)),
                    ("gelu_bwd_colsum + transpose2d(dx)", two_pass),
                    ("gelu_bwd_colsum_t", lambda g, pre: C.gelu_bwd_colsum_t(g, pre))):
                print(f"gelu  {tag:<36s} {timed(rotating(fn, gsets), win):8.3f} ms",
                      flush=True)


if __name__ == "__main__":
    main()
