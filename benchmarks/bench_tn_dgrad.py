#!/usr/bin/env python3
"""Input gradient dX[tok, in] = dY[tok, out] W[out, in] as a library TN
GEMM on a transposed weight, against today's NN GEMM, at the four
ViT-10B shapes (32768 token rows).  Per shape:

  (a) today: `lt_gemm(dy, W, idx)` with the tabled N,N index;
  (b) the TN GEMM alone on a prebuilt W^T, `lt_gemm(dy, WT.t(), idx)`,
      for the library heuristic (-1) and the tabled T,N index of the
      dual key ("T","N", in, tok, out), or every tabled T,N index when
      that key has no entry (more with ``--indices``);
  (c) `_C.dgrad_tn(dy, W, idx)`, the weight transpose included, with the
      best index of (b);

and `transpose2d(W)` alone in ms and TB/s (one read + one write).

Method as in bench_tn_wgrad.py: 4 rotating operand sets (past the 256 MB
L3), every timing window at least 1 s, ms per call and TF/s.  The
weights are views at a 16-byte offset into a flat buffer, as in the
step.  Max abs error of (a) and (c) against the fp64 product of the same
bf16 inputs is printed for the first ``--check-rows`` rows.

    python benchmarks/bench_tn_dgrad.py
    python benchmarks/bench_tn_dgrad.py --root /path/to/another/checkout

``--root`` imports the package (and its built _C) from another checkout;
a build without `dgrad_tn` reports (a), (b) and the transpose only.
"""

import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_tail import timed  # noqa: E402
from bench_tn_wgrad import rotating  # noqa: E402

# name: (out, in); dy is [tok, out], W is [out, in]
SHAPES = {
    "qkv": (15360, 5120),
    "proj": (5120, 5120),
    "fc1": (20480, 5120),
    "fc2": (5120, 20480),
}


def bf16_ulp(v):
    return 2.0 ** (math.floor(math.log2(v)) - 7) if v > 0 else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(
        os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--shapes", default="qkv,proj,fc1,fc2")
    ap.add_argument("--indices", default="",
                    help="further comma-separated library indices for (b)")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--check-rows", type=int, default=2048)
    args = ap.parse_args()
    sys.path.insert(0, args.root)

    import torch
    import vit_10b_fsdp_example_amd._C as C
    from vit_10b_fsdp_example_amd.tuning import lt_algo_table

    assert torch.cuda.is_available()
    print(f"[bench_tn_dgrad] package root {args.root}")
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    table = lt_algo_table()
    extra = [int(s) for s in args.indices.split(",") if s]
    have_new = hasattr(C, "dgrad_tn")
    tok = args.tokens
    win = args.window

    for name in [s for s in args.shapes.split(",") if s]:
        out, inn = SHAPES[name]
        fl = 2.0 * tok * out * inn
        torch.manual_seed(0)
        sets = []
        for _ in range(4):
            flat = torch.randn(out * inn + 8, device=dev, dtype=bf) * 0.02
            sets.append((torch.randn(tok, out, device=dev, dtype=bf),
                         flat[8:].view(out, inn)))
        print(f"--- {name}: dX [{tok}, {inn}] = dY [{tok}, {out}] W", flush=True)

        def line(tag, ms, extra=""):
            print(f"{name:5s} {tag:<34s} {ms:8.3f} ms {fl / ms / 1e9:7.0f} TF/s"
                  f" {extra}", flush=True)

        rows = min(args.check_rows, tok)
        dy0, w0 = sets[0]
        ref = dy0[:rows].double() @ w0.double()
        ulp = bf16_ulp(ref.abs().max().item())

        def err(got):
            return (got[:rows].double() - ref).abs().max().item()

        # (a) today's path
        idx_nn = table.get(("N", "N", inn, tok, out), -1)
        err_a = err(C.lt_gemm(dy0, w0, idx_nn))
        a_ms = timed(rotating(lambda dy, w: C.lt_gemm(dy, w, idx_nn), sets),
                     win)
        line(f"(a) library NN idx {idx_nn}", a_ms, f"max err {err_a:.4g}")

        # (b) TN GEMM alone on a prebuilt W^T
        tsets = [(dy, w.t().contiguous()) for dy, w in sets]
        idx_tn = table.get(("T", "N", inn, tok, out))
        best = None
        # a key without an entry (qkv) tries the other T,N entries, all of
        # which have run on MI355X; one that does not validate falls back
        # to the heuristic inside lt_gemm
        tabled = [idx_tn] if idx_tn is not None else sorted(
            {v for k, v in table.items() if k[:2] == ("T", "N")})
        for idx in [-1] + tabled + extra:
            e = err(C.lt_gemm(dy0, tsets[0][1].t(), idx))
            ms = timed(rotating(
                lambda dy, wT, i=idx: C.lt_gemm(dy, wT.t(), i), tsets), win)
            line(f"(b) library TN idx {idx}", ms, f"max err {e:.4g}")
            if best is None or ms < best[1]:
                best = (idx, ms)
        print(f"{name:5s} (b) best idx {best[0]} {best[1]:.3f} ms "
              f"key T,N,{inn},{tok},{out}", flush=True)
        assert torch.equal(C.transpose2d(w0), tsets[0][1])
        del tsets
        torch.cuda.empty_cache()

        by_w = 2 * out * inn * 2
        t_w = timed(rotating(lambda dy, w: C.transpose2d(w), sets), win)
        print(f"{name:5s} transpose2d(W [{out},{inn}]) {t_w:7.3f} ms "
              f"{by_w / t_w / 1e9:5.2f} TB/s", flush=True)

        if not have_new:
            print(f"{name:5s} (c) dgrad_tn: not in this build")
        else:
            got = C.dgrad_tn(dy0, w0, best[0])
            err_c = err(got)
            assert torch.equal(got, C.dgrad_tn(dy0, w0, best[0]))
            c_ms = timed(rotating(
                lambda dy, w, i=best[0]: C.dgrad_tn(dy, w, i), sets), win)
            line(f"(c) dgrad_tn idx {best[0]}", c_ms,
                 f"max err {err_c:.4g} vs (a) {err_a:.4g} + ulp {ulp:.4g}: "
                 f"{'ok' if err_c <= err_a + ulp else 'EXCEEDS'} | "
                 f"vs (a) {a_ms:.3f} ms")
            del got
        del sets, dy0, w0, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
