#!/usr/bin/env python3
"""gelu_fwd_t (csrc/gelu.hip) against what it replaces, at the shape of the
ViT-10B MLP's hidden activation.

fc2's TN weight gradient reads act^T = gelu(h)^T.  It used to come from
transpose2d(act) on the saved act; with act no longer kept it comes from
gelu_fwd_t(h), which moves the same bytes and evaluates the GELU on the
way.  Three candidates, each as a series of --repeats windows of at least
--window seconds, rotating over four operand sets (5.4 GB, past the
256 MB L3) so that every call reads cold memory:

  transpose2d(act)              what the step paid before, act being saved
  gelu_fwd_t(h)                 what it pays now
  F.gelu(h) + transpose2d(.)    act rebuilt without the new kernel

Bytes are those the algorithm needs: one read and one write of the
tensor for the single-pass kernels, two of each for the two-pass
sequence.  The series are interleaved so that drift hits all three
alike.

    python benchmarks/bench_gelu_t.py [--rows 32768 --cols 20480]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_tail import timed  # noqa: E402
from bench_tn_wgrad import rotating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(
        os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--cols", type=int, default=20480)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, args.root)

    import torch
    import torch.nn.functional as F
    import vit_10b_fsdp_example_amd._C as C

    assert torch.cuda.is_available(), "bench_gelu_t needs a GPU"
    dev = torch.device("cuda", 0)
    R, Cc = args.rows, args.cols
    torch.manual_seed(0)
    sets = [(torch.randn(R, Cc, device=dev, dtype=torch.bfloat16),)
            for _ in range(4)]
    ref = F.gelu(sets[0][0]).t().contiguous()
    same = torch.equal(C.gelu_fwd_t(sets[0][0]), ref)
    del ref
    print(f"[bench_gelu_t] [{R}, {Cc}] bf16, gelu_fwd_t == "
          f"F.gelu(h).t().contiguous(): {same}", flush=True)
    assert same

    one_pass = 2 * R * Cc * 2  # bytes: read + write
    cands = [
        ("transpose2d", lambda h: C.transpose2d(h), one_pass),
        ("gelu_fwd_t", lambda h: C.gelu_fwd_t(h), one_pass),
        ("F.gelu + transpose2d", lambda h: C.transpose2d(F.gelu(h)),
         2 * one_pass),
    ]
    series = {name: [] for name, _, _ in cands}
    for _ in range(args.repeats):
        for name, fn, _ in cands:
            series[name].append(timed(rotating(fn, sets), args.window))
    for name, _, nbytes in cands:
        ms = series[name]
        mean = sum(ms) / len(ms)
        print(f"{name:<22s} " + " / ".join(f"{m:.3f}" for m in ms)
              + f" ms   mean {mean:.3f} ms  spread {max(ms) - min(ms):.3f} ms"
              f"  {nbytes / mean / 1e9:.2f} TB/s", flush=True)
    mean = {n: sum(v) / len(v) for n, v in series.items()}
    two = series["F.gelu + transpose2d"]
    print(f"gelu_fwd_t vs two passes: {mean['F.gelu + transpose2d'] - mean['gelu_fwd_t']:+.3f} ms "
          f"saved (two-pass spread {max(two) - min(two):.3f} ms)")
    print(f"gelu_fwd_t vs transpose2d alone: "
          f"{mean['gelu_fwd_t'] - mean['transpose2d']:+.3f} ms per call")


if __name__ == "__main__":
    main()
