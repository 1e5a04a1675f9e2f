#!/usr/bin/env python3
"""Benchmark harness — measures the BASELINE.json headline metric:
images/sec (whole job) for ViT-10B FSDP training, bs=128 per GPU
(= global 1024 at 8 GPUs), 224px, synthetic data, bf16 compute with
fp32 master shards.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`;
for N>1 the driver launches via torch.distributed.run with one rank per
GPU over RCCL.  Rank 0 prints ONE JSON line.  Weak scaling: per-GPU
batch fixed at 128 as N grows.

A plain run does only what the headline figure needs: set up, warm up,
time K steps, print the result line.  `--dump-outputs DIR` additionally
writes what the last timed step computed as DIR/<name>.npy so that two
builds can be compared output for output (inputs, initial weights and
the sampled indices are all seeded, identical from run to run).
`--full` is the switch for secondary measurements; this harness has
none of its own (kernel-level benchmarks live under benchmarks/), so it
currently runs the same measurement as a plain run.
"""

import argparse
import contextlib
import json
import os
import time

import torch

MODELS = {
    # name: (image_size, patch, embed, heads, blocks, mlp_ratio, classes)
    "vit10b": (224, 14, 5120, 32, 32, 4.0, 1000),
    "vit-large": (224, 14, 1024, 16, 24, 4.0, 1000),
    "vit-tiny": (224, 14, 192, 3, 12, 4.0, 1000),
    "vit60b": (224, 14, 8192, 64, 48, 4.0, 1000),
}
PER_GPU_BATCH = 128


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--model", type=str, default="vit10b", choices=sorted(MODELS))
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--per_gpu_batch", type=int, default=PER_GPU_BATCH)
    p.add_argument("--shard_on_cpu", action="store_true")
    p.add_argument("--no_grad_ckpt", action="store_false", dest="grad_ckpt")
    # -2 = auto: checkpoint only as many blocks as the HBM headroom
    # requires (A/B: full ckpt 58.6 img/s vs first-16 63.5 at ViT-10B
    # N=1; identical gradients either way, recompute is pure overhead
    # wherever activations fit in the 288 GB)
    p.add_argument("--grad_ckpt_blocks", type=int, default=-2)
    p.add_argument("--fuse_residual", action="store_true")
    # where the synthetic initial weights are drawn.  "device" (default)
    # builds the model under the device context, so the ~10^10 uniform
    # draws of ViT-10B come from the GPU generator in well under a
    # second; "host" is the trainer's path (serial CPU generator, ~30 s
    # at ViT-10B, then a host-to-device copy per block).  Same
    # distributions and same seed either way, different random streams.
    p.add_argument("--init", type=str, default="device",
                   choices=["device", "host"])
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write the last step's "
                        "outputs as DIR/<name>.npy (float32)")
    p.add_argument("--full", action="store_true",
                   help="also run secondary measurements (none in this "
                        "harness today: same as a plain run)")
    return p.parse_args()


def dump_outputs(out_dir, last, model):
    """Write what the last timed step handed back (loss, logits, full
    gradient norm) plus a fixed seeded sample of the fp32 master weights
    it updated, as float32 .npy files (~1 MB in all at ViT-10B)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    arrays = {
        "loss": last["loss"].detach().reshape(1),
        "logits": last["logits"],
    }
    if last.get("grad_norm") is not None:
        arrays["grad_norm"] = last["grad_norm"].detach().reshape(1)
    gen = torch.Generator(device="cpu").manual_seed(2024)
    picks = []
    for prm in model.parameters():
        flat = prm.detach().reshape(-1)
        idx = torch.randint(0, flat.numel(), (4096,), generator=gen)
        picks.append(flat[idx.to(flat.device)].float().cpu())
    arrays["params_sample"] = torch.cat(picks)
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"),
                t.float().cpu().numpy().astype(np.float32))


def auto_ckpt_blocks(args, world, img, patch, embed, blocks, mlp_ratio,
                     total=None):
    """How many leading blocks to checkpoint so the rest's activations
    fit in device memory.  Sharded optimizer/master state shrinks with
    world size (weak scaling), so larger N checkpoints fewer blocks —
    at N=8 ViT-10B nothing needs checkpointing at all.

    Uses only the TOTAL device memory (identical on every rank), never
    the free amount: all ranks must derive the same checkpoint depth or
    their collective schedules diverge.  ``total`` is injectable for
    the CPU unit test."""
    if total is None:
        if not (torch.cuda.is_available() and args.grad_ckpt):
            return -1
        _free, total = torch.cuda.mem_get_info()
    elif not args.grad_ckpt:
        return -1
    from vit_10b_fsdp_example_amd.models.vit import count_vit_params
    params = count_vit_params(img, patch, embed, blocks, mlp_ratio, 1000)
    if args.shard_on_cpu:
        state = 0  # master/m/v live in host memory
    else:
        # fp32 master + exp_avg + exp_avg_sq + bf16 mirror + bf16 grads,
        # all sharded across ranks
        state = params * (4 + 4 + 4 + 2 + 2) / world
    # per-block saved activations when NOT checkpointed (bf16):
    # B*T*(8E + 2*hid) elements (ln outs, qkv, attn O, proj, sums, mlp)
    t = (img // patch) ** 2
    hid = int(embed * mlp_ratio)
    per_block = args.per_gpu_batch * t * (8 * embed + 2 * hid) * 2
    # transient: ~3 gathered units + grad payload + attention workspace
    transient = 3 * (params / blocks) * 2 * 2 + 8e9
    # 0.90 calibrated on the measured ViT-10B N=1 point: auto lands on
    # ckpt=16, the A/B-validated setting (63.5 img/s, no OOM)
    budget = 0.90 * total - state - transient
    n_nockpt = max(0, min(blocks, int(budget // per_block)))
    ckpt = blocks - n_nockpt
    return -1 if ckpt >= blocks else ckpt


def main():
    args = parse()
    from vit_10b_fsdp_example_amd import dist as xdist
    from vit_10b_fsdp_example_amd.cli import parse_args as cli_parse
    from vit_10b_fsdp_example_amd.models import build_fsdp_vit_model
    from vit_10b_fsdp_example_amd.ops import (
        CrossEntropyLoss, FusedAdamW, gemm_dispatch_context,
    )
    from vit_10b_fsdp_example_amd.utils import get_warmup_cosine_scheduler

    from vit_10b_fsdp_example_amd.tuning import enable_tunableop

    enable_tunableop()
    device = xdist.init_distributed()
    world = xdist.get_world_size()
    rank = xdist.get_rank()
    n_gpus = world if world > 1 else args.gpus
    assert n_gpus == world or world == 1, (
        f"--gpus {args.gpus} but WORLD_SIZE {world}; launch N>1 via torchrun"
    )

    img, patch, embed, heads, blocks, mlp_ratio, classes = MODELS[args.model]
    compute_dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    if not torch.cuda.is_available():
        compute_dtype = torch.float32

    if args.grad_ckpt_blocks == -2:
        args.grad_ckpt_blocks = auto_ckpt_blocks(
            args, world, img, patch, embed, blocks, mlp_ratio
        )
        xdist.master_print(
            f"[bench] auto grad_ckpt_blocks -> {args.grad_ckpt_blocks}"
        )

    cfg = cli_parse([
        "--fake_data",
        "--image_size", str(img), "--patch_size", str(patch),
        "--embed_dim", str(embed), "--num_heads", str(heads),
        "--num_blocks", str(blocks), "--mlp_ratio", str(mlp_ratio),
        "--num_classes", str(classes),
        "--batch_size", str(args.per_gpu_batch * world),
    ] + (["--shard_on_cpu"] if args.shard_on_cpu else [])
      + ([] if args.grad_ckpt else ["--no_grad_ckpt"])
      + (["--fuse_residual"] if args.fuse_residual else [])
      + (["--grad_ckpt_blocks", str(args.grad_ckpt_blocks)]
         if args.grad_ckpt_blocks >= 0 else []))

    torch.manual_seed(1234)
    t_build = time.time()
    on_device_init = (args.init == "device" and device.type == "cuda"
                      and not args.shard_on_cpu)
    with torch.device(device) if on_device_init else contextlib.nullcontext():
        model = build_fsdp_vit_model(cfg, device, compute_dtype=compute_dtype)
    loss_fn = CrossEntropyLoss()
    opt = FusedAdamW(model.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    sched = get_warmup_cosine_scheduler(opt, cfg.warmup_steps, 10**9)
    xdist.master_print(f"[bench] model built in {time.time() - t_build:.1f}s")

    b = args.per_gpu_batch
    # synthetic data: random normalized-image-like inputs (NOT zeros — a
    # zero-filled input inflates clocks/collapses softmax work), random
    # labels; two rotating buffers staged on device
    gen = torch.Generator(device="cpu").manual_seed(4242 + rank)
    batches = []
    for _ in range(2):
        x = torch.randn(b, 3, img, img, generator=gen).to(device, compute_dtype)
        y = torch.randint(0, classes, (b,), generator=gen).to(device)
        batches.append((x, y))

    last = {}  # what the most recent step computed (for --dump-outputs)

    def one_step(i):
        x, y = batches[i % 2]
        # dispatch-level GEMM rerouting (tuned hipBLASLt indices /
        # native wgrad) covers forward, recompute and backward
        with gemm_dispatch_context():
            logits = model(x)
            loss = loss_fn(logits, y)
            loss.backward()
        grad_norm = None
        if cfg.clip_grad_norm > 0:
            grad_norm = model.clip_grad_norm_(cfg.clip_grad_norm,
                                              defer_scale=True)
        opt.step()
        sched.step()
        opt.zero_grad(set_to_none=True)
        last.update(loss=loss, logits=logits.detach(), grad_norm=grad_norm)
        return loss

    def barrier_sync():
        if xdist.is_distributed():
            torch.distributed.barrier()
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    for i in range(args.warmup):
        one_step(i)
    barrier_sync()
    t0 = time.time()
    loss = None
    for i in range(args.steps):
        loss = one_step(i)
    barrier_sync()
    elapsed = time.time() - t0

    # MAX over ranks
    t = torch.tensor([elapsed], dtype=torch.float64)
    if xdist.is_distributed():
        t = t.to(device) if device.type == "cuda" else t
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
    elapsed = float(t.item())

    if args.dump_outputs and rank == 0 and last:
        dump_outputs(args.dump_outputs, last, model)

    images_per_sec = args.steps * b * world / elapsed
    ms_per_step = elapsed * 1000.0 / args.steps
    if rank == 0:
        result = {
            "metric": (
                # BASELINE.json metric on the ViT-10B config; the batch in
                # the string is the ACTUAL global batch of this run (the
                # bs=1024 node metric is its 8-GPU weak-scaling point)
                f"images/sec (whole node) for ViT-10B bs={b * world} 224px"
                " --fake_data"
                if args.model == "vit10b"
                else f"images/sec (whole node), {args.model} FSDP training"
            ),
            "value": round(images_per_sec, 2),
            "unit": "images/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 1),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no throughput
            "dtype": args.dtype if torch.cuda.is_available() else "fp32",
            "data": "synthetic",
            "config": {
                "model": {
                    "vit10b": "ViT-10B (5120d/32h/32L, patch14, 224px)",
                    "vit-large": "ViT-Large (1024d/16h/24L)",
                    "vit-tiny": "ViT-Tiny (192d/3h/12L)",
                    "vit60b": "ViT-60B-class (8192d/64h/48L)",
                }[args.model],
                "global_batch": b * world,
                "seq_len": (img // patch) ** 2,
                "parallelism": f"fsdp{world}" + ("+cpu_shard" if args.shard_on_cpu else ""),
                "grad_ckpt": cfg.grad_ckpt,
                "grad_ckpt_blocks": args.grad_ckpt_blocks,
                "fuse_residual": args.fuse_residual,
                "init": "device" if on_device_init else "host",
                "final_loss": float(loss.item()) if loss is not None else None,
            },
        }
        print(json.dumps(result), flush=True)

    if xdist.is_distributed():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
