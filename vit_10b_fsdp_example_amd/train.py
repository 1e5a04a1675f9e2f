"""Training loop / evaluation / logging (reference run_vit_training.py:203-324).

The step structure mirrors the reference exactly — forward, backward,
full-norm clip (FSDP) or all-reduce+clip (DDP baseline), AdamW step, LR
schedule, zero_grad(set_to_none) — with the MI355X-native substitutions:

  * eager HIP execution instead of XLA tracing: there is no mark_step;
    the equivalent discipline is that nothing in the hot loop calls
    .item() — logging goes through the HIP-event-gated async closure
    (dist.add_step_closure) and host scalar reduces run on a gloo
    communicator off the hot path,
  * bf16 compute with fp32 master shards under FSDP (compute dtype is
    configurable; fp32 reproduces reference numerics),
  * our own FusedAdamW (multi-tensor HIP step over the fp32 shards).
"""

import os
import pprint
import time

import torch

from . import dist as xdist
from .data import build_datasets
from .models import build_fsdp_vit_model
from .ops import CrossEntropyLoss, FusedAdamW, gemm_dispatch_context
from .utils import SmoothedValue, get_warmup_cosine_scheduler, save_ckpt, load_ckpt

MODEL_SEED = 1234


def resolve_compute_dtype(cfg):
    dtype = getattr(cfg, "dtype", "auto")
    if cfg.run_without_fsdp:
        # the plain-DDP baseline replicates the reference's fp32 end-to-end
        # numerics (no master/compute split exists without FSDP)
        return torch.float32
    if dtype == "bf16":
        return torch.bfloat16
    if dtype == "fp32":
        return torch.float32
    return torch.bfloat16 if torch.cuda.is_available() else torch.float32


def _format_mem(info):
    gib = 1 << 30
    return (
        f"used {info['bytes_used'] / gib:.1f}/{info['bytes_limit'] / gib:.1f} GiB, "
        f"torch allocated {info['allocated'] / gib:.1f} GiB, "
        f"reserved {info['reserved'] / gib:.1f} GiB"
    )


def run_logging(epoch, step, smoothed_loss, smoothed_time, loss, lr, device):
    """Deferred logging closure (reference run_vit_training.py:203-213):
    runs on the async logger thread after the step's HIP event fires, so
    loss.item() never stalls the compute stream."""
    loss_value = loss.item()
    reduced_loss = xdist.mesh_reduce("loss_value", loss_value, sum)
    reduced_loss /= xdist.get_world_size()
    smoothed_loss.update(reduced_loss, batch_size=1)
    xdist.master_print(
        f"epoch {epoch} step {step + 1}, lr: {lr:.4f}, "
        f"loss: {smoothed_loss.avg:.4f}, "
        f"sec/iter: {smoothed_time.avg:.4f}, "
        f"device memory: {_format_mem(xdist.get_memory_info(device))}"
    )


def train(cfg):
    batch_size = cfg.batch_size
    num_epochs = cfg.num_epochs
    device = xdist.init_distributed()
    rank = xdist.get_local_rank()
    compute_dtype = resolve_compute_dtype(cfg)

    # identical weight init on every rank (the reference gets this from
    # xmp.spawn's fork semantics; we seed explicitly)
    torch.manual_seed(MODEL_SEED)

    train_dataset, train_loader, train_sampler, _, val_loader, _ = build_datasets(
        cfg, device, compute_dtype=compute_dtype
    )
    xdist.rendezvous("loaded dataset")
    xdist.master_print(f"\n=== dataset ===\n{pprint.pformat(train_dataset)}\n")

    model = build_fsdp_vit_model(cfg, device, compute_dtype=compute_dtype)
    loss_fn = CrossEntropyLoss()
    xdist.rendezvous("loaded model")
    xdist.master_print(f"\n=== model ===\n{pprint.pformat(model)}\n")

    parameters = list(model.parameters())
    xdist.master_print(
        f"per-GPU (sharded) parameter num: {sum(p.numel() for p in parameters)}"
    )

    optimizer = FusedAdamW(parameters, lr=cfg.lr, weight_decay=cfg.weight_decay)
    lr_scheduler = get_warmup_cosine_scheduler(
        optimizer,
        warmup_iteration=cfg.warmup_steps,
        max_iteration=len(train_dataset) // batch_size * num_epochs,
    )
    xdist.rendezvous("loaded optimizer")
    xdist.master_print(f"\n=== optimizer ===\n{pprint.pformat(optimizer)}\n")

    os.makedirs(cfg.ckpt_dir, exist_ok=True)
    if cfg.resume_epoch > 0:
        ckpt_path = os.path.join(
            cfg.ckpt_dir, f"epoch_{cfg.resume_epoch}_rank_{rank}.ckpt"
        )
        load_ckpt(ckpt_path, model, optimizer, lr_scheduler)

    smoothed_loss = SmoothedValue(window_size=5)
    smoothed_time = SmoothedValue(window_size=5)
    from .profiling import StepProfiler

    profiler = StepProfiler(cfg, enabled=getattr(cfg, "profile", False))
    xdist.rendezvous("training begins")
    xdist.master_print("training begins")
    max_steps = getattr(cfg, "max_steps_per_epoch", 0)
    for epoch in range(cfg.resume_epoch + 1, num_epochs + 1):
        xdist.master_print(f"starting epoch {epoch}")
        time_epoch_b = time_step_b = time.time()
        model.train()
        train_sampler.set_epoch(epoch)
        for step, (data, target) in enumerate(train_loader):
            if max_steps and step >= max_steps:
                break
            # 1-2. forward + backward under the GEMM dispatch router
            # (TunedGemmMode when a tuned hipBLASLt table is present or
            # the MLP dims are configured for a fused GELU pass, which a
            # ViT's are by default; else NativeWgradMode under
            # VITFSDP_NATIVE_WGRAD=2, else a no-op: ops/linear.py)
            with gemm_dispatch_context():
                output = model(data)
                loss = loss_fn(output, target)
                loss.backward()
            if not cfg.run_without_fsdp:
                # clip on the FULL (not per-shard) gradient norm — the
                # shards partition the full gradient, so one scalar
                # all-reduce of the local sq-norms is exact
                if cfg.clip_grad_norm > 0:
                    # defer_scale: FusedAdamW folds the clip coefficient
                    # into its gradient read (no separate scale pass)
                    model.clip_grad_norm_(cfg.clip_grad_norm,
                                          defer_scale=True)
            else:
                # plain-DDP baseline (reference run_vit_training.py:271-275)
                xdist.reduce_gradients(optimizer)
                if cfg.clip_grad_norm > 0:
                    torch.nn.utils.clip_grad_norm_(parameters, cfg.clip_grad_norm)

            # 3. update
            optimizer.step()
            lr_scheduler.step()
            optimizer.zero_grad(set_to_none=True)

            profiler.step()

            # 4. logging (deferred, event-gated)
            t_new = time.time()
            time_step_elapsed, time_step_b = t_new - time_step_b, t_new
            smoothed_time.update(time_step_elapsed, batch_size=1)
            is_first_iter = epoch == cfg.resume_epoch + 1 and step == 0
            if is_first_iter or (step + 1) % cfg.log_step_interval == 0:
                lr = optimizer.param_groups[0]["lr"]
                xdist.add_step_closure(
                    run_logging,
                    args=(epoch, step, smoothed_loss, smoothed_time, loss, lr, device),
                )

        profiler.stop()
        xdist.drain_step_closures()
        time_epoch_elapsed = time.time() - time_epoch_b
        xdist.master_print(f"epoch {epoch} done ({time_epoch_elapsed:.2f} sec)")

        if epoch % cfg.ckpt_epoch_interval == 0 or epoch == num_epochs:
            ckpt_path = os.path.join(cfg.ckpt_dir, f"epoch_{epoch}_rank_{rank}.ckpt")
            save_ckpt(ckpt_path, model, optimizer, lr_scheduler, master_only=False)
        if epoch % cfg.test_epoch_interval == 0 or epoch == num_epochs:
            accuracy, _, _ = eval_on_val(val_loader, model, device)
            xdist.master_print(f"accuracy on val: {accuracy:.4f}")
    return model


@torch.no_grad()
def eval_on_val(val_loader, model, device):
    """Top-1 accuracy on the val split (reference run_vit_training.py:306-318;
    like the reference, drop_last=True on the val sampler makes the number
    approximate — tail images are dropped)."""
    model.eval()
    local_correct = torch.zeros(1, dtype=torch.long, device=device)
    local_total = 0
    for data, target in val_loader:
        output = model(data)
        pred = output.argmax(dim=-1)
        local_correct.add_(pred.eq(target.view_as(pred)).sum())
        local_total += target.size(0)
    correct = xdist.mesh_reduce("local_correct", local_correct.item(), sum)
    total = xdist.mesh_reduce("local_total", local_total, sum)
    accuracy = correct / total
    model.train()
    return accuracy, correct, total


def main(cfg):
    from .tuning import enable_tunableop

    enable_tunableop()
    device = xdist.init_distributed()
    xdist.master_print(f"\n=== cfg ===\n{pprint.pformat(vars(cfg))}\n")
    xdist.master_print(f"device: {device}, world size: {xdist.get_world_size()}")
    train(cfg)
    xdist.master_print("training completed")
    if xdist.is_distributed():
        import torch.distributed as dist

        dist.destroy_process_group()
