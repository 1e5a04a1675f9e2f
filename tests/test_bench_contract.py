"""bench.py driver contract: `python bench.py --gpus N --steps K
--warmup W` must print ONE JSON line from rank 0 with the agreed
fields/types.  The round-end BENCH/SCALE runs depend on this shape —
this test keeps refactors from breaking it."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def _free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]



def test_bench_json_contract():
    res = subprocess.run(
        [sys.executable, "bench.py", "--model", "vit-tiny",
         "--per_gpu_batch", "2", "--steps", "1", "--warmup", "0"],
        capture_output=True, text=True, cwd=REPO, timeout=600,
    )
    assert res.returncode == 0, res.stderr[-2000:]
    json_lines = [ln for ln in res.stdout.splitlines()
                  if ln.startswith("{") and ln.endswith("}")]
    assert len(json_lines) == 1, res.stdout[-2000:]
    out = json.loads(json_lines[0])

    assert isinstance(out["metric"], str) and "images/sec" in out["metric"]
    assert isinstance(out["value"], (int, float)) and out["value"] > 0
    assert out["unit"] == "images/sec"
    assert out["n_gpus"] == 1
    assert out["steps"] == 1
    assert out["warmup"] == 0
    assert isinstance(out["ms_per_step"], (int, float)) and out["ms_per_step"] > 0
    assert out["higher_is_better"] is True
    assert out["scaling"] == "weak"
    assert out["vs_baseline"] is None  # reference publishes no number
    assert out["dtype"] in ("bf16", "fp32")
    assert out["data"] == "synthetic"
    cfg = out["config"]
    for key in ("model", "global_batch", "seq_len", "parallelism"):
        assert key in cfg, key
    assert cfg["global_batch"] == 2
    # value must be consistent with ms_per_step at N=1
    implied = 1000.0 / out["ms_per_step"] * cfg["global_batch"]
    assert abs(implied - out["value"]) / out["value"] < 0.05


def test_bench_default_metric_names_baseline_config():
    """The metric string names the BASELINE.json headline shape with the
    ACTUAL global batch of the run (bs=1024 at the 8-GPU node point) —
    checked statically so we don't build a 10B model on CPU."""
    src = open(os.path.join(REPO, "bench.py")).read()
    assert 'f"images/sec (whole node) for ViT-10B bs={b * world} 224px"' in src
    assert '"vit10b"' in src


def test_bench_torchrun_ws2():
    """The driver's exact N>1 launch shape (torch.distributed.run,
    one rank per GPU) on CPU/gloo at ws=2: rendezvous, cross-rank MAX
    timing reduce, exactly one JSON line from rank 0."""
    port = _free_port()
    res = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(port),
         "bench.py", "--gpus", "2", "--model", "vit-tiny",
         "--per_gpu_batch", "2", "--steps", "1", "--warmup", "0"],
        capture_output=True, text=True, cwd=REPO, timeout=900,
    )
    assert res.returncode == 0, res.stderr[-3000:]
    json_lines = [ln for ln in res.stdout.splitlines()
                  if ln.startswith("{") and ln.endswith("}")]
    assert len(json_lines) == 1, res.stdout[-2000:]
    out = json.loads(json_lines[0])
    assert out["n_gpus"] == 2
    assert out["config"]["global_batch"] == 4
    assert out["config"]["parallelism"] == "fsdp2"


def test_auto_ckpt_blocks_formula():
    """The memory model behind bench.py's auto --grad_ckpt_blocks: pins
    the N=1 choice to the A/B-validated region, monotonic relaxation
    with world size (weak scaling), full checkpointing when state
    swamps the device, and rank-determinism by construction (only the
    TOTAL device memory enters, never per-rank free)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location(
        "benchmod", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    class A:
        grad_ckpt = True
        shard_on_cpu = False
        per_gpu_batch = 128

    total = 288e9  # MI355X HBM3E
    ten_b = (224, 14, 5120, 32, 4.0)

    def ckpt(world, args=None, model=ten_b):
        img, patch, embed, blocks, mlp = model
        return bench.auto_ckpt_blocks(
            args or A(), world, img, patch, embed, blocks, mlp, total=total)

    # N=1: the measured-good region (box measured ckpt=13 at 65+ img/s,
    # 16 at 63.5; anything in 12..18 is within the validated band)
    assert 12 <= ckpt(1) <= 18, ckpt(1)
    # weak scaling: monotonically fewer checkpointed blocks as N grows
    vals = [ckpt(n) if ckpt(n) >= 0 else 0 for n in (1, 2, 4, 8)]
    assert vals == sorted(vals, reverse=True), vals
    assert vals[3] == 0  # N=8: no checkpointing needed
    # 60B on-device at N=1 cannot fit: full checkpointing (-1)
    assert ckpt(1, model=(224, 14, 8192, 48, 4.0)) == -1
    # grad_ckpt off -> -1 regardless
    class Off(A):
        grad_ckpt = False
    assert ckpt(1, args=Off()) == -1


def test_bench_torchrun_ws4():
    """ws=4 on CPU/gloo: the driver's SCALE shape at a world size the
    other tests don't cover (rank slicing, MAX-timing reduce, global
    batch arithmetic, one JSON line)."""
    port = _free_port()
    res = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
         "--master-port", str(port),
         "bench.py", "--gpus", "4", "--model", "vit-tiny",
         "--per_gpu_batch", "2", "--steps", "1", "--warmup", "0"],
        capture_output=True, text=True, cwd=REPO, timeout=900,
    )
    assert res.returncode == 0, res.stderr[-3000:]
    json_lines = [ln for ln in res.stdout.splitlines()
                  if ln.startswith("{") and ln.endswith("}")]
    assert len(json_lines) == 1, res.stdout[-2000:]
    out = json.loads(json_lines[0])
    assert out["n_gpus"] == 4
    assert out["config"]["global_batch"] == 8
    assert out["config"]["parallelism"] == "fsdp4"


def _run_bench(*extra):
    res = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--model", "vit-tiny",
         "--per_gpu_batch", "2", "--steps", "2", "--warmup", "1", *extra],
        capture_output=True, text=True, cwd=REPO, timeout=600,
    )
    assert res.returncode == 0, res.stderr[-2000:]
    json_lines = [ln for ln in res.stdout.splitlines()
                  if ln.startswith("{") and ln.endswith("}")]
    assert len(json_lines) == 1, res.stdout[-2000:]
    return json.loads(json_lines[0])


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs DIR writes the last timed step's outputs as
    float32 .npy files; inputs and initial weights are seeded, so two
    runs (one plain, one with --full) agree — exactly on CPU, where the
    eager ops are deterministic.  --full keeps the result line's shape."""
    import numpy as np

    a, b = tmp_path / "a", tmp_path / "b"
    out_a = _run_bench("--dump-outputs", str(a))
    out_b = _run_bench("--dump-outputs", str(b), "--full")
    assert out_a["steps"] == out_b["steps"] == 2
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert out_a[key] == out_b[key], key
    assert out_b["ms_per_step"] > 0

    names = sorted(p.name for p in a.iterdir())
    assert names == ["grad_norm.npy", "logits.npy", "loss.npy",
                     "params_sample.npy"]
    total = 0
    for name in names:
        x, y = np.load(a / name), np.load(b / name)
        assert x.dtype == np.float32 and np.isfinite(x).all(), name
        assert x.shape == y.shape and np.array_equal(x, y), name
        total += x.nbytes
    assert total <= 64 * 2**20
    assert np.load(a / "logits.npy").shape == (2, 1000)
    # the dumped loss IS the last timed step's loss
    loss = float(np.load(a / "loss.npy")[0])
    assert abs(loss - out_a["config"]["final_loss"]) < 1e-6
