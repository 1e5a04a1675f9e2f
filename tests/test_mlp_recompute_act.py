"""gelu(h) rebuilt in the backward instead of kept for it, on the CPU:
the saved-tensor hooks around fc2 (ops/linear.py mlp_fc2_recompute_act),
the TN weight-gradient route taking a pre-transposed activation, the rule
that opens the MLP half of checkpointed blocks (parallel/checkpoint.py)
and the model built with it.  fp32 throughout: the recompute is
deterministic, so every comparison is torch.equal."""

import pytest
import torch
import torch.nn.functional as F

from tests.utils_mp import CountMM
from vit_10b_fsdp_example_amd.cli import parse_args
from vit_10b_fsdp_example_amd.models import build_fsdp_vit_model
from vit_10b_fsdp_example_amd.models.vit import Block, Mlp
from vit_10b_fsdp_example_amd.ops import linear as linmod
from vit_10b_fsdp_example_amd.parallel import CommContext
from vit_10b_fsdp_example_amd.parallel.checkpoint import (
    CheckpointWrapper, checkpoint_module, n_open_mlp_blocks,
)

ROWS, DIM, HID = 12, 8, 32


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    monkeypatch.delenv("VITFSDP_MLP_RECOMPUTE_ACT", raising=False)
    monkeypatch.delenv("VITFSDP_FUSED_GELU", raising=False)


# ---- the hooks -------------------------------------------------------------


def _mlp_run(monkeypatch, switch, drop=0.0, wrap=None):
    """(grads of input, weights and biases, graph root) of one Mlp."""
    monkeypatch.setenv("VITFSDP_MLP_RECOMPUTE_ACT", switch)
    torch.manual_seed(0)
    mlp = Mlp(DIM, HID, drop=drop)
    x = torch.randn(3, ROWS // 3, DIM, requires_grad=True)
    run = (lambda t: mlp(t)[0]) if wrap is None else wrap(mlp)
    torch.manual_seed(1)  # the dropout masks, where there are any
    out = run(x)
    root = out.grad_fn
    out.pow(2).sum().backward()
    return [x.grad] + [p.grad for p in mlp.parameters()], root


def _rows_hid_storages_kept(switch, monkeypatch, drop=0.0, wrap=None):
    """Distinct [rows, hid]-sized storages an Mlp's graph keeps: counted
    through pack hooks of an outer pair, which see every tensor the
    forward saves that no inner pair has replaced."""
    monkeypatch.setenv("VITFSDP_MLP_RECOMPUTE_ACT", switch)
    torch.manual_seed(0)
    mlp = Mlp(DIM, HID, drop=drop)
    x = torch.randn(ROWS, DIM, requires_grad=True)
    kept = {}

    def pack(t):
        if t.numel() == ROWS * HID:
            kept[t.untyped_storage().data_ptr()] = t
        return t

    handles = []
    orig = linmod._ActHandle.__init__

    def spy(self, h, shape):
        orig(self, h, shape)
        handles.append(self)

    monkeypatch.setattr(linmod._ActHandle, "__init__", spy)
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        run = (lambda t: mlp(t)[0]) if wrap is None else wrap(mlp)
        torch.manual_seed(1)
        out = run(x)
    for h in handles:  # what a handle holds is kept too
        kept[h.h.untyped_storage().data_ptr()] = h.h
    return len(kept), len(handles), out


def test_hook_leaves_gradients_unchanged(monkeypatch):
    on, _ = _mlp_run(monkeypatch, "1")
    off, _ = _mlp_run(monkeypatch, "0")
    assert len(on) == len(off) == 5
    for a, b in zip(on, off):
        assert a is not None and torch.equal(a, b)


def test_hook_keeps_one_rows_by_hid_storage(monkeypatch):
    n_on, handles_on, _ = _rows_hid_storages_kept("1", monkeypatch)
    assert handles_on == 1
    assert n_on == 1  # h, held by GeluBackward and by the handle
    n_off, handles_off, _ = _rows_hid_storages_kept("0", monkeypatch)
    assert handles_off == 0
    assert n_off == 2  # h and gelu(h)


def test_no_hook_inside_a_whole_block_checkpoint(monkeypatch):
    """Nested hooks apply the innermost pair only: ours would hide fc2's
    input from the checkpoint and pin h, so a region runs without them."""
    def wrap(mlp):
        class _M(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.mlp = mlp

            def forward(self, t):
                return self.mlp(t)[0]

        return checkpoint_module(_M())

    _, handles, _ = _rows_hid_storages_kept("1", monkeypatch, wrap=wrap)
    assert handles == 0
    on, _ = _mlp_run(monkeypatch, "1", wrap=wrap)
    off, _ = _mlp_run(monkeypatch, "0")
    for a, b in zip(on, off):
        assert torch.equal(a, b)


def test_no_hook_behind_hidden_dropout(monkeypatch):
    _, handles, _ = _rows_hid_storages_kept("1", monkeypatch, drop=0.25)
    assert handles == 0
    assert not linmod.mlp_recompute_act_on(0.25)
    on, _ = _mlp_run(monkeypatch, "1", drop=0.25)
    off, _ = _mlp_run(monkeypatch, "0", drop=0.25)
    for a, b in zip(on, off):
        assert torch.equal(a, b)


def test_switches(monkeypatch):
    assert linmod.mlp_recompute_act_on(0.0)
    monkeypatch.setenv("VITFSDP_FUSED_GELU", "1")
    assert not linmod.mlp_recompute_act_on(0.0)
    monkeypatch.delenv("VITFSDP_FUSED_GELU")
    monkeypatch.setenv("VITFSDP_MLP_RECOMPUTE_ACT", "0")
    assert not linmod.mlp_recompute_act_on(0.0)


def test_unpack_off_the_gpu_route_is_plain_gelu():
    h = torch.randn(ROWS, HID)
    act = linmod._rebuild_act(h, (ROWS, HID), DIM)
    assert act.is_contiguous() and torch.equal(act, F.gelu(h))
    act3 = linmod._rebuild_act(h.view(3, 4, HID), (ROWS, HID), DIM)
    assert torch.equal(act3, F.gelu(h))


# ---- the route -------------------------------------------------------------


class _Fakes:
    def __init__(self):
        self.log = []

    def gemm(self, a, b, idx, bias):
        self.log.append(("gemm", linmod._op_layout(a), linmod._op_layout(b),
                         tuple(a.shape), tuple(b.shape)))
        return torch.mm(a, b)

    def transpose(self, t, want_colsum):
        assert t.dim() == 2 and t.is_contiguous()
        self.log.append(("transpose", tuple(t.shape), want_colsum))
        return t.t().contiguous(), (t.sum(0) if want_colsum else None)


def _routed_dw(monkeypatch, pre_transposed):
    monkeypatch.delenv("VITFSDP_TN_WGRAD", raising=False)
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", 0)
    monkeypatch.setitem(linmod._GELU_CFG, "hid", 0)
    g = torch.Generator().manual_seed(0)
    dy = torch.randn(16, 24, generator=g)
    x = torch.randn(16, 8, generator=g)
    if pre_transposed:
        x = x.t().contiguous().t()  # same values, x.t() contiguous
        assert not x.is_contiguous() and x.t().is_contiguous()
    fakes = _Fakes()
    with linmod.TunedGemmMode(table={}, native_wgrad=False,
                              handler=fakes.gemm,
                              tn_handler=fakes.transpose) as m:
        dw = torch.mm(dy.t(), x)
        assert m.tn_hits == 1
    return dw, fakes.log


def test_pre_transposed_x_is_not_transposed_again(monkeypatch):
    dw_c, log_c = _routed_dw(monkeypatch, False)
    dw_t, log_t = _routed_dw(monkeypatch, True)
    assert log_c == [("transpose", (16, 24), True),
                     ("transpose", (16, 8), False),
                     ("gemm", "N", "T", (24, 16), (16, 8))]
    assert log_t == [("transpose", (16, 24), True),
                     ("gemm", "N", "T", (24, 16), (16, 8))]
    assert torch.equal(dw_t, dw_c)


def test_wgemm_route_still_asks_for_a_contiguous_x():
    dy = torch.randn(64, 256)
    x = torch.randn(256, 64).t()
    assert linmod._wgrad_mm_dims(dy.t(), x) is None
    assert linmod._wgrad_mm_dims(dy.t(), x, b_t_ok=True) == (256, 256, 64)
    assert linmod._wgrad_mm_dims(dy.t(), x.contiguous()) == (256, 256, 64)
    # neither layout
    assert linmod._wgrad_mm_dims(dy.t(), torch.randn(64, 512)[:, ::2],
                                 b_t_ok=True) is None


# ---- the rule --------------------------------------------------------------


def test_n_open_rule():
    assert n_open_mlp_blocks(32, 13, 5120, 20480) == 12
    assert n_open_mlp_blocks(32, 32, 5120, 20480) == 0
    assert n_open_mlp_blocks(32, 0, 5120, 20480) == 0
    assert n_open_mlp_blocks(24, 20, 5120, 20480) == 2
    for n_blocks in (1, 4, 24, 32):
        for n_ckpt in range(n_blocks + 1):
            for e, hid in ((5120, 20480), (64, 64), (32, 256)):
                n = n_open_mlp_blocks(n_blocks, n_ckpt, e, hid)
                assert 0 <= n <= n_ckpt
                # saved elements per token row do not grow
                assert n * (2 * e + hid) <= (n_blocks - n_ckpt) * hid


# ---- the model -------------------------------------------------------------


def _model_step(extra):
    CommContext.reset()
    cfg = parse_args([
        "--fake_data", "--image_size", "16", "--patch_size", "4",
        "--embed_dim", "32", "--num_heads", "2", "--num_blocks", "4",
        "--num_classes", "5", "--batch_size", "2", "--num_workers", "0",
        *extra,
    ])
    torch.manual_seed(0)
    model = build_fsdp_vit_model(cfg, torch.device("cpu"))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 16, 16, generator=g)
    y = torch.randint(0, 5, (2,), generator=g)
    loss = F.cross_entropy(model(x), y)
    counter = CountMM()
    with counter:
        loss.backward()
    # an FSDP unit hands its gradient shard to the optimizer as
    # flat_param._comm_grad (fp32 here: one rank, fp32 compute)
    grads = [(p.grad if p.grad is not None else p._comm_grad).clone()
             for p in model.parameters()]
    opened = [m.open_mlp for m in model.modules()
              if isinstance(m, CheckpointWrapper)]
    names = sorted(model.state_dict()) + [n for n, _ in model.named_modules()]
    return loss.detach(), grads, counter.n, opened, names


@pytest.mark.parametrize("deferred", [False, True])
def test_model_gradients_and_recompute_gemms(monkeypatch, deferred):
    extra = ["--fuse_residual"] if deferred else []
    ckpt = extra + ["--grad_ckpt_blocks", "2"]
    monkeypatch.setenv("VITFSDP_MLP_RECOMPUTE_ACT", "1")
    l_on, g_on, n_on, open_on, names_on = _model_step(ckpt)
    l_none, g_none, n_none, open_none, _ = _model_step(
        extra + ["--no_grad_ckpt"])
    monkeypatch.setenv("VITFSDP_MLP_RECOMPUTE_ACT", "0")
    l_off, g_off, n_off, open_off, names_off = _model_step(ckpt)
    # floor(2 * 4E / 6E) = 1 of the 2 checkpointed blocks is opened
    assert open_on == [True, False] and open_off == [False, False]
    assert open_none == []
    assert names_on == names_off
    assert any("_checkpoint_wrapped_module.mlp.fc1" in n for n in names_on)
    assert torch.equal(l_on, l_off) and torch.equal(l_on, l_none)
    assert len(g_on) == len(g_off) == len(g_none)
    for a, b, c in zip(g_on, g_off, g_none):
        assert torch.equal(a, b) and torch.equal(a, c)
    # a block checkpointed whole re-runs qkv, proj and fc1 (fc2 is
    # early-stopped, tests/test_checkpoint_earlystop.py); an opened one
    # re-runs qkv and proj
    assert n_off == n_none + 3 + 3
    assert n_on == n_none + 2 + 3


def test_block_halves_compose_to_forward():
    torch.manual_seed(0)
    for deferred in (False, True):
        blk = Block(32, 2, deferred_residual=deferred)
        x = torch.randn(2, 5, 32)
        if deferred:
            x = (x, torch.randn(2, 5, 32))
        out = blk(x)
        halves = blk.mlp_half(*blk.attn_half(x))
        if deferred:
            assert all(torch.equal(a, b) for a, b in zip(out, halves))
        else:
            assert torch.equal(out, halves)
