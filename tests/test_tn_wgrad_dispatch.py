"""Routing of the weight gradient as a TN GEMM on transposed operands
(ops/linear.py TunedGemmMode, csrc/transpose.hip) on the CPU, through
the mode's ``handler`` / ``tn_handler`` seams with fake kernels in plain
torch: which ops are answered and in what sequence, that gradients are
unchanged, that the one-entry stash never answers the wrong sum or
outlives its step, and that checkpoint early-stop survives."""

import pytest
import torch
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils.checkpoint import checkpoint

from tests.utils_mp import CountMM
from vit_10b_fsdp_example_amd.ops import linear as linmod

TOK, DIN, DOUT = 16, 8, 24


class _Fakes:
    """Fake kernels that log what the route asks of them."""

    def __init__(self):
        self.log = []

    def gemm(self, a, b, idx, bias):
        self.log.append(("gemm", linmod._op_layout(a), linmod._op_layout(b),
                         tuple(a.shape), tuple(b.shape), idx))
        out = torch.mm(a, b)  # aten.mm, which the GEMM counter counts
        return out + bias if bias is not None else out

    def transpose(self, t, want_colsum):
        assert t.dim() == 2 and t.is_contiguous()
        self.log.append(("transpose", tuple(t.shape), want_colsum))
        return t.t().contiguous(), (t.sum(0) if want_colsum else None)


class _OpLog(TorchDispatchMode):
    """Outer mode: the aten ops that reach the backend."""

    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.ops.append(str(func))
        return func(*args, **(kwargs or {}))


@pytest.fixture()
def open_gate(monkeypatch):
    monkeypatch.delenv("VITFSDP_TN_WGRAD", raising=False)
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", 0)
    monkeypatch.setitem(linmod._GELU_CFG, "hid", 0)  # no fused dgelu here


def _mode(fakes, **kw):
    return linmod.TunedGemmMode(table=kw.pop("table", {}), native_wgrad=False,
                                handler=fakes.gemm,
                                tn_handler=fakes.transpose, **kw)


def _linear_params(seed=0, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(TOK, DIN, generator=g, requires_grad=True)
    w = torch.randn(DOUT, DIN, generator=g, requires_grad=True)
    b = torch.randn(DOUT, generator=g, requires_grad=True) if bias else None
    return x, w, b


def _reference_grads(x, w, b):
    leaves = [t.detach().clone().requires_grad_(True)
              for t in (x, w, b) if t is not None]
    F.linear(*leaves).pow(2).sum().backward()
    return [t.grad for t in leaves]


def test_routed_sequence_and_hit_counts(open_gate):
    fakes = _Fakes()
    x, w, b = _linear_params()
    with _mode(fakes) as m:
        F.linear(x, w, b).pow(2).sum().backward()
        assert m._tn_stash is None  # the bias sum consumed it
    # one pass over dy with its column sums, one over x, then the TN
    # GEMM: row-contiguous dy^T [out, K] times a transposed view of
    # x^T [in, K], heuristic index (empty table)
    assert fakes.log == [
        ("transpose", (TOK, DOUT), True),
        ("transpose", (TOK, DIN), False),
        ("gemm", "N", "T", (DOUT, TOK), (TOK, DIN), -1),
    ]
    assert m.tn_hits == 1 and m.tn_dbias_hits == 1
    assert m.hits == 0 and m.wgrad_hits == 0
    assert w.grad.shape == (DOUT, DIN) and w.grad.is_contiguous()
    for got, ref in zip((x.grad, w.grad, b.grad), _reference_grads(x, w, b)):
        assert torch.allclose(got, ref, rtol=1e-5, atol=1e-5)


def test_tuned_index_under_the_dual_key(open_gate):
    fakes = _Fakes()
    x, w, b = _linear_params()
    table = {("T", "N", DIN, DOUT, TOK): 4242}
    with _mode(fakes, table=table) as m:
        F.linear(x, w, b).pow(2).sum().backward()
    assert fakes.log[-1][-1] == 4242 and m.tn_hits == 1


def test_sum_of_another_tensor_is_not_answered(open_gate):
    fakes = _Fakes()
    dy = torch.randn(TOK, DOUT)
    x = torch.randn(TOK, DIN)
    other = torch.randn(TOK, DOUT)  # same shape, different storage
    with _mode(fakes) as m:
        dw = torch.mm(dy.t(), x)
        assert m.tn_hits == 1 and m._tn_stash is not None
        s_other = other.sum(0, keepdim=True)
        s_cols = dy.sum(1)  # same tensor, not the row reduction
        s_part = dy[:3].sum(0, keepdim=True)  # same pointer, fewer rows
        s_cast = dy.sum(0, keepdim=True, dtype=torch.float64)
        assert m.tn_dbias_hits == 0 and m._tn_stash is not None
        s_dy = dy.sum(0, keepdim=True)
        assert m.tn_dbias_hits == 1 and m._tn_stash is None
    assert len([e for e in fakes.log if e[0] == "transpose"]) == 2
    assert torch.allclose(dw, dy.t() @ x, rtol=1e-5, atol=1e-5)
    assert torch.equal(s_other, other.sum(0, keepdim=True))
    assert torch.equal(s_cols, dy.sum(1))
    assert torch.equal(s_part, dy[:3].sum(0, keepdim=True))
    assert torch.equal(s_cast, dy.sum(0, keepdim=True, dtype=torch.float64))
    assert s_dy.shape == (1, DOUT)
    assert torch.allclose(s_dy, dy.sum(0, keepdim=True))


def test_sum_before_gemm(open_gate):
    """The other arrival order: the sum does the pass over dy and parks
    dy^T, the GEMM takes it and transposes only x."""
    fakes = _Fakes()
    dy = torch.randn(TOK, DOUT)
    x = torch.randn(TOK, DIN)
    with _mode(fakes) as m:
        s = dy.sum(0)
        assert m.tn_dbias_hits == 1 and m._tn_stash is not None
        dw = torch.mm(dy.t(), x)
        assert m.tn_hits == 1 and m._tn_stash is None
    assert fakes.log == [
        ("transpose", (TOK, DOUT), True),
        ("transpose", (TOK, DIN), False),
        ("gemm", "N", "T", (DOUT, TOK), (TOK, DIN), -1),
    ]
    assert s.shape == (DOUT,) and torch.allclose(s, dy.sum(0))
    assert torch.allclose(dw, dy.t() @ x, rtol=1e-5, atol=1e-5)


def test_no_guessing_at_sums_once_a_gemm_came_first(open_gate):
    fakes = _Fakes()
    dy, x = torch.randn(TOK, DOUT), torch.randn(TOK, DIN)
    other = torch.randn(TOK, DOUT)
    with _mode(fakes) as m:
        torch.mm(dy.t(), x)
        dy.sum(0)
        n = len(fakes.log)
        s = other.sum(0)  # a row sum with no GEMM of ours: stock op
        assert len(fakes.log) == n and m.tn_dbias_hits == 1
    assert torch.equal(s, other.sum(0))


@pytest.mark.parametrize("dgelu_t", [True, False])
def test_fc1_takes_the_gelu_backwards_sums(monkeypatch, open_gate, dgelu_t):
    """With the fused GELU backward on, dy of fc1 already has its column
    sums parked, and dy^T too when that kernel writes it: the route
    transposes dy only when it has to, and parks nothing."""
    monkeypatch.setenv("VITFSDP_TN_DGELU_T", "1" if dgelu_t else "0")
    hid, d = 24, 8
    monkeypatch.setitem(linmod._GELU_CFG, "d", d)
    monkeypatch.setitem(linmod._GELU_CFG, "hid", hid)
    monkeypatch.delenv("VITFSDP_FUSED_DGELU_DBIAS", raising=False)
    fakes = _Fakes()

    def dgelu(dy, pre):
        dx = torch.ops.aten.gelu_backward(dy, pre, approximate="none")
        return dx, dx.reshape(-1, dx.shape[-1]).sum(0)

    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, d, generator=g, requires_grad=True)
    p = [torch.randn(*s, generator=g, requires_grad=True)
         for s in ((hid, d), (hid,), (d, hid), (d,))]

    def mlp(t, q):
        return F.linear(F.gelu(F.linear(t, q[0], q[1])), q[2], q[3])

    with _mode(fakes, dgelu_handler=dgelu) as m:
        mlp(x, p).pow(2).sum().backward()
        assert m._tn_stash is None and m._dgelu_stash is None
    assert m.tn_hits == 2
    assert m.tn_dbias_hits == 1 and m.dbias_hits == 1  # fc2's, fc1's
    wants = [e[2] for e in fakes.log if e[0] == "transpose"]
    # fc2: dy with sums, x; fc1: (dy,) x
    assert wants == ([True, False, False] if dgelu_t
                     else [True, False, False, False])
    got = [x.grad] + [t.grad for t in p]
    x2 = x.detach().clone().requires_grad_(True)
    p2 = [t.detach().clone().requires_grad_(True) for t in p]
    mlp(x2, p2).pow(2).sum().backward()
    for a, b in zip(got, [x2.grad] + [t.grad for t in p2]):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5)


def test_stash_cleared_on_exit(open_gate):
    fakes = _Fakes()
    m = _mode(fakes)
    with m:
        torch.mm(torch.randn(TOK, DOUT).t(), torch.randn(TOK, DIN))
        assert m._tn_stash is not None  # a linear without bias: no sum
    assert m._tn_stash is None
    with m:
        torch.randn(TOK, DOUT).sum(0)  # _tn_mm_first is per mode, set above
        assert m._tn_stash is None
    m2 = _mode(fakes)
    with m2:
        torch.randn(TOK, DOUT).sum(0)  # a parked dy^T whose GEMM never comes
        assert m2._tn_stash is not None
    assert m2._tn_stash is None


def _trace(fakes, env_off, monkeypatch):
    if env_off:
        monkeypatch.setenv("VITFSDP_TN_WGRAD", "0")
    else:
        monkeypatch.delenv("VITFSDP_TN_WGRAD", raising=False)
    x, w, b = _linear_params(seed=1)
    log = _OpLog()
    with log, _mode(fakes) as m:
        F.linear(x, w, b).pow(2).sum().backward()
    return log.ops, m, (x.grad, w.grad, b.grad)


def test_closed_gate_is_the_route_switched_off(monkeypatch):
    """Default gate (the measured ViT-10B shapes only): at a small shape
    the ops that reach the backend are those of VITFSDP_TN_WGRAD=0."""
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", -1)
    monkeypatch.setitem(linmod._GELU_CFG, "hid", 0)
    f_on, f_off = _Fakes(), _Fakes()
    ops_on, m_on, g_on = _trace(f_on, False, monkeypatch)
    ops_off, m_off, g_off = _trace(f_off, True, monkeypatch)
    assert m_on.tn_wgrad and not m_off.tn_wgrad
    assert ops_on == ops_off
    assert f_on.log == f_off.log == []
    assert m_on.tn_hits == m_on.tn_dbias_hits == 0
    for a, b in zip(g_on, g_off):
        assert torch.equal(a, b)
    # and with the gate open the same call is routed
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", 0)
    ops_open, m_open, _ = _trace(_Fakes(), False, monkeypatch)
    assert m_open.tn_hits == 1 and ops_open != ops_off


def test_gate_table_and_floors(monkeypatch):
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", -1)
    ok = linmod._tn_wgrad_shapes_ok
    assert ok(20480, 5120, 32768) and ok(5120, 20480, 32768)
    assert not ok(15360, 5120, 32768) and not ok(5120, 5120, 32768)
    assert not ok(20480, 5120, 1024)  # below the K floor
    assert linmod._tn_wgrad_out_ok(20480, 32768)
    assert not linmod._tn_wgrad_out_ok(15360, 32768)
    monkeypatch.setattr(linmod, "_TN_MIN_ELEMS", 256 * 256)
    assert ok(256, 256, 64) and not ok(256, 248, 64)
    assert not ok(260, 256, 64)  # not a multiple of 8 columns


def test_handler_without_tn_handler_keeps_the_route_off():
    m = linmod.TunedGemmMode(table={}, native_wgrad=False,
                             handler=lambda a, b, idx, bias: a @ b)
    assert not m.tn_wgrad


def _checkpoint_backward_gemms(mode_factory):
    torch.manual_seed(0)
    w1 = torch.randn(8, 8, requires_grad=True)
    b1 = torch.randn(8, requires_grad=True)
    w2 = torch.randn(8, 8, requires_grad=True)
    b2 = torch.randn(8, requires_grad=True)
    x = torch.randn(4, 8, requires_grad=True)

    def block(t):
        return F.linear(F.gelu(F.linear(t, w1, b1)), w2, b2)

    # the counter is the outer mode: it sees what the route emits
    counter = CountMM()
    with counter, mode_factory() as m:
        out = checkpoint(block, x, use_reentrant=False)
        n_fwd = counter.n
        out.pow(2).sum().backward()
    return counter.n - n_fwd, m, [t.grad for t in (x, w1, b1, w2, b2)]


def test_checkpoint_early_stop_preserved(open_gate):
    """As tests/test_checkpoint_earlystop.py: the recompute re-runs fc1
    only, then 2 dgrads + 2 wgrads.  The routed wgrads are one GEMM each,
    so the count is the stock one."""
    fakes = _Fakes()
    n, m, grads = _checkpoint_backward_gemms(lambda: _mode(fakes))
    assert n == 5
    assert m.tn_hits == 2 and m.tn_dbias_hits == 2 and m._tn_stash is None

    class _Off:
        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    n_off, _, grads_off = _checkpoint_backward_gemms(_Off)
    assert n_off == 5
    for a, b in zip(grads, grads_off):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5)
