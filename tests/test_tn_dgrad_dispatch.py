"""Routing of the input gradient as a TN GEMM on a transposed weight
(ops/linear.py TunedGemmMode, _C.dgrad_tn) on the CPU, through the
mode's ``handler`` / ``dgrad_handler`` seams with fake kernels in plain
torch: which mm is taken, under which tuned key, that a closed gate and
VITFSDP_TN_DGRAD=0 leave the parent's op sequence, and that checkpoint
early-stop survives."""

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

    def dgrad(self, dy, w, idx):
        assert linmod._op_layout(dy) == "N" and linmod._op_layout(w) == "N"
        self.log.append(("dgrad", tuple(dy.shape), tuple(w.shape), idx))
        return torch.mm(dy, w)  # one aten.mm, which the GEMM counter counts


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
    monkeypatch.delenv("VITFSDP_TN_DGRAD", raising=False)
    monkeypatch.setenv("VITFSDP_TN_WGRAD", "0")  # the dgrad route alone
    monkeypatch.setattr(linmod, "_TN_DGRAD_MIN_ELEMS", 0)
    monkeypatch.setitem(linmod._GELU_CFG, "hid", 0)  # no fused dgelu here


def _mode(fakes, **kw):
    return linmod.TunedGemmMode(table=kw.pop("table", {}), native_wgrad=False,
                                handler=fakes.gemm,
                                dgrad_handler=fakes.dgrad, **kw)


def _linear_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(TOK, DIN, generator=g, requires_grad=True)
    w = torch.randn(DOUT, DIN, generator=g, requires_grad=True)
    b = torch.randn(DOUT, generator=g, requires_grad=True)
    return x, w, b


def _reference_grads(x, w, b):
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, w, b)]
    F.linear(*leaves).pow(2).sum().backward()
    return [t.grad for t in leaves]


def test_gate_table_floor_and_override(monkeypatch):
    # what ships in the table is (out, in) pairs the entry accepts
    for out, inn in linmod._TN_DGRAD_SHAPES:
        assert out % 8 == 0 and inn % 8 == 0
    monkeypatch.setattr(linmod, "_TN_DGRAD_MIN_ELEMS", -1)
    monkeypatch.setattr(linmod, "_TN_DGRAD_SHAPES", frozenset({(24, 8)}))
    ok = linmod._tn_dgrad_shapes_ok
    assert linmod._TN_DGRAD_MIN_TOK == 4096
    assert ok(24, 8, 4096) and ok(24, 8, 32768)
    assert not ok(24, 8, 4095)  # below the token floor
    assert not ok(8, 24, 32768)  # (out, in), not (in, out)
    assert not ok(32, 8, 32768)  # not in the table
    monkeypatch.setattr(linmod, "_TN_DGRAD_MIN_ELEMS", 24 * 8)
    assert ok(24, 8, 1) and ok(32, 8, 1) and not ok(16, 8, 32768)
    assert not ok(60, 8, 32768) and not ok(24, 12, 32768)  # multiples of 8


def test_routed_dgrad_and_hit_counts(open_gate):
    fakes = _Fakes()
    x, w, b = _linear_params()
    with _mode(fakes) as m:
        F.linear(x, w, b).pow(2).sum().backward()
    # the weight gradient and the forward are not the route's: with an
    # empty table they are stock ops and never reach the GEMM seam
    assert fakes.log == [("dgrad", (TOK, DOUT), (DOUT, DIN), -1)]
    assert m.tn_dgrad_hits == 1
    assert m.hits == 0 and m.wgrad_hits == 0 and m.tn_hits == 0
    for got, ref in zip((x.grad, w.grad, b.grad), _reference_grads(x, w, b)):
        assert torch.allclose(got, ref, rtol=1e-5, atol=1e-5)


def test_tuned_index_under_the_forward_dual_key(open_gate):
    """The GEMM is lt_gemm(dy, wT.t()): key ("T","N", in, tok, out).  The
    N,N entry of the same mm belongs to today's path and must not leak."""
    fakes = _Fakes()
    x, w, b = _linear_params()
    table = {("T", "N", DIN, TOK, DOUT): 4242,
             ("N", "N", DIN, TOK, DOUT): 1111}
    with _mode(fakes, table=table) as m:
        F.linear(x, w, b).pow(2).sum().backward()
    assert ("dgrad", (TOK, DOUT), (DOUT, DIN), 4242) in fakes.log
    assert m.tn_dgrad_hits == 1 and m.hits == 0
    # with the route off the same mm takes the N,N entry
    fakes = _Fakes()
    x, w, b = _linear_params()
    with linmod.TunedGemmMode(table=table, native_wgrad=False,
                              handler=fakes.gemm) as m:
        F.linear(x, w, b).pow(2).sum().backward()
    assert m.tn_dgrad_hits == 0 and m.hits == 1
    assert fakes.log == [("gemm", "N", "N", (TOK, DOUT), (DOUT, DIN), 1111)]


def test_handler_without_dgrad_handler_keeps_the_route_off(monkeypatch):
    monkeypatch.delenv("VITFSDP_TN_DGRAD", raising=False)
    m = linmod.TunedGemmMode(table={}, native_wgrad=False,
                             handler=lambda a, b, idx, bias: a @ b)
    assert not m.tn_dgrad
    # nor do the weight-gradient seams or knobs open it
    monkeypatch.setenv("VITFSDP_TN_WGRAD", "1")
    m = linmod.TunedGemmMode(
        table={}, native_wgrad=False, handler=lambda a, b, idx, bias: a @ b,
        tn_handler=lambda t, c: (t.t().contiguous(), None))
    assert m.tn_wgrad and not m.tn_dgrad
    monkeypatch.setenv("VITFSDP_TN_DGRAD", "0")
    f = _Fakes()
    assert not _mode(f).tn_dgrad


def _trace(fakes, monkeypatch, env_off, with_seam=True):
    if env_off:
        monkeypatch.setenv("VITFSDP_TN_DGRAD", "0")
    else:
        monkeypatch.delenv("VITFSDP_TN_DGRAD", raising=False)
    x, w, b = _linear_params(seed=1)
    log = _OpLog()
    kw = {"dgrad_handler": fakes.dgrad} if with_seam else {}
    mode = linmod.TunedGemmMode(table={}, native_wgrad=False,
                                handler=fakes.gemm, **kw)
    with log, mode as m:
        F.linear(x, w, b).pow(2).sum().backward()
    return log.ops, m, (x.grad, w.grad, b.grad)


def test_switched_off_and_closed_gate_are_the_parent_route(monkeypatch):
    """The op list that reaches the backend with VITFSDP_TN_DGRAD=0, and
    with the default gate at a shape outside the table, is the one of a
    mode that has no dgrad route at all (handler without dgrad_handler)."""
    monkeypatch.setenv("VITFSDP_TN_WGRAD", "0")
    monkeypatch.setitem(linmod._GELU_CFG, "hid", 0)
    monkeypatch.setattr(linmod, "_TN_DGRAD_MIN_ELEMS", 0)
    f_par, f_off = _Fakes(), _Fakes()
    ops_par, m_par, g_par = _trace(f_par, monkeypatch, False, with_seam=False)
    ops_off, m_off, g_off = _trace(f_off, monkeypatch, True)
    assert not m_par.tn_dgrad and not m_off.tn_dgrad
    assert ops_off == ops_par and f_off.log == f_par.log == []
    monkeypatch.setattr(linmod, "_TN_DGRAD_MIN_ELEMS", -1)
    f_closed = _Fakes()
    ops_closed, m_closed, g_closed = _trace(f_closed, monkeypatch, False)
    assert m_closed.tn_dgrad and m_closed.tn_dgrad_hits == 0
    assert ops_closed == ops_par and f_closed.log == []
    for a, b, c in zip(g_par, g_off, g_closed):
        assert torch.equal(a, b) and torch.equal(a, c)
    # and with the gate open the same call is routed
    monkeypatch.setattr(linmod, "_TN_DGRAD_MIN_ELEMS", 0)
    f_open = _Fakes()
    _, m_open, g_open = _trace(f_open, monkeypatch, False)
    assert m_open.tn_dgrad_hits == 1 and len(f_open.log) == 1
    for a, b in zip(g_par, g_open):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5)


def test_wgrad_and_forward_mms_are_never_taken_for_a_dgrad(open_gate):
    fakes = _Fakes()
    dy, x = torch.randn(TOK, DOUT), torch.randn(TOK, DIN)
    w = torch.randn(DOUT, DIN)
    with _mode(fakes) as m:
        dw = torch.mm(dy.t(), x)  # transposed first operand
        y = torch.mm(x, w.t())  # transposed second operand
        part = torch.mm(dy[:, :16], w[:16])  # rows of dy with gaps
        assert m.tn_dgrad_hits == 0 and fakes.log == []
        dx = torch.mm(dy, w)
        assert m.tn_dgrad_hits == 1
    assert torch.equal(dw, dy.t() @ x) and torch.equal(y, x @ w.t())
    assert torch.equal(part, dy[:, :16] @ w[:16])
    assert torch.allclose(dx, dy @ w, rtol=1e-5, atol=1e-5)
    # square operands, where shapes alone cannot tell the two apart
    a, b = torch.randn(TOK, TOK), torch.randn(TOK, TOK)
    with _mode(_Fakes()) as m:
        torch.mm(a.t(), b)
        assert m.tn_dgrad_hits == 0
        torch.mm(a, b)
        assert m.tn_dgrad_hits == 1


def test_what_the_entry_refuses_falls_through(open_gate):
    """An odd-sized or misaligned weight goes down the stock path."""
    fakes = _Fakes()
    dy = torch.randn(TOK, DOUT)
    w60 = torch.randn(DOUT, 60)
    flat = torch.randn(DOUT * DIN + 8)
    w_off = flat[1:1 + DOUT * DIN].view(DOUT, DIN)  # 4 bytes past 16
    assert w_off.data_ptr() % 16 != 0
    with _mode(fakes) as m:
        r60 = torch.mm(dy, w60)
        roff = torch.mm(dy, w_off)
    assert m.tn_dgrad_hits == 0 and fakes.log == []
    assert torch.equal(r60, dy @ w60) and torch.equal(roff, dy @ w_off)


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
    only, then 2 dgrads + 2 wgrads.  A routed dgrad is one GEMM, so the
    count is the stock one."""
    fakes = _Fakes()
    n, m, grads = _checkpoint_backward_gemms(lambda: _mode(fakes))
    assert n == 5
    assert m.tn_dgrad_hits == 2

    class _Off:
        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    n_off, _, grads_off = _checkpoint_backward_gemms(_Off)
    assert n_off == 5
    for a, b in zip(grads, grads_off):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5)
