"""GPU: row_linear's backward over a saved bf16 X: dW from
linear_bwd_weight_bf16z_f32g (the bf16 X read as stored), dX from
linear_fwd_to_bf16 (the data-gradient GEMM storing bf16 rows), each behind its
path option and each falling back to the widened chain -- X.float() for dW,
the fp32 GEMM and .to(bfloat16) for dX -- with the same bits.

M = 123,003 at K = 512, C = 128 (emb2 at net_size 256) is just above that
shape's x6 floor of 122,071 rows, with M % 16 == 11: a ragged last K16 step in
the dW kernel and a ragged last row tile in the bf16 store."""
import functools

import pytest
import torch

import grl.ops
from grl import TypedGraph, _lib
from grl.ops import row_linear

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
M, K, C = 123_003, 512, 128
OPTIONS = ("dw_bf16z_f32g", "linear_out_bf16")


def _i32(t):
    return t.contiguous().view(torch.int32)


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _same(a, r):
    assert a.shape == r.shape and a.dtype == r.dtype
    return torch.equal(_bits16(a), _bits16(r)) if a.dtype == BF16 else torch.equal(_i32(a), _i32(r))


@functools.lru_cache(maxsize=None)
def _case():
    """X (bf16, with exact +0 and -0), W, b, the output gradient, and
    row_linear(X.float(), ...)'s (out, dX rounded once, dW, db): made once."""
    assert M % 16 == 11 and M >= 122_071 and 2 * M * K * C >= 1.6e10
    gen = torch.Generator(device=DEV).manual_seed(25)
    X = torch.randn(M, K, device=DEV, generator=gen).to(BF16)
    u = torch.rand(M, K, device=DEV, generator=gen)
    X = torch.where(u < 0.05, torch.zeros((), dtype=BF16, device=DEV), X)
    X = torch.where((u >= 0.05) & (u < 0.10), -torch.zeros((), dtype=BF16, device=DEV), X)
    del u
    W = torch.randn(C, K, device=DEV, generator=gen) / K ** 0.5
    b = torch.randn(C, device=DEV, generator=gen)
    g = torch.randn(M, C, device=DEV, generator=gen)
    x, w, bb = X.float().requires_grad_(True), W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = row_linear(x, w, bb, relu=True)
    out.backward(g)
    ref = (out.detach(), x.grad.to(BF16), w.grad, bb.grad)
    return X, W, b, g, ref


def _backward(X, W, b, g):
    x, w, bb = X.detach().clone().requires_grad_(True), W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = row_linear(x, w, bb, relu=True)
    out.backward(g)
    assert x.grad.dtype == BF16 and w.grad.dtype == torch.float32
    return out.detach(), x.grad, w.grad, bb.grad


class _Spy:
    """Whether each of the two wrappers the backward tries returned a result."""

    def __init__(self, monkeypatch):
        self.dw, self.dx = [], []
        dw, dx = grl.ops.linear_bwd_weight_bf16z_f32g, grl.ops.linear_fwd_to_bf16

        def dw_spy(*a, **kw):
            res = dw(*a, **kw)
            self.dw.append(res is not None)
            return res

        def dx_spy(*a, **kw):
            res = dx(*a, **kw)
            self.dx.append(res is not None)
            return res

        monkeypatch.setattr(grl.ops, "linear_bwd_weight_bf16z_f32g", dw_spy)
        monkeypatch.setattr(grl.ops, "linear_fwd_to_bf16", dx_spy)


@pytest.mark.parametrize("dw_on,dx_on", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_row_linear_gradients_keep_their_bits(dw_on, dx_on, grl_option, monkeypatch):
    """out, dX (bf16), dW and db of row_linear on the bf16 X are
    row_linear(X.float(), ...)'s bit for bit, dX rounded once, whichever of the
    two options is on; each wrapper returns a result exactly when its option
    is on."""
    grl_option("gemm_x6", 1)
    grl_option("linear_bf16x", 1)
    X, W, b, g, ref = _case()
    grl_option("dw_bf16z_f32g", dw_on)
    grl_option("linear_out_bf16", dx_on)
    spy = _Spy(monkeypatch)
    got = _backward(X, W, b, g)
    assert spy.dw == [bool(dw_on)] and spy.dx == [bool(dx_on)]
    for name, a, r in zip(("out", "dX", "dW", "db"), got, ref):
        assert _same(a, r), f"{name} (dw_bf16z_f32g {dw_on}, linear_out_bf16 {dx_on})"
    assert bool(got[1].float().abs().sum() > 0) and bool(got[2].abs().sum() > 0) and bool(got[3].abs().sum() > 0)


def _backward_peak(X, W, b, g):
    """The backward's peak allocation over what is allocated when it starts."""
    x, w, bb = X.detach().clone().requires_grad_(True), W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = row_linear(x, w, bb, relu=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    out.backward(g)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(DEV) - before


def test_backward_makes_no_fp32_copy_of_the_table(grl_option):
    """With both options on the backward's own buffers are the fp32 copy of g
    (the ReLU's selection) [M, C], the bf16 dX [M, K], dW, the dW workspace,
    W's planes for the data-gradient GEMM and db; neither an fp32 X nor an
    fp32 dX (M K 4 bytes each) fits on top.  With both off -- X.float() for dW,
    an fp32 dX before the cast -- the peak is at least M K 4 bytes above the
    peak with both on."""
    grl_option("gemm_x6", 1)
    grl_option("linear_bf16x", 1)
    X, W, b, g, _ = _case()
    lib = _lib.lib()
    own = (M * C * 4 + M * K * 2 + K * C * 4 + lib.grl_linear_bwd_weight_workspace_size(M, K, C)
           + lib.grl_linear_fwd_ex_workspace_size(M, C, K, M) + C * 4)
    grl_option("dw_bf16z_f32g", 1)
    grl_option("linear_out_bf16", 1)
    on = _backward_peak(X, W, b, g)
    assert on < own + M * K * 4, (f"the backward allocated {on} bytes; its own buffers are {own}, an fp32 copy of X "
                                  f"or of dX {M * K * 4}")
    grl_option("dw_bf16z_f32g", 0)
    grl_option("linear_out_bf16", 0)
    off = _backward_peak(X, W, b, g)
    assert off >= on + M * K * 4, (on, off, M * K * 4)


# ---- the model -------------------------------------------------------------------
def _train_step(N, option):
    """(logits, {name: grad}) of one training forward + backward of the model
    with bf16 activations, both options at `option`."""
    from gnn.models import GraphCNNDropEdge

    D = 16
    torch.manual_seed(0)
    model = GraphCNNDropEdge(D, 5, 2, net_size=256, use_attention=False, dropedge_seed=7).to(DEV)  # (fixed masks)
    graph = TypedGraph.synthetic(N, 4.0, 2, seed=1, device=DEV)
    V = torch.randn(1, N, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    R = torch.randn(1, N, 5, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    model.train_activation_dtype = BF16
    model.train()
    model.edge_dropout.reset_calls()
    model.dropout.reset_calls()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    with _lib.options(dw_bf16z_f32g=option, linear_out_bf16=option):
        logits = model([V, graph])
        grads = torch.autograd.grad((logits * R).sum(), [p for _, p in named], allow_unused=True)
    return logits.detach(), {n: g for (n, _), g in zip(named, grads)}


def test_model_training_step_does_not_depend_on_the_options(grl_option, monkeypatch):
    """GraphCNNDropEdge with train_activation_dtype = bfloat16 at 123,000
    nodes (emb2's K = 512, C = 128 is above its x6 floor): emb2's backward takes
    both new entries with the options 1 and the widened chain with them 0; the
    logits and every parameter gradient are equal bit for bit."""
    grl_option("gemm_x6", 1)
    grl_option("linear_bf16x", 1)
    N = 123_000
    spy = _Spy(monkeypatch)
    on, on_grads = _train_step(N, 1)
    assert True in spy.dw and True in spy.dx, "emb2's backward did not take the new entries"
    spy.dw.clear()
    spy.dx.clear()
    off, off_grads = _train_step(N, 0)
    assert True not in spy.dw and True not in spy.dx
    assert on.dtype == torch.float32 and on.shape == (1, N, 5) and bool(torch.isfinite(on).all())
    assert torch.equal(_i32(on), _i32(off))
    assert set(on_grads) == set(off_grads) and {"emb2.0.weight", "emb2.0.bias", "gcn1.h_weights"} <= set(on_grads)
    for name, gr in on_grads.items():
        if gr is None:
            assert off_grads[name] is None, name
            continue
        assert torch.equal(_i32(gr), _i32(off_grads[name])), name
    assert bool(on_grads["emb2.0.weight"].abs().sum() > 0)
