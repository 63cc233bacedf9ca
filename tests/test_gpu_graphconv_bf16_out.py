"""GPU: the one-kernel GraphConv layer writing bf16 rows into a strided table
(grl_graphconv_fwd_bf16_to_bf16, grl_graphconv_fwd_train_bf16_to_bf16;
graphconv_ws_bf16o_kernel).

The MFMA waves round the finished fp32 tile to nearest even in registers and
store it with the caller's row stride, so every check here is on BITS: out
viewed as int16 equals the existing bf16-table entry's fp32 out cast by torch
(finite data: the same round-to-nearest-even), Z is torch.equal to that
entry's, and the columns beside a slice keep their sentinel.  The shapes sit
just above the x6 GEMM's 1.6e10-flop floor, as in test_gpu_graphconv_bf16.py:
below it no fusion runs, so every one-kernel case also checks the path by the
workspace query."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from grl import DropEdge, TypedGraph, _lib
from grl.ops import graph_conv, graph_conv_fwd_train, graph_conv_infer
from oracle import hash as ohash

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SENTINEL = 0x5A5A  # a finite bf16 bit pattern no result has by chance in every column


def _ws_query(X, g, W, C, out):
    csr = g.csr_c(X.shape[1])
    return _lib.lib().grl_graphconv_fwd_bf16_to_bf16_workspace_query(
        ctypes.byref(csr), X.data_ptr(), X.stride(0), X.shape[1], W.data_ptr(), C, out.data_ptr(), out.stride(0))


def _planes_only(ws, N, K, C):
    """W's planes (and the status word), far below Z: the one kernel."""
    return ws < 3 * (256 if C <= 256 else 512) * K * 2 + 4096 < N * K * 4


def _bits(t):
    return t.view(torch.int16)


def _bf16_randn(N, F, gen):
    return torch.randn(N, F, device=DEV, generator=gen).to(BF16)


def _sentinel_table(N, cols):
    return torch.full((N, cols), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)


CASES = [
    # N, L, F, C, has_self, deg
    (20_011, 6, 256, 256, True, 16.0),   # ragged last tile: both epilogue blocks
    (60_001, 3, 256, 200, False, 20.0),  # no self term, ragged C
    (24_001, 6, 256, 512, True, 12.0),   # 4 + 8 waves
    (10_007, 6, 1024, 512, True, 8.0),   # four virtual segments, 4 + 8 waves
    (70_001, 6, 64, 256, True, 12.0),    # NH = 1
]
VARIANTS = ["plain", "drop_bias_relu", "slice"]


@pytest.mark.parametrize("N,L,F,C,has_self,deg", CASES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_inference_bits_are_the_rounded_fp32_out(N, L, F, C, has_self, deg, variant, grl_option):
    de = DropEdge(0.3, 3, 2, True) if variant == "drop_bias_relu" else None
    bias = relu = variant == "drop_bias_relu"
    g = TypedGraph.synthetic(N, deg, L, seed=N % 7, device=DEV)
    if not has_self:
        g = TypedGraph(g.rowptr, g.colidx, L, has_self=False, num_cols=N)
    g = g.with_dropedge(de)
    gen = torch.Generator(device=DEV).manual_seed(N + F)
    Xb = _bf16_randn(N, F, gen)
    K = g.segments * F
    W = torch.randn(K, C, device=DEV, generator=gen) / K ** 0.5
    b = torch.randn(C, device=DEV, generator=gen) if bias else None
    want = _bits(graph_conv_infer(Xb, g, W, b, relu).to(BF16))

    def target():
        if variant != "slice":
            return None, torch.empty(N, C, dtype=BF16, device=DEV)
        table = _sentinel_table(N, C + 128)
        return table, table[:, 64:64 + C]

    table, out = target()
    assert _planes_only(_ws_query(Xb, g, W, C, out), N, K, C)  # one kernel, not SpMM + GEMM + rounding
    res = graph_conv_infer(Xb, g, W, b, relu, out=out)
    assert res is out and out.dtype == BF16
    assert torch.equal(_bits(out), want)
    if table is not None:
        assert out.stride(0) == C + 128 and not out.is_contiguous()
        assert bool((_bits(table[:, :64]) == SENTINEL).all()) and bool((_bits(table[:, 64 + C:]) == SENTINEL).all())
    with torch.no_grad():  # graph_conv routes here when no gradient is wanted
        got = graph_conv(Xb, g, W, b, relu, out_dtype=BF16)
    assert got.dtype == BF16 and got.is_contiguous() and torch.equal(_bits(got), want)
    grl_option("graphconv_fused", 0)
    table, out = target()
    assert _ws_query(Xb, g, W, C, out) >= N * K * 4 + N * C * 4
    graph_conv_infer(Xb, g, W, b, relu, out=out)
    assert torch.equal(_bits(out), want)
    if table is not None:
        assert bool((_bits(table[:, :64]) == SENTINEL).all()) and bool((_bits(table[:, 64 + C:]) == SENTINEL).all())


def test_edge_values():
    """fc_similarity-style edge values (vals != NULL) through the bf16-output kernel."""
    N, L, F, C = 20_480, 6, 256, 256
    rowptr, colidx = ohash.synth_csr(0, L, N, N * 12, 5)
    rng = np.random.default_rng(3)
    vals = rng.random(len(colidx)).astype(np.float32)
    g = TypedGraph.from_csr_host(rowptr, colidx, L, DEV, vals=vals).with_dropedge(DropEdge(0.3, 1, 4, True))
    K = 7 * F
    Xb = torch.from_numpy(rng.standard_normal((N, F)).astype(np.float32)).to(DEV).to(BF16)
    W = torch.from_numpy((rng.standard_normal((K, C)) / np.sqrt(K)).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).to(DEV)
    out = torch.empty(N, C, dtype=BF16, device=DEV)
    assert _planes_only(_ws_query(Xb, g, W, C, out), N, K, C)
    graph_conv_infer(Xb, g, W, b, True, out=out)
    assert torch.equal(_bits(out), _bits(graph_conv_infer(Xb, g, W, b, True).to(BF16)))


@functools.lru_cache(maxsize=None)
def _base():
    """The base shape's operands, shared (read-only) by the tests below."""
    N, L, F, C = 20_011, 6, 256, 256
    g = TypedGraph.synthetic(N, 16.0, L, seed=3, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    Xb = _bf16_randn(N, F, gen)
    W = torch.randn(7 * F, C, device=DEV, generator=gen) / 40
    b = torch.randn(C, device=DEV, generator=gen)
    R = torch.randn(N, C, device=DEV, generator=gen)
    return g, Xb, W, b, R


@pytest.mark.parametrize("F,C", [(256, 256), (512, 512)])
@pytest.mark.parametrize("de", [None, DropEdge(0.3, 4, 2, True)])
def test_training_forward_keeps_z_and_rounds_out(F, C, de, grl_option):
    N, L = 20_011, 6
    g = TypedGraph.synthetic(N, 10.0 if F > 256 else 16.0, L, seed=2, device=DEV).with_dropedge(de)
    gen = torch.Generator(device=DEV).manual_seed(F + C)
    Xb = _bf16_randn(N, F, gen)
    K = 7 * F
    W = torch.randn(K, C, device=DEV, generator=gen) / K ** 0.5
    b = torch.randn(C, device=DEV, generator=gen)
    out_f, Z_f = graph_conv_fwd_train(Xb, g, W, b, True)
    table = _sentinel_table(N, 2 * C)
    out = table[:, C:]
    assert _planes_only(_ws_query(Xb, g, W, C, out), N, K, C)
    res, Z = graph_conv_fwd_train(Xb, g, W, b, True, out=out)
    assert res is out and Z.dtype == torch.float32
    assert torch.equal(Z, Z_f)
    assert torch.equal(_bits(out), _bits(out_f.to(BF16)))
    assert bool((_bits(table[:, :C]) == SENTINEL).all())
    grl_option("graphconv_fused", 0)  # SpMM into Z, the linear into the workspace, the rounding pass
    out2 = torch.empty(N, C, dtype=BF16, device=DEV)
    _, Z2 = graph_conv_fwd_train(Xb, g, W, b, True, out=out2)
    assert torch.equal(Z2, Z_f) and torch.equal(_bits(out2), _bits(out))


def test_out_rows_off_the_dword_grid_take_two_kernels_and_give_the_same_bits():
    """out one element into a row: 2 B-aligned only, so no dword stores."""
    g, Xb, W, b, _ = _base()
    N, F = Xb.shape
    K, C = W.shape
    want = _bits(graph_conv_infer(Xb, g, W, b, True).to(BF16))
    table = _sentinel_table(N, C + 8)
    out = table[:, 1:1 + C]
    assert out.data_ptr() % 4 == 2
    assert _ws_query(Xb, g, W, C, out) >= N * K * 4 + N * C * 4
    graph_conv_infer(Xb, g, W, b, True, out=out)
    assert torch.equal(_bits(out), want)
    assert bool((_bits(table[:, :1]) == SENTINEL).all()) and bool((_bits(table[:, 1 + C:]) == SENTINEL).all())
    table = _sentinel_table(N, C + 3)  # an odd row stride
    out = table[:, :C]
    assert _ws_query(Xb, g, W, C, out) >= N * K * 4 + N * C * 4
    _, Z = graph_conv_fwd_train(Xb, g, W, b, True, out=out)
    assert torch.equal(_bits(out), want) and bool((_bits(table[:, C:]) == SENTINEL).all())
    assert torch.equal(Z, graph_conv_fwd_train(Xb, g, W, b, True)[1])
    with pytest.raises(_lib.GrlError, match="workspace"):
        graph_conv_infer(Xb, g, W, b, True, out=out, max_workspace_bytes=1 << 20)


def test_a_stack_in_one_table_is_the_chain_of_casts_and_cat():
    """gcn1 -> slice 0, gcn2 from slice 0 -> slice 1, gcn3 over the whole
    table: bitwise the existing bf16-table entries with explicit .bfloat16()
    and torch.cat between them."""
    g, Xb, W1, b1, _ = _base()
    g = g.with_dropedge(DropEdge(0.3, 4, 2, True))
    N, C = Xb.shape[0], W1.shape[1]
    gen = torch.Generator(device=DEV).manual_seed(11)
    W2 = torch.randn(7 * C, C, device=DEV, generator=gen) / 40
    W3 = torch.randn(7 * 2 * C, C, device=DEV, generator=gen) / 60
    r1 = graph_conv_infer(Xb, g, W1, b1, True).to(BF16)
    r2 = graph_conv_infer(r1, g, W2, None, True).to(BF16)
    r3 = graph_conv_infer(torch.cat([r1, r2], -1), g, W3, b1, True).to(BF16)
    table = _sentinel_table(N, 2 * C)
    s0, s1 = table[:, :C], table[:, C:]
    for X, W, out in ((Xb, W1, s0), (s0, W2, s1)):
        assert _planes_only(_ws_query(X, g, W, C, out), N, W.shape[0], C)
    graph_conv_infer(Xb, g, W1, b1, True, out=s0)
    graph_conv_infer(s0, g, W2, None, True, out=s1)  # reads one column range of the table, writes the other
    g3 = graph_conv_infer(table, g, W3, b1, True, out=torch.empty(N, C, dtype=BF16, device=DEV))
    assert torch.equal(_bits(s0), _bits(r1)) and torch.equal(_bits(s1), _bits(r2))
    assert torch.equal(_bits(g3), _bits(r3))


def _layer(X0, g, W0, b0, R, recompute, out_dtype=None):
    X, W, b = (t.clone().requires_grad_(True) for t in (X0, W0, b0))
    out = graph_conv(X, g, W, b, relu=True, recompute=recompute, out_dtype=out_dtype)
    out.backward(R.to(out.dtype))
    return out.detach(), X.grad, W.grad, b.grad


@pytest.mark.parametrize("recompute", [False, True])
def test_layer_gradients_are_the_bf16_layers_under_the_rounded_upstream(recompute):
    g, Xb, W, b, R = _base()
    g = g.with_dropedge(DropEdge(0.3, 4, 2, True))
    ref = _layer(Xb, g, W, b, R.to(BF16).float(), recompute)
    got = _layer(Xb, g, W, b, R, recompute, out_dtype=BF16)
    assert got[0].dtype == BF16 and got[0].is_contiguous() and got[1].dtype == BF16
    assert torch.equal(_bits(got[0]), _bits(ref[0].to(BF16))), "out"
    assert torch.equal(got[1], ref[1]), "dX"
    assert torch.equal(got[2], ref[2]), "dW"
    assert torch.equal(got[3], ref[3]), "db"


def test_no_fp32_copy_of_out_on_the_one_kernel_path():
    g, Xb, W, b, _ = _base()
    N, F = Xb.shape
    K, C = W.shape
    out = torch.empty(N, C, dtype=BF16, device=DEV)
    ws = _ws_query(Xb, g, W, C, out)
    assert _planes_only(ws, N, K, C)
    graph_conv_infer(Xb, g, W, b, True, out=out)  # warm: the graph's cached arrays exist
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    graph_conv_infer(Xb, g, W, b, True, out=out)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    assert extra < ws + N * C * 4, f"the call allocated {extra} bytes beyond out (an fp32 out is {N * C * 4})"


def test_dtype_errors():
    g, Xb, W, b, _ = _base()
    N, C = Xb.shape[0], W.shape[1]
    out = torch.empty(N, C, dtype=BF16, device=DEV)
    for fn in (graph_conv_infer, graph_conv_fwd_train):
        with pytest.raises(_lib.GrlError, match="bfloat16 out needs bfloat16 node features"):
            fn(Xb.float(), g, W, b, True, out=out)
        for bad in (torch.float16, torch.float64):
            with pytest.raises(_lib.GrlError, match="contiguous float32"):
                fn(Xb, g, W, b, True, out=out.to(bad))
        with pytest.raises(_lib.GrlError, match="unit column stride"):
            fn(Xb, g, W, b, True, out=torch.empty(C, N, dtype=BF16, device=DEV).t())
    with pytest.raises(_lib.GrlError, match="out_dtype=bfloat16 needs bfloat16 node features"):
        graph_conv(Xb.float(), g, W, b, True, out_dtype=BF16)
    with pytest.raises(_lib.GrlError, match="out_dtype must be"):
        graph_conv(Xb, g, W, b, True, out_dtype=torch.float16)


# ---------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def _model_case():
    from gnn.models import GraphCNNDropEdge

    N, D = 20_011, 64
    torch.manual_seed(0)
    model = GraphCNNDropEdge(D, 5, 6, net_size=256, dropedge_seed=7).to(DEV)
    graph = TypedGraph.synthetic(N, 16.0, 6, seed=1, device=DEV)
    V = torch.randn(1, N, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    return model, graph, V


def _logits(model, V, graph, act, train=False):
    model.activation_dtype = act
    model.train(train)
    model.edge_dropout.reset_calls()
    model.dropout.reset_calls()
    try:
        if train:
            return model([V, graph]).detach()
        with torch.no_grad():
            return model([V, graph])
    finally:
        model.activation_dtype = None
        model.eval()


def test_model_eval_with_bf16_activations_is_the_chain_by_hand():
    from gnn.models.networks.robust_gcn import apply_linear

    model, graph, V = _model_case()
    got = _logits(model, V, graph, BF16)
    with torch.no_grad():
        x0 = model._embed(V)[0].to(BF16)
        layer = lambda gc, x: graph_conv_infer(x, graph, gc.h_weights, gc.bias, True).to(BF16)  # noqa: E731
        g1 = layer(model.gcn1, x0)
        g2 = layer(model.gcn2, g1)
        g3 = layer(model.gcn3, torch.cat([g1, g2], -1))
        v = apply_linear(model.emb2, torch.cat([g1, g3], -1).float()[None])
        v = model.self_atten(v)
        v = apply_linear(model.w_rand.projection, v, relu=True)
        want = apply_linear(model.classifier, v)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got, want)
    assert not torch.equal(got, _logits(model, V, graph, None))  # it is the bf16 path that ran


def test_model_ignores_the_attribute_where_it_does_not_apply():
    model, graph, V = _model_case()
    assert model.activation_dtype is None  # the default
    assert torch.equal(_logits(model, V, graph, BF16, train=True), _logits(model, V, graph, None, train=True))
    model.activation_dtype = BF16
    model.eval()
    try:
        with_grad = model([V, graph]).detach()  # eval, but gradients enabled: the fp32 autograd path
    finally:
        model.activation_dtype = None
    assert torch.equal(with_grad, _logits(model, V, graph, None))
