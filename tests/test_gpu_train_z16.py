"""GPU: a bf16 saved Z through the GraphConv layer and GraphCNNDropEdge
(grl.ops.graph_conv(..., z_dtype=torch.bfloat16), train_z_dtype; DESIGN.md
§4.21).

The multiply consumes the unrounded Z and neither the data gradient nor db
reads Z, so out, X.grad and b.grad are held BITWISE to z_dtype=None; W.grad is
held bitwise to today's dW on the fp32 Z rounded once to bf16, and within the
derived bound of one rounding to the fp32-Z W.grad."""
import functools

import numpy as np
import pytest
import torch

import grl.ops
from grl import DropEdge, TypedGraph, _lib
from grl.ops import (PREMASK_ROWS, feature_dropout, feature_dropout_apply, graph_conv, graph_conv_fwd_train,
                     linear_bwd_weight, relu_grad_bf16, relu_grad_bf16_scaled)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
# (N, L, F, C): above PREMASK_ROWS with 2 N 7F C = 1.8e10; below it
LAYERS = [(80_000, 6, 64, 256), (20_011, 6, 256, 256)]


def _i32(t):
    return t.contiguous().view(torch.int32)


def _b16(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(N, L, F, C, p):
    g = TypedGraph.synthetic(N, 12.0 if F == 64 else 16.0, L, seed=3, device=DEV)
    g = g.with_dropedge(DropEdge(p, 4, 2, True) if p else None)
    gen = torch.Generator(device=DEV).manual_seed(N + C)
    Xb = torch.randn(N, F, device=DEV, generator=gen).to(BF16)
    K = g.segments * F
    W = torch.randn(K, C, device=DEV, generator=gen) / K ** 0.5
    b = torch.randn(C, device=DEV, generator=gen)
    R = torch.randn(N, C, device=DEV, generator=gen).to(BF16)
    return g, Xb, W, b, R


def _layer(Xb, g, W0, b0, R, relu, z_dtype, recompute=False, fdrop=None):
    X, W, b = (t.clone().requires_grad_(True) for t in (Xb, W0, b0))
    out = graph_conv(X, g, W, b, relu=relu, out_dtype=BF16, recompute=recompute, z_dtype=z_dtype, fdrop=fdrop)
    out.backward(R)
    return out.detach(), X.grad, W.grad, b.grad


class _Spy:
    def __init__(self, monkeypatch):
        self.ran = []
        dw = grl.ops.linear_bwd_weight_bf16z

        def dw_spy(*a, **kw):
            res = dw(*a, **kw)
            self.ran.append(res is not None)
            return res

        monkeypatch.setattr(grl.ops, "linear_bwd_weight_bf16z", dw_spy)


FDROP = DropEdge(0.5, 9, (1 << 48) + 1)


def _want_dw(Xb, g, W, b, R, relu, fd=None):
    """(W.grad by hand, the fp32 Z, the unmasked-or-masked fp32 gradient): today's dW -- the mask pass from
    PREMASK_ROWS rows (scaled under a fused dropout), else the GEMM that masks on its loads -- with the saved Z
    replaced by the fp32 Z rounded once to bf16."""
    N, C = R.shape
    out_f, Z_f = graph_conv_fwd_train(Xb, g, W, b, relu, out=torch.empty(N, C, dtype=BF16, device=DEV))
    Zr = Z_f.to(BF16).float()
    if fd is not None:
        scale = float(fd.to_c().scale)
        feature_dropout_apply(out_f, fd, 0, out=out_f)  # the dropped output: what the fused node saves
        g16, g32, _ = relu_grad_bf16_scaled(R, out_f, scale, want_f32=True)
        want = (linear_bwd_weight(Zr, g16.float(), None, False) if N >= PREMASK_ROWS
                else linear_bwd_weight(Zr, g32, out_f.float(), False))[0]
        return want, Z_f, g32
    if relu and N >= PREMASK_ROWS:
        g16 = relu_grad_bf16(R, out_f)[0]
        return linear_bwd_weight(Zr, g16.float(), None, False)[0], Z_f, g16.float()
    want = linear_bwd_weight(Zr, R.float().contiguous(), out_f.float() if relu else None, False)[0]
    return want, Z_f, (R.float() * (out_f > 0)) if relu else R.float()


def _same(a, c, what):
    assert torch.equal(_b16(a[0]), _b16(c[0])), f"{what}: out"
    assert torch.equal(_b16(a[1]), _b16(c[1])), f"{what}: X.grad"
    assert torch.equal(_i32(a[2]), _i32(c[2])), f"{what}: W.grad"
    assert torch.equal(_i32(a[3]), _i32(c[3])), f"{what}: b.grad"


@pytest.mark.parametrize("N,L,F,C", LAYERS)
@pytest.mark.parametrize("p", [0.3, 0.0])
@pytest.mark.parametrize("form", ["relu", "plain", "relu_fdrop"])
def test_layer_bits(N, L, F, C, p, form, grl_option, monkeypatch):
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16z", 1)
    relu, fd = form != "plain", FDROP if form == "relu_fdrop" else None
    g, Xb, W, b, R = _case(N, L, F, C, p)
    ref = _layer(Xb, g, W, b, R, relu, None, fdrop=fd)
    spy = _Spy(monkeypatch)
    got = _layer(Xb, g, W, b, R, relu, BF16, fdrop=fd)
    # the one-plane kernel ran exactly from PREMASK_ROWS rows, or without a ReLU
    assert spy.ran == ([True] if (N >= PREMASK_ROWS or not relu) else [])
    assert torch.equal(_b16(got[0]), _b16(ref[0])), "out"
    assert torch.equal(_b16(got[1]), _b16(ref[1])), "X.grad"
    assert torch.equal(_i32(got[3]), _i32(ref[3])), "b.grad"
    # W.grad: today's dW with the saved Z replaced by the fp32 Z rounded once
    want, Z_f, geff = _want_dw(Xb, g, W, b, R, relu, fd)
    assert torch.equal(_i32(got[2]), _i32(want)), "W.grad"
    # the accuracy of what did change: one RNE to bf16 (unit roundoff 2^-9) of every Z element, plus the
    # project's bound of an fp32 sum relative to sum |terms| (1e-5, test_gpu_x6_planes.py); 16 x 16 sampled (k, c)
    rng = np.random.default_rng(N)
    ks = torch.from_numpy(rng.integers(0, Z_f.shape[1], 16)).to(DEV)
    cs = torch.from_numpy(rng.integers(0, C, 16)).to(DEV)
    bound = (2.0 ** -9 + 1e-5) * (Z_f[:, ks].double().abs().t() @ geff[:, cs].double().abs())
    err = (got[2][ks][:, cs].double() - ref[2][ks][:, cs].double()).abs()
    assert bool((err <= bound).all()), f"W.grad error {float((err / bound).max()):.3f} of the bound"
    assert not torch.equal(_i32(got[2]), _i32(ref[2]))  # dW does see the rounded Z
    del Z_f, geff
    # dw_bf16z 0: Z widened once, the same bits
    grl_option("dw_bf16z", 0)
    spy.ran.clear()
    off = _layer(Xb, g, W, b, R, relu, BF16, fdrop=fd)
    assert spy.ran == []
    _same(off, got, "dw_bf16z 0")
    grl_option("dw_bf16z", 1)
    # recompute=True: z_dtype has no effect
    _same(_layer(Xb, g, W, b, R, relu, BF16, recompute=True, fdrop=fd),
          _layer(Xb, g, W, b, R, relu, None, recompute=True, fdrop=fd), "recompute")
    assert spy.ran == []


@pytest.mark.parametrize("case", ["gemm_x6_0", "graphconv_bwd_bf16_0", "below_the_floor"])
def test_where_the_one_plane_dw_does_not_apply_the_layer_yields_the_widened_paths_bits(case, grl_option, monkeypatch):
    """(dw_bf16z = 0 is in test_layer_bits.)  The split-bf16 kernels off, the
    widened backward (no bf16 data-gradient plan: an fp32 g), and a layer below
    the flop floor: Z is widened once and today's backward runs on it."""
    N, L, F, C = (3_000, 6, 64, 64) if case == "below_the_floor" else LAYERS[0]
    if case != "below_the_floor":
        grl_option(case[:-2], 0)
    g, Xb, W, b, R = _case(N, L, F, C, 0.3)
    spy = _Spy(monkeypatch)
    for relu in (True, False):
        ref = _layer(Xb, g, W, b, R, relu, None)
        got = _layer(Xb, g, W, b, R, relu, BF16)
        assert torch.equal(_b16(got[0]), _b16(ref[0])) and torch.equal(_b16(got[1]), _b16(ref[1]))
        assert torch.equal(_i32(got[3]), _i32(ref[3]))
        if case == "graphconv_bwd_bf16_0":  # the widened path masks in relu_grad (fp32) from PREMASK_ROWS rows
            out_f, Z_f = graph_conv_fwd_train(Xb, g, W, b, relu, out=torch.empty(N, C, dtype=BF16, device=DEV))
            g32, mask, _ = grl.ops.relu_grad(R.float().contiguous(), out_f.float() if relu else None, False)
            want = linear_bwd_weight(Z_f.to(BF16).float(), g32, mask, False)[0]
        else:
            want = _want_dw(Xb, g, W, b, R, relu)[0]
        assert torch.equal(_i32(got[2]), _i32(want)), (case, relu)
    assert not any(spy.ran)


def test_saved_z_is_half_the_bytes():
    N, L, F, C = LAYERS[0]
    g, Xb, W, b, R = _case(N, L, F, C, 0.3)
    K = g.segments * F
    _layer(Xb, g, W, b, R, True, BF16)  # warm: whatever the graph caches on its first passes exists

    def held(z_dtype):
        X, Wp, bp = (t.clone().requires_grad_(True) for t in (Xb, W, b))
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        out = graph_conv(X, g, Wp, bp, relu=True, out_dtype=BF16, z_dtype=z_dtype)
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated() - before, out

    h32, o32 = held(None)
    del o32
    h16, o16 = held(BF16)
    assert h16 - h32 < -N * K * 2 + (1 << 20), (h16, h32)
    # the backward on the eligible path makes no widened Z (N K 4 = 143 MB here).  Its buffers: the masked bf16
    # gradient, the bf16 dX, dW, the dW GEMM's and the data gradient's workspaces (W's planes); 16 MB of slack
    # for the allocator's rounding -- so a widened copy trips the bound.
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    o16.backward(R)
    torch.cuda.synchronize()
    ws = _lib.lib().grl_linear_bwd_weight_workspace_size(N, K, C)
    planes = K * 512 * 3 * 2 + 4096
    listed = N * C * 2 + N * F * 2 + K * C * 4 + ws + planes + (16 << 20)
    peak = torch.cuda.max_memory_allocated() - base
    print(f"backward peak {peak} bytes, listed {listed}, N K 4 = {N * K * 4}")
    assert N * K * 4 > 4 * (16 << 20)  # a widened Z is far more than the slack: it would trip the bound
    assert peak < listed


def test_recompute_none_counts_two_bytes_an_element(monkeypatch):
    N, L, F, C = LAYERS[1]
    g, Xb, W, b, R = _case(N, L, F, C, 0.0)
    K = g.segments * F
    monkeypatch.setattr(grl.ops, "RECOMPUTE_Z_BYTES", N * K * 3)
    calls = []
    train, infer = grl.ops.graph_conv_fwd_train, grl.ops.graph_conv_infer
    monkeypatch.setattr(grl.ops, "graph_conv_fwd_train", lambda *a, **kw: (calls.append("train"), train(*a, **kw))[1])
    monkeypatch.setattr(grl.ops, "graph_conv_infer", lambda *a, **kw: (calls.append("infer"), infer(*a, **kw))[1])
    X = Xb.clone().requires_grad_(True)
    graph_conv(X, g, W, b, relu=True, out_dtype=BF16, z_dtype=BF16)
    assert calls == ["train"]  # Z is kept: N K 2 bytes
    calls.clear()
    graph_conv(X, g, W, b, relu=True, out_dtype=BF16)
    assert calls == ["infer"]  # an fp32 Z would take N K 4: recomputed, as today


def test_z_dtype_needs_a_bf16_out():
    g, Xb, W, b, R = _case(*LAYERS[1], 0.0)
    with pytest.raises(_lib.GrlError, match="out_dtype=bfloat16"):
        graph_conv(Xb, g, W, b, z_dtype=BF16)
    with pytest.raises(_lib.GrlError, match="z_dtype"):
        graph_conv(Xb, g, W, b, out_dtype=BF16, z_dtype=torch.float16)
    with torch.no_grad():  # no gradient wanted: ignored
        a = graph_conv(Xb, g, W, b, out_dtype=BF16, z_dtype=BF16)
        assert torch.equal(_b16(a), _b16(graph_conv(Xb, g, W, b, out_dtype=BF16)))


# ---- the model -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_case():
    from gnn.models import GraphCNNDropEdge

    N, D = 20_011, 64
    torch.manual_seed(0)
    model = GraphCNNDropEdge(D, 5, 6, net_size=256, dropedge_seed=7).to(DEV)
    graph = TypedGraph.synthetic(N, 16.0, 6, seed=1, device=DEV)
    V = torch.randn(1, N, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    R = torch.randn(1, N, 5, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    return model, graph, V, R


def _run(model, forward, R, train=True):
    model.train(train)
    model.edge_dropout.reset_calls()
    model.dropout.reset_calls()
    try:
        logits = forward()
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        grads = torch.autograd.grad((logits * R).sum(), [p for _, p in named], allow_unused=True)
        return logits.detach(), {n: g for (n, _), g in zip(named, grads)}
    finally:
        model.eval()


def _head_by_hand(model, x):
    from gnn.models.networks.robust_gcn import apply_linear

    v = apply_linear(model.emb2, x)
    v = model.self_atten(v)
    v = model.dropout(apply_linear(model.w_rand.projection, v, relu=True))
    return apply_linear(model.classifier, v)


def _z16_chain_by_hand(model, V, graph):
    """The training forward with bf16 activations and a bf16 saved Z from the
    public ops, every dropout unfused; g1's consumers in the model's order
    (gcn2, cat[g1, g2], cat[g1, g3])."""
    C = model.net_size
    drop, edges = model.dropout, model.edge_dropout

    def layer(gc, x):
        out = graph_conv(x, edges(graph, True), gc.h_weights, gc.bias, relu=True, out_dtype=BF16, z_dtype=BF16)
        return feature_dropout(out, drop.record(DEV), 0)

    x0 = feature_dropout(model._embed(V).reshape(-1, C).to(BF16), drop.record(DEV), 0)
    g1 = layer(model.gcn1, x0)
    g2 = layer(model.gcn2, g1)
    g3 = layer(model.gcn3, torch.cat([g1, g2], dim=-1))
    return _head_by_hand(model, torch.cat([g1, g3], dim=-1).float().view(1, -1, 2 * C))


def test_model_train_z_dtype(monkeypatch):
    from gnn.models.networks.robust_gcn import GraphConv

    model, graph, V, R = _model_case()
    seen = []
    propagate = GraphConv.propagate

    def spy(self, *a, **kw):
        seen.append(kw.get("z_dtype"))
        return propagate(self, *a, **kw)

    monkeypatch.setattr(GraphConv, "propagate", spy)
    try:
        model.train_activation_dtype = BF16
        base, base_g = _run(model, lambda: model([V, graph]), R)
        assert seen == [None] * 3
        seen.clear()
        model.train_z_dtype = BF16
        got, got_g = _run(model, lambda: model([V, graph]), R)
        assert seen == [BF16] * 3
        # logits and EVERY parameter gradient: bitwise the chain written out by hand with z_dtype=bfloat16
        want, want_g = _run(model, lambda: _z16_chain_by_hand(model, V, graph), R)
        assert torch.equal(got, want)
        assert set(got_g) == set(want_g) and len(got_g) >= 10
        for n, gr in got_g.items():
            assert gr is not None and torch.equal(gr, want_g[n]) and bool(gr.abs().sum() > 0), n
        assert torch.equal(got, base)  # logits: bitwise train_z_dtype = None
        for n in got_g:
            if n.endswith("h_weights"):  # the three that read Z: rounded once, so other bits
                assert not torch.equal(got_g[n], base_g[n]), n
            else:
                assert torch.equal(got_g[n], base_g[n]), n
        # train_z_dtype alone, and eval mode: today's bits
        model.train_activation_dtype = None
        seen.clear()
        alone, alone_g = _run(model, lambda: model([V, graph]), R)
        model.train_z_dtype = None
        fp32, fp32_g = _run(model, lambda: model([V, graph]), R)
        assert all(z is None for z in seen)
        assert torch.equal(alone, fp32) and all(torch.equal(alone_g[n], fp32_g[n]) for n in fp32_g)
        model.train_activation_dtype = model.train_z_dtype = BF16
        with torch.no_grad():
            model.eval()
            ev = model([V, graph])
            model.train_activation_dtype = model.train_z_dtype = None
            assert torch.equal(ev, model([V, graph]))
    finally:
        model.train_activation_dtype = model.train_z_dtype = None


def test_a_dense_a_gives_todays_bits():
    """A dense collate-layout A is outside the bf16 training path: both
    attributes are ignored, logits and gradients are today's."""
    from gnn.models import GraphCNNDropEdge

    B, N, L, D = 1, 1500, 6, 32  # a page: torch's dropout, reproduced by torch.manual_seed before each run
    torch.manual_seed(0)
    model = GraphCNNDropEdge(D, 5, L, net_size=64, dropedge_seed=7).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(4)
    A = (torch.rand(B, N, L, N, device=DEV, generator=gen) < 0.004).float()
    V = torch.randn(B, N, D, device=DEV, generator=gen)
    R = torch.randn(B, N, 5, device=DEV, generator=gen)
    try:
        torch.manual_seed(1)
        want, want_g = _run(model, lambda: model([V, A]), R)
        model.train_activation_dtype = model.train_z_dtype = BF16
        torch.manual_seed(1)
        got, got_g = _run(model, lambda: model([V, A]), R)
    finally:
        model.train_activation_dtype = model.train_z_dtype = None
    assert torch.equal(got, want) and bool(want.abs().sum() > 0)
    for n, gr in want_g.items():
        assert torch.equal(got_g[n], gr), n
