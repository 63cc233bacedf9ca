"""Training with bf16 GraphConv activations: the GraphConv autograd node with
its feature dropout fused (grl.ops.graph_conv(..., fdrop=)) against the unfused
chain feature_dropout(graph_conv(...)) on bits, from PREMASK_ROWS rows and below
it, and GraphCNNDropEdge.train_activation_dtype against that chain written out
by hand from the public ops."""
import functools

import pytest
import torch

from grl import DropEdge, TypedGraph
from grl.ops import PREMASK_ROWS, feature_dropout, graph_conv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
FDROP = DropEdge(0.5, 11, (1 << 48) + 2)  # the feature dropout's record


def _bits(t):
    return t.view(torch.int16)


@functools.lru_cache(maxsize=None)
def _layer_case(N, L, F, C):
    g = TypedGraph.synthetic(N, 12.0 if C == 64 else 16.0, L, seed=3, device=DEV)
    g = g.with_dropedge(DropEdge(0.3, 4, 2, True))
    gen = torch.Generator(device=DEV).manual_seed(N + C)
    Xb = torch.randn(N, F, device=DEV, generator=gen).to(BF16)
    K = g.segments * F
    W = torch.randn(K, C, device=DEV, generator=gen) / K ** 0.5
    b = torch.randn(C, device=DEV, generator=gen)
    R = torch.randn(N, C, device=DEV, generator=gen).to(BF16)
    return g, Xb, W, b, R


def _layer(case, fused, grads=(True, True, True), row0=0):
    g, Xb, W0, b0, R = case
    X, W, b = (t.clone().requires_grad_(r) for t, r in zip((Xb, W0, b0), grads))
    if fused:
        out = graph_conv(X, g, W, b, relu=True, out_dtype=BF16, fdrop=FDROP, row0=row0)
    else:
        out = feature_dropout(graph_conv(X, g, W, b, relu=True, out_dtype=BF16), FDROP, row0)
    out.backward(R)
    return out.detach(), X.grad, W.grad, b.grad


SHAPES = [(80_000, 6, 256, 64), (20_011, 6, 256, 256)]  # from PREMASK_ROWS rows, and below it


@pytest.mark.parametrize("bwd_bf16", [1, 0])  # the bf16 data gradient, and the widened backward behind the scaled pass
@pytest.mark.parametrize("N,L,F,C", SHAPES)
def test_fused_node_is_the_unfused_chain_on_bits(N, L, F, C, bwd_bf16, grl_option):
    assert (N >= PREMASK_ROWS) == (C == 64)
    grl_option("graphconv_bwd_bf16", bwd_bf16)
    case = _layer_case(N, L, F, C)
    row0 = 5 if C == 64 else 0
    got = _layer(case, True, row0=row0)
    ref = _layer(case, False, row0=row0)
    assert got[0].dtype == BF16 and got[1].dtype == BF16 and got[1].shape == case[1].shape
    assert torch.equal(_bits(got[0]), _bits(ref[0])), "out"
    assert torch.equal(_bits(got[1]), _bits(ref[1])), "dX"
    assert torch.equal(got[2], ref[2]), "dW"
    assert torch.equal(got[3], ref[3]), "db"
    kept = float((got[0] > 0).float().mean())
    assert 0.1 < kept < 0.4  # about half of the open half
    assert bool(got[1].float().abs().sum() > 0) and bool(got[2].abs().sum() > 0)


def test_single_gradients_and_no_grad_are_the_chains_too():
    case = _layer_case(*SHAPES[1])
    ref = _layer(case, False)
    for i, grads in enumerate([(True, False, False), (False, True, False), (False, False, True)]):
        got = _layer(case, True, grads=grads)[1 + i]
        want = ref[1 + i]
        assert got.dtype == want.dtype and torch.equal(got.view(torch.int32), want.view(torch.int32)), grads
    g, Xb, W, b, _ = case
    with torch.no_grad():
        out = graph_conv(Xb, g, W, b, relu=True, out_dtype=BF16, fdrop=FDROP)
    assert out.dtype == BF16 and torch.equal(_bits(out), _bits(ref[0]))


def test_where_the_fused_form_does_not_apply_fdrop_is_a_separate_dropout():
    g, Xb, W, b, _ = _layer_case(*SHAPES[1])
    with torch.no_grad():
        Xf = Xb.float()
        for kw in ({"relu": True}, {"relu": False, "out_dtype": BF16}):
            X = Xb if "out_dtype" in kw else Xf
            got = graph_conv(X, g, W, b, fdrop=FDROP, row0=3, **kw)
            want = feature_dropout(graph_conv(X, g, W, b, **kw), FDROP, 3)
            assert got.dtype == want.dtype and torch.equal(got, want), kw
    X = Xf.clone().requires_grad_(True)
    graph_conv(X, g, W, b, relu=True, fdrop=FDROP).sum().backward()
    Y = Xf.clone().requires_grad_(True)
    feature_dropout(graph_conv(Y, g, W, b, relu=True), FDROP).sum().backward()
    assert torch.equal(X.grad, Y.grad)


def test_the_node_holds_one_bf16_output_between_the_passes():
    """What the fused node keeps alive after its forward is Z and ONE bf16
    [N, C] tensor (the dropped output, returned and saved); the unfused chain
    keeps the layer's output for the ReLU mask and the dropped one."""
    N, L, F, C = SHAPES[0]
    g, Xb, W0, b0, _ = _layer_case(N, L, F, C)
    with torch.no_grad():  # warm: whatever the graph caches on its first forward exists
        graph_conv(Xb, g, W0, b0, relu=True, out_dtype=BF16, fdrop=FDROP)
    held = {}
    for fused in (True, False):
        X, W, b = (t.clone().requires_grad_(True) for t in (Xb, W0, b0))
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        if fused:
            out = graph_conv(X, g, W, b, relu=True, out_dtype=BF16, fdrop=FDROP)
        else:
            out = feature_dropout(graph_conv(X, g, W, b, relu=True, out_dtype=BF16), FDROP)
        torch.cuda.synchronize()
        held[fused] = torch.cuda.memory_allocated() - before
        del out, X, W, b
    Z, one = N * g.segments * F * 4, N * C * 2
    slack = 1 << 20
    assert held[True] <= Z + one + slack, f"the fused node holds {held[True]} bytes; Z is {Z}, one bf16 output {one}"
    assert held[False] >= Z + 2 * one
    assert held[False] - held[True] >= one - slack


# ---------------------------------------------------------------- the model
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


def _params(model):
    return [(n, p) for n, p in model.named_parameters() if p.requires_grad]


def _run(model, forward, R, train=True):
    """(logits, {name: grad}) of one forward + backward on the scalar loss sum(logits * R)."""
    model.train(train)
    model.edge_dropout.reset_calls()
    model.dropout.reset_calls()
    try:
        logits = forward()
        named = _params(model)
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


def _bf16_chain_by_hand(model, V, graph):
    """The training forward with bf16 activations from the public ops, every
    dropout unfused; g1's consumers in the model's order (gcn2, cat[g1, g2],
    cat[g1, g3])."""
    C = model.net_size
    drop, edges = model.dropout, model.edge_dropout

    def layer(gc, x):
        out = graph_conv(x, edges(graph, True), gc.h_weights, gc.bias, relu=True, out_dtype=BF16)
        return feature_dropout(out, drop.record(DEV), 0)

    x0 = feature_dropout(model._embed(V).reshape(-1, C).to(BF16), drop.record(DEV), 0)
    g1 = layer(model.gcn1, x0)
    g2 = layer(model.gcn2, g1)
    g3 = layer(model.gcn3, torch.cat([g1, g2], dim=-1))
    return _head_by_hand(model, torch.cat([g1, g3], dim=-1).float().view(1, -1, 2 * C))


def _fp32_forward_by_hand(model, V, graph):
    """The fp32 training forward, as it stands without the attribute."""
    drop, edges = model.dropout, model.edge_dropout
    x0 = drop(model._embed(V))
    g1 = model.gcn1.propagate(x0, edges(graph, True), relu=True, dropout=drop)
    g2 = model.gcn2.propagate(g1, edges(graph, True), relu=True, dropout=drop)
    g3 = model.gcn3.propagate(torch.cat([g1, g2], dim=-1), edges(graph, True), relu=True, dropout=drop)
    return _head_by_hand(model, torch.cat([g1, g3], dim=-1))


def test_model_trains_with_bf16_activations_as_the_chain_by_hand(monkeypatch):
    from gnn.models.networks.robust_gcn import GraphConv

    model, graph, V, R = _model_case()
    assert model.train_activation_dtype is None
    seen = []  # (layer input dtype, output dtype), and the dtype of the gradient reaching each layer's output
    grads_seen = []
    propagate = GraphConv.propagate

    def spy(self, X, *a, **kw):
        out = propagate(self, X, *a, **kw)
        seen.append((X.dtype, out.dtype))
        if out.requires_grad:
            name = {id(model.gcn1): "gcn1", id(model.gcn2): "gcn2", id(model.gcn3): "gcn3"}[id(self)]
            out.register_hook(lambda g, name=name: grads_seen.append((name, g.dtype)))
        return out

    model.train_activation_dtype = BF16
    try:
        monkeypatch.setattr(GraphConv, "propagate", spy)
        got, got_grads = _run(model, lambda: model([V, graph]), R)
        monkeypatch.setattr(GraphConv, "propagate", propagate)
        # the inputs of gcn2 / gcn3 (and gcn1) are bfloat16, and so is the gradient reaching every layer's output
        assert seen == [(BF16, BF16)] * 3
        assert sorted(grads_seen) == [("gcn1", BF16), ("gcn2", BF16), ("gcn3", BF16)]
        want, want_grads = _run(model, lambda: _bf16_chain_by_hand(model, V, graph), R)
        # eval mode ignores the attribute
        with torch.no_grad():
            eval_bf16 = model([V, graph])
    finally:
        model.train_activation_dtype = None
    fp32, fp32_grads = _run(model, lambda: model([V, graph]), R)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got, want)
    assert not torch.equal(got, fp32)  # it is the bf16 path that ran
    assert set(got_grads) == set(want_grads) and len(got_grads) >= 10
    for name, g in got_grads.items():
        assert g is not None and g.dtype == torch.float32, name
        assert torch.equal(g, want_grads[name]), name
        assert bool(g.abs().sum() > 0), name
    # with the attribute None the training forward is the fp32 one, bit for bit
    by_hand, by_hand_grads = _run(model, lambda: _fp32_forward_by_hand(model, V, graph), R)
    assert torch.equal(fp32, by_hand)
    for name, g in fp32_grads.items():
        assert torch.equal(g, by_hand_grads[name]), name
    with torch.no_grad():
        assert torch.equal(eval_bf16, model([V, graph]))


def test_small_pages_keep_torchs_dropout_in_bf16_training():
    """A graph of at most ROW_LINEAR_MIN_ROWS rows keeps nn.Dropout, which
    takes bfloat16 as is: the bf16 training path still runs there."""
    from gnn.models import GraphCNNDropEdge

    torch.manual_seed(0)
    model = GraphCNNDropEdge(32, 5, 6, net_size=64).to(DEV).train()
    graph = TypedGraph.synthetic(300, 8.0, 6, seed=1, device=DEV)
    V = torch.randn(1, 300, 32, device=DEV)
    model.train_activation_dtype = BF16
    logits = model([V, graph])
    logits.sum().backward()
    assert logits.dtype == torch.float32 and bool(torch.isfinite(logits).all())
    assert model.gcn1.h_weights.grad is not None and bool(torch.isfinite(model.gcn1.h_weights.grad).all())
