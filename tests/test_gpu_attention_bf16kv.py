"""The attention forward over key / value tables stored as bf16
(grl_node_attention_fwd_bf16kv_rows) against the fp32 entry on
the widened tables: row_max / row_sum bitwise, out / o_norm equal as values (a
zero may differ in sign); against float64; query ranges; large scores; the
fallbacks; autograd through node_self_attention; NodeSelfAtten.kv_dtype."""
import functools

import pytest
import torch

import grl.ops
from grl import TypedGraph, _lib
from grl.ops import current_stream_handle, node_attention_forward, node_self_attention
from test_gpu_attention import _inputs, _ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16

# (B, N, dk, dv): the smallest shapes that reach each form of the kernel
SHAPES = [(1, 74, 16, 128),    # one partial block chain, S = 1, below the fp32 entry's plane threshold
          (4, 1100, 16, 128),  # key split S > 1, combine kernel
          (3, 4099, 16, 128),  # NW = 8 / B2, partial last block, unrolled loop and tails
          (2, 300, 32, 256),   # NT = 8, rolled loop
          (1, 600, 16, 64),    # NT = 2
          (2, 257, 32, 32)]    # NT = 1


@functools.lru_cache(maxsize=None)
def _case(B, N, dk, dv, scale=1.0, seed=None):
    """Inputs with K and H rounded to bf16, the fp32 entry's results on the
    widened tables (default options) and the float64 result: computed once."""
    Q, K, H, V, gamma = _inputs(B, N, dk, dv, seed=N + dk if seed is None else seed, scale=scale)
    K16, H16 = K.to(BF16), H.to(BF16)
    want = node_attention_forward(Q, K16.float(), H16.float(), V, gamma, stats=True)
    ref = _ref(*(t.double() for t in (Q, K16, H16, V, gamma)))
    return (Q, K16, H16, V, gamma), want, ref


def _bits(t):
    return t.view(torch.int32)


def _assert_same(got, want, what=""):
    out, onorm, rmax, rsum = got
    w_out, w_onorm, w_rmax, w_rsum = want
    assert torch.equal(_bits(rmax), _bits(w_rmax)), f"{what}: row_max bits"
    assert torch.equal(_bits(rsum), _bits(w_rsum)), f"{what}: row_sum bits"
    assert torch.equal(out, w_out), f"{what}: out"
    assert torch.equal(onorm, w_onorm), f"{what}: o_norm"


def _c_entry(Q, K16, H16, V, gamma, out, onorm=None, rmax=None, rsum=None, q0=0, q1=None, workspace=True):
    """grl_node_attention_fwd_bf16kv_rows called directly: its status."""
    B, N, dk = Q.shape
    dv = V.shape[2]
    lib = _lib.lib()
    n = lib.grl_node_attention_fwd_bf16kv_workspace_size(B, N, dk, dv) if workspace else 0
    ws = torch.empty(n, dtype=torch.uint8, device=DEV) if n else None
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = lib.grl_node_attention_fwd_bf16kv_rows(p(Q), p(K16), p(H16), p(V), p(gamma), p(out), p(onorm), p(rmax), p(rsum),
                                                B, N, dk, dv, q0, N if q1 is None else q1, p(ws), n,
                                                current_stream_handle(DEV))
    torch.cuda.synchronize()
    return rc


def _spy_entries(monkeypatch):
    """The names of the libgrl attention entries node_attention_forward calls."""
    seen = []
    real = grl.ops.call

    def call(name, *a):
        if name.startswith("grl_node_attention_fwd"):
            seen.append(name)
        return real(name, *a)

    monkeypatch.setattr(grl.ops, "call", call)
    return seen


@pytest.mark.parametrize("fwd8", [1, 0])
@pytest.mark.parametrize("B,N,dk,dv", SHAPES)
def test_forward_is_the_fp32_entrys_on_the_widened_tables(B, N, dk, dv, fwd8, monkeypatch, grl_option):
    (Q, K16, H16, V, gamma), want, ref = _case(B, N, dk, dv)
    grl_option("attn_fwd8", fwd8)
    seen = _spy_entries(monkeypatch)
    got = node_attention_forward(Q, K16, H16, V, gamma, stats=True)
    assert seen == ["grl_node_attention_fwd_bf16kv_rows"]
    _assert_same(got, want, f"fwd8={fwd8}")
    # ... and float64 on the widened tables (a mistake shared with the fp32 entry): test_gpu_attention.py's bounds
    tol = 1e-5 if N <= 2048 else 1e-4
    torch.testing.assert_close(got[0].double(), ref, rtol=tol, atol=tol)


def test_the_key_split_is_the_fp32_entrys():
    lib = _lib.lib()
    B, N, dk, dv = 4, 1100, 16, 128
    S = 4  # attn_splits(4, 1100) on the MI355X's 256 CUs (test_gpu_attention.py's SHAPES)
    # the (o, m, l) partials alone, S B N (dv + 2) floats rounded up to 256 B, plus the alignment slack: no planes
    want = (S * B * N * (dv + 2) * 4 + 255) // 256 * 256 + 512
    assert lib.grl_node_attention_fwd_bf16kv_workspace_size(B, N, dk, dv) == want
    assert lib.grl_node_attention_fwd_bf16kv_workspace_size(1, 74, dk, dv) == 0  # S = 1: nothing, no planes
    assert lib.grl_node_attention_fwd_bf16kv_workspace_size(1, 131072, dk, dv) == 0  # two full rounds: unsplit


def test_without_a_workspace_the_call_runs_unsplit():
    (Q, K16, H16, V, gamma), want, ref = _case(4, 1100, 16, 128)
    out = torch.empty_like(V)
    assert _c_entry(Q, K16, H16, V, gamma, out, workspace=False) == _lib.GRL_OK
    torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-5)


def test_query_ranges():
    (Q, K16, H16, V, gamma), want, _ = _case(4, 1100, 16, 128)
    B, N = Q.shape[:2]
    fill = -7.25
    outs = [torch.full_like(V, fill), torch.full_like(V, fill), torch.full_like(V[..., 0], fill),
            torch.full_like(V[..., 0], fill)]
    assert _c_entry(Q, K16, H16, V, gamma, *outs, q0=100, q1=1000) == _lib.GRL_OK
    for got, w in zip(outs, want):
        assert torch.equal(_bits(got[:, 100:1000]), _bits(w[:, 100:1000]))  # the whole call's rows
        assert (got[:, :100] == fill).all() and (got[:, 1000:] == fill).all()  # outside: untouched
    got = node_attention_forward(Q, K16, H16, V, gamma, stats=True, q_range=(100, 1000))
    for g, w in zip(got, want):
        assert torch.equal(_bits(g[:, 100:1000]), _bits(w[:, 100:1000]))


def test_large_scores(grl_option):
    """Scores of several hundred (test_large_scores_are_stable's inputs): the
    running max moves, so the alpha rescales happen."""
    (Q, K16, H16, V, gamma), want, ref = _case(2, 200, 16, 128, scale=6.0, seed=5)
    for fwd8 in (1, 0):
        grl_option("attn_fwd8", fwd8)
        got = node_attention_forward(Q, K16, H16, V, gamma, stats=True)
        assert torch.isfinite(got[0]).all()
        _assert_same(got, want, f"fwd8={fwd8}")
        torch.testing.assert_close(got[0].double(), ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("B,N,dk,dv,x6", [(2, 300, 9, 100, 1), (1, 500, 16, 96, 1), (2, 300, 16, 128, 0)])
def test_fallback_widens(B, N, dk, dv, x6, monkeypatch, grl_option):
    Q, K, H, V, gamma = _inputs(B, N, dk, dv, seed=N + dk)
    K16, H16 = K.to(BF16), H.to(BF16)
    grl_option("attn_x6", x6)
    want = node_attention_forward(Q, K16.float(), H16.float(), V, gamma, stats=True)
    seen = _spy_entries(monkeypatch)
    got = node_attention_forward(Q, K16, H16, V, gamma, stats=True)
    assert seen == ["grl_node_attention_fwd_rows"]
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    out = torch.full_like(V, 3.0)
    assert _c_entry(Q, K16, H16, V, gamma, out) == _lib.GRL_E_UNSUPPORTED
    assert (out == 3.0).all()


def test_unaligned_tables(monkeypatch):
    (Q, K16, H16, V, gamma), want, _ = _case(1, 600, 16, 64)
    for which in ("K", "H"):
        src = K16 if which == "K" else H16
        buf = torch.empty(src.numel() + 1, dtype=BF16, device=DEV)
        off = buf[1:].view(src.shape)  # one bf16 element past a 16 B boundary
        off.copy_(src)
        assert off.is_contiguous() and off.data_ptr() % 16 == 2
        k, h = (off, H16) if which == "K" else (K16, off)
        out = torch.full_like(V, 3.0)
        assert _c_entry(Q, k, h, V, gamma, out) == _lib.GRL_E_UNSUPPORTED
        assert (out == 3.0).all()
        seen = _spy_entries(monkeypatch)
        got = node_attention_forward(Q, k, h, V, gamma, stats=True)
        assert seen == ["grl_node_attention_fwd_rows"]
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        monkeypatch.undo()


def test_values_wider_than_one_call(monkeypatch):
    B, N, dk, dv = 1, 400, 32, 512  # two _dv_blocks of 256 columns
    Q, K, H, V, gamma = _inputs(B, N, dk, dv, seed=N + dk)
    K16, H16 = K.to(BF16), H.to(BF16)
    want = node_attention_forward(Q, K16.float(), H16.float(), V, gamma, stats=True)
    seen = _spy_entries(monkeypatch)
    got = node_attention_forward(Q, K16, H16, V, gamma, stats=True)
    assert seen == ["grl_node_attention_fwd_bf16kv_rows"] * 2
    _assert_same(got, want)


def test_dtypes():
    (Q, K16, H16, V, gamma), want, _ = _case(1, 600, 16, 64)
    with pytest.raises(_lib.GrlError, match="both"):
        node_attention_forward(Q, K16, H16.float(), V, gamma)
    with pytest.raises(_lib.GrlError, match="both"):
        node_attention_forward(Q, K16.float(), H16, V, gamma)
    with pytest.raises(_lib.GrlError, match="float32"):
        node_attention_forward(Q, K16.half(), H16.half(), V, gamma)
    with pytest.raises(_lib.GrlError, match="float32"):
        node_attention_forward(Q, K16, H16, V.to(BF16), gamma)
    # a bf16 Q is widened
    Q16 = Q.to(BF16)
    got = node_attention_forward(Q16, K16, H16, V, gamma)
    assert torch.equal(got, node_attention_forward(Q16.float(), K16.float(), H16.float(), V, gamma))


@pytest.mark.parametrize("B,N,dk,dv", [(1, 2048, 16, 128), (2, 700, 32, 64)])
def test_autograd(B, N, dk, dv):
    Q, K, H, V, gamma = _inputs(B, N, dk, dv, seed=7 * N + dv)
    K16, H16 = K.to(BF16), H.to(BF16)
    dout = torch.randn(V.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    a = [t.clone().requires_grad_(True) for t in (Q, K16, H16, V, gamma)]
    out = node_self_attention(*a)
    saved = out.grad_fn.saved_tensors
    out.backward(dout)
    w = [t.clone().requires_grad_(True) for t in (Q, K16.float(), H16.float(), V, gamma)]
    want = node_self_attention(*w)
    want.backward(dout)
    assert torch.equal(out, want)
    for i, name in ((0, "Q"), (3, "V"), (4, "gamma")):
        assert a[i].grad.dtype == torch.float32 and torch.equal(a[i].grad, w[i].grad), f"d{name}"
    for i, name in ((1, "K"), (2, "H")):
        assert a[i].grad.dtype == BF16 and torch.equal(a[i].grad, w[i].grad.to(BF16)), f"d{name}"
    # the node keeps K16 and H16, no widened copy: of the saved tensors shaped like K, one is bf16 (K16) and one
    # fp32 (Q); of those shaped like H, one is bf16 (H16) and one fp32 (o_norm)
    for shape, b16 in ((K16.shape, a[1]), (H16.shape, a[2])):
        like = [t for t in saved if t.shape == shape]
        assert sorted(str(t.dtype) for t in like) == ["torch.bfloat16", "torch.float32"]
        assert [t.data_ptr() for t in like if t.dtype == BF16] == [b16.data_ptr()]


def test_deterministic():
    (Q, K16, H16, V, gamma), _, _ = _case(3, 4099, 16, 128)
    a = node_attention_forward(Q, K16, H16, V, gamma, stats=True)
    b = node_attention_forward(Q, K16, H16, V, gamma, stats=True)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


# ---- the model -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_case(N):
    from gnn.models import GraphCNNDropEdge

    D = 64
    torch.manual_seed(0)
    model = GraphCNNDropEdge(D, 5, 6, net_size=256, dropedge_seed=7).to(DEV).eval()
    graph = TypedGraph.synthetic(N, 16.0 if N > 1000 else 4.0, 6, seed=1, device=DEV)
    V = torch.randn(1, N, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    return model, graph, V


def _attention_by_hand(self, V, shard=None):
    """NodeSelfAtten.forward on the libgrl path with bf16 key / value tables,
    from the public ops."""
    from gnn.models.networks.robust_gcn import linear_rows

    lins = (self.f[0], self.g[0], self.h[0])
    fgh = linear_rows(V, torch.cat([m.weight for m in lins]), torch.cat([m.bias for m in lins]), True, 0)
    dk = self.f[0].out_features
    f, g, h = fgh[..., :dk], fgh[..., dk:2 * dk], fgh[..., 2 * dk:]
    return node_self_attention(f, g.to(BF16), h.to(BF16), V, self.gamma)


def test_model_kv_dtype(monkeypatch):
    from gnn.models.networks.robust_gcn import ROW_LINEAR_MIN_ROWS, NodeSelfAtten

    N = 5000
    assert N > ROW_LINEAR_MIN_ROWS
    model, graph, V = _model_case(N)
    assert model.self_atten.kv_dtype is None
    try:
        with torch.no_grad():
            base = model([V, graph])
            model.self_atten.kv_dtype = BF16
            seen = _spy_entries(monkeypatch)
            got = model([V, graph])
            assert seen == ["grl_node_attention_fwd_bf16kv_rows"]
            monkeypatch.undo()
            model.self_atten.kv_dtype = None
            assert torch.equal(_bits(model([V, graph])), _bits(base))  # None: the untouched model, bit for bit
            monkeypatch.setattr(NodeSelfAtten, "forward", _attention_by_hand)
            want = model([V, graph])
            monkeypatch.undo()
        assert torch.equal(got, want)
        assert not torch.equal(got, base)  # the rounding of g and h is visible
        # one training step: every parameter has a finite gradient, and logits and gradients are those of the
        # by-hand forward under the same DropEdge / dropout masks (a fixed seed, calls numbered from 0)
        model.self_atten.kv_dtype = BF16
        model.train()
        y = torch.arange(N, device=DEV) % 5

        def step():
            model.edge_dropout.reset_calls()
            model.dropout.reset_calls()
            model.zero_grad(set_to_none=True)
            logits = model([V, graph])
            torch.nn.functional.cross_entropy(logits.view(N, -1), y).backward()
            return logits.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.requires_grad}

        logits, grads = step()
        for name, g in grads.items():
            assert torch.isfinite(g).all(), name
        monkeypatch.setattr(NodeSelfAtten, "forward", _attention_by_hand)
        want_logits, want_grads = step()
        monkeypatch.undo()
        assert torch.equal(logits, want_logits)
        for name, g in grads.items():
            assert torch.equal(g, want_grads[name]), name
    finally:
        model.self_atten.kv_dtype = None
        model.eval()
        model.zero_grad(set_to_none=True)


def test_model_kv_dtype_is_ignored_on_the_torch_path(monkeypatch):
    model, graph, V = _model_case(74)  # a page: below ROW_LINEAR_MIN_ROWS, torch's three GEMMs
    try:
        with torch.no_grad():
            base = model([V, graph])
            model.self_atten.kv_dtype = BF16
            seen = _spy_entries(monkeypatch)
            got = model([V, graph])
            assert seen == ["grl_node_attention_fwd_rows"]
        assert torch.equal(_bits(got), _bits(base))
    finally:
        model.self_atten.kv_dtype = None
