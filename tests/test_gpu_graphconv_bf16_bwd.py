"""GPU: the one-kernel GraphConv data gradient over a bf16 gradient table,
writing a bf16 dX (grl_graphconv_bwd_data_bf16; graphconv_ws_bf16g_kernel),
the one-pass bf16 ReLU mask (grl_relu_grad_bf16) and the layer's backward on
them.

Widening bf16 is exact, the kernel runs the fp32 data gradient's fmaf chains
and MFMA products and rounds once in its epilogue, and the mask is a
selection, so every check here is on BITS: dX viewed as int16 equals the fp32
entry's dX on G.float() cast by torch (finite data: the same
round-to-nearest-even), G_agg, dW and db are torch.equal, and the columns
beside a slice keep their sentinel.  The shapes sit just above the x6 GEMM's
1.6e10-flop floor, as in test_gpu_graphconv_bf16_out.py; each case first
asserts through the workspace query that the one kernel runs."""
import ctypes
import functools

import pytest
import torch

from grl import DropEdge, TypedGraph, _lib
from grl.graph import current_stream_handle
from grl.ops import PREMASK_ROWS, _relu_grad_bf16, graph_conv, graph_conv_bwd_data, relu_grad, relu_grad_bf16

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SENTINEL = 0x5A5A  # a finite bf16 bit pattern no result has by chance in every column


def _bits(t):
    return t.view(torch.int16)


def _sentinel_table(N, cols):
    return torch.full((N, cols), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)


def _transpose(g, C):
    gt, eid = g.typed_transpose()
    return gt.with_dropedge(g.dropedge).csr_c(C), eid


def _ws_query(G, g, W, F, dX):
    csr, _ = _transpose(g, G.shape[1])
    return _lib.lib().grl_graphconv_bwd_data_bf16_workspace_query(
        ctypes.byref(csr), G.data_ptr(), G.stride(0), G.shape[1], W.data_ptr(), min(F, 512), dX.data_ptr(),
        dX.stride(0))


def _planes(S, C, w):
    """W's planes for a dX block w wide, and the status word."""
    return S * C * (256 if w <= 256 else 512) * 3 * 2 + 256


def _graph(N, L, has_self, deg, variant):
    de = {"plain": None, "drop_self": DropEdge(0.3, 3, 2, True), "drop_spare_self_vals": DropEdge(0.25, 9, 0, False)}
    g = TypedGraph.synthetic(N, deg, L, seed=N % 5, device=DEV)
    if variant.endswith("vals"):
        vals = torch.rand(g.nnz, generator=torch.Generator(device=DEV).manual_seed(2), device=DEV)
        g = TypedGraph(g.rowptr, g.colidx, L, vals=vals, has_self=has_self, num_cols=N)
    elif not has_self:
        g = TypedGraph(g.rowptr, g.colidx, L, has_self=False, num_cols=N)
    return g.with_dropedge(de[variant])


CASES = [
    # N, L, F (dX's width), C (the gathered width), has_self, deg
    (20_011, 6, 256, 256, True, 16.0),   # ragged last tile
    (60_001, 3, 200, 256, False, 20.0),  # no self term, ragged output width on packed stores
    (20_011, 6, 512, 512, True, 10.0),   # 4 + 8 waves, two virtual segments
    (10_007, 6, 1024, 512, True, 8.0),   # two dX column blocks written in place
    (80_000, 6, 256, 64, True, 12.0),    # one unit per virtual segment, above PREMASK_ROWS
]
VARIANTS = ["plain", "drop_self", "drop_spare_self_vals"]


@pytest.mark.parametrize("N,L,F,C,has_self,deg", CASES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_dx_bits_are_the_rounded_fp32_dx(N, L, F, C, has_self, deg, variant):
    g = _graph(N, L, has_self, deg, variant)
    gen = torch.Generator(device=DEV).manual_seed(N + F)
    K = g.segments * F
    G = torch.randn(N, C, device=DEV, generator=gen).to(BF16)
    W = torch.randn(K, C, device=DEV, generator=gen) / K ** 0.5
    want = graph_conv_bwd_data(G.float(), g, W, F)
    assert want is not None and want.dtype == torch.float32
    want = _bits(want.to(BF16))
    dX = torch.empty(N, F, dtype=BF16, device=DEV)
    assert _ws_query(G, g, W, F, dX) == _planes(g.segments, C, min(F, 512))  # the one kernel runs
    got = graph_conv_bwd_data(G, g, W, F)
    assert got is not None and got.dtype == BF16 and got.shape == (N, F) and got.is_contiguous()
    assert torch.equal(_bits(got), want)
    assert graph_conv_bwd_data(G, g, W, F, out=dX) is dX
    assert torch.equal(_bits(dX), want)  # two calls, equal bits


@functools.lru_cache(maxsize=None)
def _base():
    """The base shape's operands, shared (read-only) by the tests below."""
    N, L, F, C = 20_011, 6, 256, 256
    g = TypedGraph.synthetic(N, 16.0, L, seed=3, device=DEV).with_dropedge(DropEdge(0.3, 4, 2, True))
    gen = torch.Generator(device=DEV).manual_seed(5)
    G = torch.randn(N, C, device=DEV, generator=gen).to(BF16)
    W = torch.randn(7 * F, C, device=DEV, generator=gen) / 40
    return g, G, W, F


def test_slices_of_wider_tables_and_the_aggregate():
    g, G0, W, F = _base()
    N, C = G0.shape
    wide = _sentinel_table(N, C + 64)
    wide[:, 32:32 + C] = G0
    G = wide[:, 32:32 + C]  # a column slice: 8 B-aligned rows, ldg = C + 64
    dXf, Gagg_f, _ = graph_conv_bwd_data(G0.float(), g, W, F, want_aggregate=True)
    table = _sentinel_table(N, F + 128)
    out = table[:, 64:64 + F]
    assert _ws_query(G, g, W, F, out) == _planes(g.segments, C, F)
    dX, Gagg, g_eff = graph_conv_bwd_data(G, g, W, F, want_aggregate=True, out=out)
    assert dX is out and out.stride(0) == F + 128 and g_eff is G
    assert torch.equal(_bits(out), _bits(dXf.to(BF16)))
    assert bool((_bits(table[:, :64]) == SENTINEL).all()) and bool((_bits(table[:, 64 + F:]) == SENTINEL).all())
    assert Gagg.dtype == torch.float32 and torch.equal(Gagg, Gagg_f)
    assert bool((_bits(wide[:, :32]) == SENTINEL).all()) and bool((_bits(wide[:, 32 + C:]) == SENTINEL).all())
    # through the ReLU below PREMASK_ROWS: the selection is exact on bf16
    R = torch.randn(N, C, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)).to(BF16)
    assert N < PREMASK_ROWS
    want = graph_conv_bwd_data(G0.float(), g, W, F, R.float()).to(BF16)
    assert torch.equal(_bits(graph_conv_bwd_data(G, g, W, F, R)), _bits(want))


def test_self_term_for_the_first_rows_only():
    """g_rows = N // 2: transpose rows beyond carry no self term (a shard's
    halo rows), in the bf16 entry as in the fp32 one."""
    g, G, W, F = _base()
    N, C = G.shape
    csr, eid = _transpose(g, C)
    half = N // 2
    Gf = G.float()
    de = ctypes.byref(g.dropedge.to_c())
    stream = current_stream_handle(DEV)
    lib = _lib.lib()
    ws_bytes = lib.grl_graphconv_bwd_data_workspace_query(ctypes.byref(csr), Gf.data_ptr(), C, C, W.data_ptr(), F)
    dX16 = torch.empty(N, F, dtype=BF16, device=DEV)
    assert ws_bytes and ws_bytes == lib.grl_graphconv_bwd_data_bf16_workspace_query(
        ctypes.byref(csr), G.data_ptr(), C, C, W.data_ptr(), F, dX16.data_ptr(), F)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    dX32 = torch.empty(N, F, device=DEV)
    _lib.call("grl_graphconv_bwd_data", ctypes.byref(csr), eid.data_ptr(), Gf.data_ptr(), C, half, C, W.data_ptr(), F,
              dX32.data_ptr(), None, de, ws.data_ptr(), ws_bytes, stream)
    _lib.call("grl_graphconv_bwd_data_bf16", ctypes.byref(csr), eid.data_ptr(), G.data_ptr(), C, half, C,
              W.data_ptr(), F, dX16.data_ptr(), F, None, de, ws.data_ptr(), ws_bytes, stream)
    assert torch.equal(_bits(dX16), _bits(dX32.to(BF16)))
    full = graph_conv_bwd_data(G, g, W, F)
    assert torch.equal(_bits(dX16[:half]), _bits(full[:half]))  # rows below half: the same sums
    assert not torch.equal(_bits(dX16[half:]), _bits(full[half:]))  # the self term is what differs


@pytest.mark.parametrize("M,C", [(70_001, 256), (5, 8)])
def test_relu_grad_bf16_is_relu_grad_on_the_widened_operands(M, C, monkeypatch):
    import grl.ops as ops

    monkeypatch.setattr(ops, "PREMASK_ROWS", 1)  # the (5, 8) case through grl_relu_grad too
    gen = torch.Generator(device=DEV).manual_seed(M)
    g = torch.randn(M, C, device=DEV, generator=gen).to(BF16)
    out = torch.relu(torch.randn(M, C, device=DEV, generator=gen)).to(BF16)
    out[0, 0] = -0.0  # not > 0
    want, _, want_db = relu_grad(g.float(), out.float(), True)
    g16, g32, db = relu_grad_bf16(g, out, True, True)
    assert g16.dtype == BF16 and g32.dtype == torch.float32 and g32.is_contiguous()
    assert torch.equal(g32, want) and torch.equal(_bits(g16), _bits(want.to(BF16))) and torch.equal(db, want_db)
    assert bool((_bits(g16)[out <= 0] == 0).all())  # masked entries are +0
    # each output NULL in turn
    a, b, c = relu_grad_bf16(g, out, False, True)
    assert c is None and torch.equal(b, want) and torch.equal(_bits(a), _bits(g16))
    a, b, c = relu_grad_bf16(g, out, True, False)
    assert b is None and torch.equal(c, want_db) and torch.equal(_bits(a), _bits(g16))
    a, b, c = _relu_grad_bf16(g, out, True, True, want_16=False)
    assert a is None and torch.equal(b, want) and torch.equal(c, want_db)
    # strided inputs, a strided g_eff16 beside sentinels
    gw, ow = _sentinel_table(M, C + 8), _sentinel_table(M, 2 * C)
    gw[:, 4:4 + C] = g
    ow[:, C:] = out
    table = _sentinel_table(M, C + 16)
    a, b, c = _relu_grad_bf16(gw[:, 4:4 + C], ow[:, C:], True, True, g_eff16=table[:, 8:8 + C])
    assert torch.equal(_bits(a), _bits(g16)) and torch.equal(b, want) and torch.equal(c, want_db)
    assert bool((_bits(table[:, :8]) == SENTINEL).all()) and bool((_bits(table[:, 8 + C:]) == SENTINEL).all())
    # in place: g_eff16 aliasing g
    gi = gw[:, 4:4 + C]
    a, b, c = _relu_grad_bf16(gi, ow[:, C:], True, True, g_eff16=gi)
    assert a is gi and torch.equal(_bits(gi), _bits(g16)) and torch.equal(b, want) and torch.equal(c, want_db)
    assert bool((_bits(gw[:, :4]) == SENTINEL).all()) and bool((_bits(gw[:, 4 + C:]) == SENTINEL).all())


def _layer(Xb, g, W0, b0, R, grads=(True, True, True), relu=True):
    X, W, b = (t.clone().requires_grad_(r) for t, r in zip((Xb, W0, b0), grads))
    out = graph_conv(X, g, W, b, relu=relu, out_dtype=BF16)
    out.backward(R)
    return out.detach(), X.grad, W.grad, b.grad


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


def _eligible(g, R, W, F):
    dX = torch.empty(g.num_cols, F, dtype=BF16, device=DEV)
    return _ws_query(R, g, W, F, dX) == _planes(g.segments, R.shape[1], F)


@pytest.mark.parametrize("N,L,F,C", [(80_000, 6, 256, 64), (20_011, 6, 256, 256)])
def test_layer_gradients_are_the_widened_backwards_bits(N, L, F, C, grl_option):
    g, Xb, W, b, R = _layer_case(N, L, F, C)
    assert _eligible(g, R, W, F)
    grl_option("graphconv_bwd_bf16", 1)
    got = _layer(Xb, g, W, b, R)
    grl_option("graphconv_bwd_bf16", 0)
    assert not _eligible(g, R, W, F)
    ref = _layer(Xb, g, W, b, R)
    assert got[1].dtype == BF16 and got[1].shape == Xb.shape
    assert torch.equal(_bits(got[0]), _bits(ref[0])), "out"
    assert torch.equal(_bits(got[1]), _bits(ref[1])), "dX"
    assert torch.equal(got[2], ref[2]), "dW"
    assert torch.equal(got[3], ref[3]), "db"
    assert bool(got[1].float().abs().sum() > 0)


def test_backward_allocates_no_fp32_dx(grl_option):
    """X.grad alone at (80_000, 6, 256, 64): the path's own buffers are the
    masked bf16 gradient [N, C], the bf16 dX [N, F] and W's planes; an fp32
    [N, F] dX (the widened path has one, and rounds it) does not fit on top."""
    N, L, F, C = 80_000, 6, 256, 64
    g, Xb, W, b, R = _layer_case(N, L, F, C)
    grl_option("graphconv_bwd_bf16", 1)
    assert _eligible(g, R, W, F) and N >= PREMASK_ROWS
    _layer(Xb, g, W, b, R, grads=(True, False, False))  # warm: the graph's cached transpose exists
    X = Xb.clone().requires_grad_(True)
    out = graph_conv(X, g, W, b, relu=True, out_dtype=BF16)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out.backward(R)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    own = N * C * 2 + N * F * 2 + _planes(g.segments, C, F)
    assert X.grad.dtype == BF16
    assert extra < own + N * F * 4, (f"the backward allocated {extra} bytes; its own buffers are {own}, an fp32 dX "
                                     f"{N * F * 4}")


def test_rows_off_the_load_and_store_grids_fall_back_to_the_same_bits():
    g, G, W, F = _base()
    N, C = G.shape
    want = graph_conv_bwd_data(G, g, W, F)
    table = _sentinel_table(N, F + 8)
    out = table[:, 1:1 + F]
    assert out.data_ptr() % 4 == 2
    assert graph_conv_bwd_data(G, g, W, F, out=out) is None  # no dword stores: the caller widens
    assert bool((_bits(table) == SENTINEL).all())
    wide = _sentinel_table(N, C + 8)
    wide[:, 1:1 + C] = G
    assert wide[:, 1:1 + C].data_ptr() % 8 == 2
    assert graph_conv_bwd_data(wide[:, 1:1 + C], g, W, F) is None  # no 8 B loads
    # autograd with such an upstream gradient (no ReLU: the gradient is gathered as handed over, so the
    # backward widens it instead; with the ReLU the masked copy is a new, aligned tensor): the same bits
    g, Xb, W, b, R = _layer_case(20_011, 6, 256, 256)
    wide = _sentinel_table(N, C + 8)
    wide[:, 1:1 + C] = R
    Rv = wide[:, 1:1 + C]
    assert Rv.data_ptr() % 8 == 2 and not _eligible(g, Rv, W, F) and _eligible(g, R, W, F)
    for relu in (False, True):
        ref = _layer(Xb, g, W, b, R, relu=relu)
        got = _layer(Xb, g, W, b, Rv, relu=relu)
        assert torch.equal(_bits(got[1]), _bits(ref[1])) and torch.equal(got[2], ref[2])
        assert torch.equal(got[3], ref[3])


def test_a_misaligned_g_through_the_relu_is_gathered_from_its_masked_copy():
    """With relu_out the kernel gathers the masked copy, a new contiguous
    tensor: the query is asked for that, so g's own address does not refuse."""
    g, G, W, F = _base()
    N, C = G.shape
    R = torch.randn(N, C, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)).to(BF16)
    wide = _sentinel_table(N, C + 8)
    wide[:, 1:1 + C] = G
    Gv = wide[:, 1:1 + C]
    assert Gv.data_ptr() % 8 == 2 and graph_conv_bwd_data(Gv, g, W, F) is None
    got = graph_conv_bwd_data(Gv, g, W, F, R)
    assert got is not None and torch.equal(_bits(got), _bits(graph_conv_bwd_data(G, g, W, F, R)))


@pytest.mark.parametrize("relu", [True, False])
def test_an_expanded_gradient_gives_the_widened_backwards_bits(relu, grl_option):
    """A sum over nodes hands the layer an expanded gradient (row stride 0)
    at M >= PREMASK_ROWS: copied once, then the bf16 entries; the same bits
    as under option 0."""
    N, L, F, C = 80_000, 6, 256, 64
    g, Xb, W0, b0, _ = _layer_case(N, L, F, C)
    assert N >= PREMASK_ROWS
    v = torch.randn(C, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    res = {}
    for option in (1, 0):
        grl_option("graphconv_bwd_bf16", option)
        X, W, b = (t.clone().requires_grad_(True) for t in (Xb, W0, b0))
        out = graph_conv(X, g, W, b, relu=relu, out_dtype=BF16)
        strides = []
        out.register_hook(lambda gr: strides.append((gr.dtype, gr.stride())))
        (out.sum(0).float() * v).sum().backward()
        assert strides == [(BF16, (0, 1))]  # what the node was handed
        res[option] = (X.grad, W.grad, b.grad)
    assert res[1][0].dtype == BF16 and bool(res[1][0].float().abs().sum() > 0)
    assert torch.equal(_bits(res[1][0]), _bits(res[0][0])), "dX"
    assert torch.equal(res[1][1], res[0][1]) and torch.equal(res[1][2], res[0][2])
    with pytest.raises(_lib.GrlError, match="row stride"):
        relu_grad_bf16(torch.zeros(1, C, dtype=BF16, device=DEV).expand(N, C), torch.zeros(N, C, dtype=BF16, device=DEV))
    assert graph_conv_bwd_data(torch.zeros(1, C, dtype=BF16, device=DEV).expand(N, C), g, W0, F) is None


def test_dtype_errors():
    g, G, W, F = _base()
    N = G.shape[0]
    with pytest.raises(_lib.GrlError, match="no mixed form"):
        graph_conv_bwd_data(G.float(), g, W, F, out=torch.empty(N, F, dtype=BF16, device=DEV))
    with pytest.raises(_lib.GrlError, match="no mixed form"):
        graph_conv_bwd_data(G, g, W, F, out=torch.empty(N, F, device=DEV))
    with pytest.raises(_lib.GrlError, match="out= is a bfloat16 dX"):
        graph_conv_bwd_data(G.float(), g, W, F, out=torch.empty(N, F, device=DEV))
    with pytest.raises(_lib.GrlError, match="unit column stride"):
        graph_conv_bwd_data(G, g, W, F, out=torch.empty(F, N, dtype=BF16, device=DEV).t())
