"""GPU: the weight gradient dW = Z^T g over a bf16 output gradient read as
stored (grl_linear_bwd_weight_bf16g; gemm_x3t_kernel) and the
GraphConv layer's backward on it.

A bf16 g is one plane of the split-bf16 scheme: the kernel issues the three
plane products a2 b, a1 b, a0 b where gemm_x6t_kernel issues six, three of them
on all-zero planes, over the same K16 steps, splits and slab order.  So the
checks are on BITS against grl_linear_bwd_weight on g.float(); the shapes are
the smallest above the x6t floor 2 M K C >= 1.6e10 that reach the ragged last
K16 step, ragged row and column tiles with clamped loads, and the one-split
store epilogue.  Each case first asserts through the workspace query that the
kernel under test runs."""
import functools

import numpy as np
import pytest
import torch

import grl.ops
import x6_isolate as xi
from grl import DropEdge, TypedGraph, _lib
from grl.ops import PREMASK_ROWS, graph_conv, linear_bwd_weight, linear_bwd_weight_bf16

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SENTINEL = 0x5A5A  # a finite bf16 bit pattern

SHAPES = [
    (20_011, 1792, 256),  # the layer's shape class; M % 16 == 11: a ragged last K16 step; ~70 splits
    (60_001, 1400, 100),  # ragged dW row tiles, a ragged column tile with clamped loads
    (250, 8192, 4096),    # one split at 256 CUs: the store epilogue, no slab reduce; M % 16 == 10
]


def _i32(t):
    return t.contiguous().view(torch.int32)


def _bits16(t):
    return t.view(torch.int16)


def _query(Z, g):
    return _lib.lib().grl_linear_bwd_weight_bf16g_workspace_query(Z.data_ptr(), Z.stride(0), g.data_ptr(), g.stride(0),
                                                                 Z.shape[0], Z.shape[1], g.shape[1])


@functools.lru_cache(maxsize=None)
def _operands(M, K, C):
    """Z = randn, g = randn.to(bf16) with a sprinkling of exact +0 and -0, and
    the fp32 entry's (dW, db) on the widened g: made once, read-only."""
    gen = torch.Generator(device=DEV).manual_seed(M + K + C)
    Z = torch.randn(M, K, device=DEV, generator=gen)
    g = torch.randn(M, C, device=DEV, generator=gen).to(BF16)
    u = torch.rand(M, C, device=DEV, generator=gen)
    g = torch.where(u < 0.05, torch.zeros((), dtype=BF16, device=DEV), g)
    g = torch.where((u >= 0.05) & (u < 0.10), -torch.zeros((), dtype=BF16, device=DEV), g)
    assert bool((_bits16(g) == -32768).any()) and bool((_bits16(g) == 0).any())  # -0 and +0 are there
    ref = linear_bwd_weight(Z, g.float(), None, True)
    return Z, g, ref


@pytest.mark.parametrize("M,K,C", SHAPES)
def test_bits_are_the_fp32_entrys_on_the_widened_g(M, K, C, grl_option):
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16g", 1)
    assert 2 * M * K * C >= 1.6e10
    Z, g, (dW_ref, db_ref) = _operands(M, K, C)
    assert _query(Z, g) == _lib.lib().grl_linear_bwd_weight_workspace_size(M, K, C) > 0  # the kernel under test runs
    res = linear_bwd_weight_bf16(Z, g, True)
    assert res is not None
    dW, db = res
    assert dW.shape == (K, C) and db.shape == (C,) and dW.dtype == db.dtype == torch.float32
    assert bool(torch.isfinite(dW).all()) and bool(dW.abs().sum() > 0)
    assert torch.equal(_i32(dW), _i32(dW_ref)), f"dW: {int((_i32(dW) != _i32(dW_ref)).sum())} elements differ"
    assert torch.equal(_i32(db), _i32(db_ref)), "db"
    dW2, db2 = linear_bwd_weight_bf16(Z, g, True)  # two calls, equal bits
    assert torch.equal(_i32(dW2), _i32(dW)) and torch.equal(_i32(db2), _i32(db))
    dW3, none = linear_bwd_weight_bf16(Z, g, False)  # db = NULL is accepted
    assert none is None and torch.equal(_i32(dW3), _i32(dW))


@pytest.mark.parametrize("M,K,C", SHAPES[:2])
def test_strided_operands(M, K, C, grl_option):
    """g a column slice of a wider sentinel-filled bf16 table (ldg = C + 64, 32
    columns in), Z a slice with ldz > K: the contiguous call's bits, and the
    table's other columns are untouched (g is only read)."""
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16g", 1)
    Z, g, (dW_ref, db_ref) = _operands(M, K, C)
    table = torch.full((M, C + 64), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)
    table[:, 32:32 + C] = g
    gv = table[:, 32:32 + C]
    Zw = torch.full((M, K + 24), float("nan"), device=DEV)  # a stray read of the padding would poison dW
    Zw[:, 8:8 + K] = Z
    Zv = Zw[:, 8:8 + K]
    assert gv.stride(0) == C + 64 and gv.data_ptr() % 8 == 0 and Zv.stride(0) == K + 24 and Zv.data_ptr() % 16 == 0
    assert _query(Zv, gv) > 0
    dW, db = linear_bwd_weight_bf16(Zv, gv, True)
    assert torch.equal(_i32(dW), _i32(dW_ref)) and torch.equal(_i32(db), _i32(db_ref))
    assert bool((_bits16(table[:, :32]) == SENTINEL).all()) and bool((_bits16(table[:, 32 + C:]) == SENTINEL).all())
    assert torch.equal(_bits16(table[:, 32:32 + C]), _bits16(g))


# ---- single products ---------------------------------------------------------
BWD_SHAPE = (17_443, 1792, 256)  # test_gpu_x6_planes.py's: just above the floor, M 3 past a multiple of 16


def _rows_over(n, M):
    """n rows spread evenly over [0, M), the first three moved to the last
    three rows: every 256-row stretch (a split-K slab is at least that long)
    and the final, partial K16 step hold one."""
    r = (np.arange(n, dtype=np.int64) * M) // n
    r[:3] = [M - 1, M - 2, M - 3]
    assert len(np.unique(r)) == n and len(np.unique(r // 256)) == -(-M // 256) and (r >= M // 16 * 16).sum() == 3
    return r


def _full(shape, gen):
    """randn * 2^randint(-8, 9) on the device: full-mantissa fp32 values."""
    scale = torch.pow(2.0, torch.randint(-8, 9, shape, device=DEV, generator=gen).float())
    v = torch.randn(shape, device=DEV, generator=gen) * scale
    return torch.where(v == 0, torch.full_like(v, 1 + 2.0 ** -23), v)


def _full16(shape, gen):
    """the same rounded to bf16 (never 0: a rounding does not reach 0 from a normal value)."""
    return _full(shape, gen).to(BF16)


def _check(got, a, b, what):
    ref = (a.double() * b.double()).cpu().numpy()
    return xi.check_bound(got.cpu().numpy(), ref, ref, xi.BARE, what)


@pytest.mark.parametrize("variant", ["z_one_hot", "g_one_hot"])
def test_single_products(variant, grl_option):
    """Every dW[k, c] is ONE product Z[r, k] g[r, c] (all other terms add exact
    zeros), held to 2^-22 of the float64 product: since a0 + a1 + a2 == a and
    g is one plane, the three products alone sit far inside it, and a dropped
    or misplaced a2 b or a1 b (2^-16, 2^-8 of the term) breaks it."""
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16g", 1)
    M, K, C = BWD_SHAPE
    assert M % 16 == 3 and 2 * M * K * C >= 1.6e10
    gen = torch.Generator(device=DEV).manual_seed(11)
    if variant == "z_one_hot":  # dW[k, c] = Z[r(k), k] g[r(k), c]
        g = _full16((M, C), gen)
        r = torch.from_numpy(_rows_over(K, M)).to(DEV)
        k = torch.arange(K, device=DEV)
        Z = torch.zeros(M, K, device=DEV)
        Z[r, k] = _full((K,), gen)
        a, b = Z[r, k][:, None], g[r].float()
    else:  # dW[k, c] = Z[r(c), k] g[r(c), c]
        Z = _full((M, K), gen)
        r = torch.from_numpy(_rows_over(C, M)).to(DEV)
        c = torch.arange(C, device=DEV)
        g = torch.zeros(M, C, dtype=BF16, device=DEV)
        g[r, c] = _full16((C,), gen)
        a, b = Z[r].t(), g[r, c].float()[None, :]
    assert _query(Z, g) > 0
    dW, db = linear_bwd_weight_bf16(Z, g, True)
    worst = _check(dW, a, b, f"dW, {variant}")
    ref = g.double().sum(0)  # the fp32 column sum, as test_gpu_x6_planes.py holds it: 1e-5 of sum |terms|
    xi.check_bound(db.cpu().numpy(), ref.cpu().numpy(), g.double().abs().sum(0).cpu().numpy(), 1e-5, "db")
    # the MFMA kernel ran: the fp32 GEMM (gemm_x6 = 0), whose single products are correctly rounded, gives other bits
    grl_option("gemm_x6", 0)
    assert _query(Z, g) == 0
    other = linear_bwd_weight(Z, g.float(), None, False)[0]
    grl_option("gemm_x6", 1)
    assert not torch.equal(other, dW), "the fp32 GEMM's bits -- gemm_x3t_kernel did not run"
    print(f"gemm_x3t dW {variant}: worst error {worst:.3f} x 2^-22 |a b|")


# ---- the layer -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layer_case(N, L, F, C):
    g = TypedGraph.synthetic(N, 12.0, L, seed=3, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(N + C)
    Xb = torch.randn(N, F, device=DEV, generator=gen).to(BF16)
    K = g.segments * F
    W = torch.randn(K, C, device=DEV, generator=gen) / K ** 0.5
    b = torch.randn(C, device=DEV, generator=gen)
    R = torch.randn(N, C, device=DEV, generator=gen).to(BF16)
    return g, Xb, W, b, R


def _layer(Xb, g, W0, b0, R, relu=True, recompute=False):
    X, W, b = (t.clone().requires_grad_(True) for t in (Xb, W0, b0))
    out = graph_conv(X, g, W, b, relu=relu, out_dtype=BF16, recompute=recompute)
    out.backward(R)
    return X.grad, W.grad, b.grad


def _same(got, ref, what):
    assert got[0].dtype == BF16 and torch.equal(_bits16(got[0]), _bits16(ref[0])), f"{what}: dX"
    assert torch.equal(_i32(got[1]), _i32(ref[1])), f"{what}: dW"
    assert torch.equal(_i32(got[2]), _i32(ref[2])), f"{what}: db"


class _Spy:
    """Records the calls of grl.ops' two helpers the backward chooses between."""

    def __init__(self, monkeypatch):
        self.want_f32, self.dw16 = [], []
        relu_grad, dw = grl.ops._relu_grad_bf16, grl.ops.linear_bwd_weight_bf16

        def relu_grad_spy(g, out, want_db, want_f32, *a, **kw):
            self.want_f32.append(want_f32)
            return relu_grad(g, out, want_db, want_f32, *a, **kw)

        def dw_spy(*a, **kw):
            res = dw(*a, **kw)
            self.dw16.append(res is not None)
            return res

        monkeypatch.setattr(grl.ops, "_relu_grad_bf16", relu_grad_spy)
        monkeypatch.setattr(grl.ops, "linear_bwd_weight_bf16", dw_spy)


# (N, L, F, C): above PREMASK_ROWS with 2 N 7F C = 1.8e10 (the one-pass mask); below it (torch.where)
LAYERS = [(80_000, 6, 64, 256), (20_011, 6, 256, 256)]


@pytest.mark.parametrize("p", [0.3, 0.0])
@pytest.mark.parametrize("N,L,F,C", LAYERS)
def test_layer_gradients_keep_their_bits(N, L, F, C, p, grl_option, monkeypatch):
    """graph_conv(Xb, ..., relu=True, out_dtype=bfloat16) forward + backward:
    dX, dW and db bitwise equal between dw_bf16g 0 and 1, with DropEdge and
    without, and with recompute=True.  From PREMASK_ROWS rows option 1 takes
    the bf16 dW (the mask pass is asked for no fp32 output); below them the
    widened path's dW masks on its loads in the fp32-MFMA kernel, so the
    backward keeps that GEMM to keep its bits.  Without a ReLU the bf16 dW
    runs at either size."""
    grl_option("gemm_x6", 1)
    g, Xb, W, b, R = _layer_case(N, L, F, C)
    assert 2 * N * g.segments * F * C >= 1.6e10
    if p > 0:
        g = g.with_dropedge(DropEdge(p, 4, 2, True))
    premask = N >= PREMASK_ROWS
    for relu in (True, False):
        grl_option("dw_bf16g", 0)
        ref = _layer(Xb, g, W, b, R, relu=relu)
        grl_option("dw_bf16g", 1)
        spy = _Spy(monkeypatch)
        got = _layer(Xb, g, W, b, R, relu=relu)
        _same(got, ref, f"relu={relu}")
        assert bool(got[1].abs().sum() > 0) and bool(got[2].abs().sum() > 0)
        if premask or not relu:
            assert spy.dw16 == [True], "the bf16 dW did not run"
        else:
            assert spy.dw16 == []
        if relu and premask:  # no fp32 [N, C] tensor: the one pass writes the bf16 gradient and db only
            assert spy.want_f32 == [False]
        if relu and p > 0:
            _same(_layer(Xb, g, W, b, R, relu=True, recompute=True), ref, "recompute")
        monkeypatch.undo()


def test_backward_makes_no_fp32_gradient_copy(grl_option):
    """At N >= PREMASK_ROWS with the option on, the backward's own buffers are
    the masked bf16 gradient [N, C], the bf16 dX [N, F], W's planes, dW and the
    dW workspace; an fp32 [N, C] copy of the gradient does not fit on top."""
    N, L, F, C = LAYERS[0]
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16g", 1)
    g, Xb, W0, b0, R = _layer_case(N, L, F, C)
    assert N >= PREMASK_ROWS
    _layer(Xb, g, W0, b0, R)  # warm: the graph's cached transpose exists
    X, W, b = (t.clone().requires_grad_(True) for t in (Xb, W0, b0))
    out = graph_conv(X, g, W, b, relu=True, out_dtype=BF16)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out.backward(R)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    K = g.segments * F
    planes = g.segments * C * 256 * 3 * 2 + 256  # W's planes for the data gradient, and the status word
    own = (N * C * 2 + N * F * 2 + planes + K * C * 4 + _lib.lib().grl_linear_bwd_weight_workspace_size(N, K, C)
           + _lib.lib().grl_relu_grad_workspace_size(N, C) + 2 * C * 4)
    assert extra < own + N * C * 4, (f"the backward allocated {extra} bytes; its own buffers are {own}, an fp32 copy "
                                     f"of the gradient {N * C * 4}")


@pytest.mark.parametrize("case", ["g_off_the_8B_grid", "C_not_a_multiple_of_4", "M_below_the_floor", "dw_bf16g_0",
                                  "gemm_x6_0"])
def test_fallbacks_keep_the_bits(case, grl_option):
    """Where the query is 0, linear_bwd_weight_bf16 returns None, and the
    layer's backward still yields the widened path's dW and db."""
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16g", 1)
    M, K, C = SHAPES[0]
    Z, g, _ = _operands(M, K, C)
    if case == "g_off_the_8B_grid":
        wide = torch.zeros(M, C + 8, dtype=BF16, device=DEV)
        wide[:, 1:1 + C] = g
        g = wide[:, 1:1 + C]
        assert g.data_ptr() % 8 == 2
    elif case == "C_not_a_multiple_of_4":
        g = g[:, :C - 2].contiguous()
    elif case == "M_below_the_floor":
        Z, g = Z[:17_000], g[:17_000]
        assert 2 * 17_000 * K * C < 1.6e10
    elif case == "dw_bf16g_0":
        grl_option("dw_bf16g", 0)
    else:
        grl_option("gemm_x6", 0)
    assert _query(Z, g) == 0
    assert linear_bwd_weight_bf16(Z, g, True) is None
    # the layer at the case's conditions (no ReLU: the gradient is read as handed over) against the widened
    # backward -- g.float() through grl_linear_bwd_weight, both bf16 backward options off
    N, L, F, C = {"C_not_a_multiple_of_4": (20_011, 6, 256, 254), "M_below_the_floor": (17_000, 6, 256, 256)}.get(
        case, LAYERS[1])
    gr, Xb, W, b, R = _layer_case(N, L, F, C)
    Rv = R
    if case == "g_off_the_8B_grid":
        wide = torch.zeros(N, C + 8, dtype=BF16, device=DEV)
        wide[:, 1:1 + C] = R
        Rv = wide[:, 1:1 + C]
        assert Rv.data_ptr() % 8 == 2
    got = _layer(Xb, gr, W, b, Rv, relu=False)
    grl_option("dw_bf16g", 0)
    grl_option("graphconv_bwd_bf16", 0)
    ref = _layer(Xb, gr, W, b, R, relu=False)
    _same(got, ref, case)


def test_wrapper_refuses_what_the_entry_cannot_read():
    M, K, C = 64, 32, 16
    Z = torch.zeros(M, K, device=DEV)
    g = torch.zeros(M, C, dtype=BF16, device=DEV)
    assert linear_bwd_weight_bf16(Z, g, True) is None  # well-formed, far below the floor
    for bad in (g.float(), g[0], g.t().contiguous().t(), g[:1].expand(M, C)):
        with pytest.raises(_lib.GrlError, match="linear_bwd_weight_bf16: g must be"):
            linear_bwd_weight_bf16(Z, bad, True)
    for bad in (Z.to(BF16), Z[:M - 1], Z.t().contiguous().t()):
        with pytest.raises(_lib.GrlError, match="linear_bwd_weight_bf16: Z must be"):
            linear_bwd_weight_bf16(bad, g, True)


def test_empty_operands():
    """M == 0: dW = 0 and db = 0 (an empty node-range shard); db = NULL accepted."""
    K, C = 64, 32
    lib = _lib.lib()
    from grl.graph import current_stream_handle
    dW = torch.full((K, C), 7.0, device=DEV)
    db = torch.full((C,), 7.0, device=DEV)
    st = current_stream_handle(DEV)
    assert lib.grl_linear_bwd_weight_bf16g(None, K, None, C, dW.data_ptr(), db.data_ptr(), 0, K, C, None, 0,
                                           st) == _lib.GRL_OK
    torch.cuda.synchronize()
    assert not bool(dW.any()) and not bool(db.any())
    dW.fill_(7.0)
    assert lib.grl_linear_bwd_weight_bf16g(None, K, None, C, dW.data_ptr(), None, 0, K, C, None, 0, st) == _lib.GRL_OK
    torch.cuda.synchronize()
    assert not bool(dW.any())
