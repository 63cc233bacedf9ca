"""GPU: the forward GEMM over an X stored as bf16 (grl_linear_fwd_bf16x;
gemm_x3a_kernel).

X is one plane of the split-bf16 scheme: the kernel DMAs it as stored into one
LDS plane and issues the three plane products a b2, a b1, a b0 where
gemm_x6_kernel issues six, three of them on all-zero planes, over the same
tiles and K16 steps.  So the checks are on BITS against grl_linear_fwd_ex on
X.float() with the same path_rows: ragged row and column tiles with clamped
loads, one to four K16 steps, both weight layouts, both epilogues; a column
slice of a NaN-padded table; single products against float64; row_linear's
forward, gradients and memory; the model's emb2.  path_rows puts the small M
on the x6 path; each case first asserts that the kernel under test runs."""
import functools

import numpy as np
import pytest
import torch

import x6_isolate as xi
from grl import _lib
from grl.ops import linear_fwd_bf16x, linear_fwd_ex, row_linear

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SENTINEL = 123456.0
PR = 1 << 23

# (M, K, C, path_rows)
SHAPES = [
    (300, 48, 40, PR),    # a ragged second row tile (clamped loads), a ragged column tile; prologue, steady state, tail
    (256, 16, 256, PR),   # the whole-row-tile epilogue, nk == 1
    (1, 32, 8, 1 << 25),  # one row, every A load clamped, nk == 2 (2 R K C >= 1.6e10 needs R >= 2^25 at K C = 256)
    (513, 64, 260, PR),   # three row tiles, two column tiles of which the second is 4 columns wide
]


def _i32(t):
    return t.contiguous().view(torch.int32)


def _bits16(t):
    return t.view(torch.int16)


def _query(X, W, C, pr):
    M, K = X.shape
    return _lib.lib().grl_linear_fwd_bf16x_workspace_query(X.data_ptr(), max(X.stride(0), K), W.data_ptr(), M, K, C, pr)


def _assert_runs(X, W, C, pr):
    """The x6 path for these sizes, and the entry under test eligible."""
    M, K = X.shape
    lib = _lib.lib()
    assert lib.grl_linear_fwd_path(M, K, C, pr) == 1
    assert _query(X, W, C, pr) == lib.grl_linear_fwd_ex_workspace_size(M, K, C, pr) > 0


def _sprinkled(M, K, gen):
    """randn rounded to bf16 with about 5 % exact +0 and 5 % exact -0."""
    t = torch.randn(M, K, device=DEV, generator=gen).to(BF16)
    u = torch.rand(M, K, device=DEV, generator=gen)
    t = torch.where(u < 0.05, torch.zeros((), dtype=BF16, device=DEV), t)
    t = torch.where((u >= 0.05) & (u < 0.10), -torch.zeros((), dtype=BF16, device=DEV), t)
    return t


@functools.lru_cache(maxsize=None)
def _operands(M, K, C):
    """X, W [K, C], W^T [C, K] and the bias: made once, read-only."""
    gen = torch.Generator(device=DEV).manual_seed(M + K + C)
    X = _sprinkled(M, K, gen)
    if M * K < 256:  # 32 values: the two zeros placed by hand
        X[0, 3], X[0, 17] = 0.0, -0.0
    assert bool((_bits16(X) == -32768).any()) and bool((_bits16(X) == 0).any())
    W = torch.randn(K, C, device=DEV, generator=gen) / K ** 0.5
    b = torch.randn(C, device=DEV, generator=gen)
    return X, W, W.t().contiguous(), b


def _run(X, W, layout, b, relu, pr):
    """linear_fwd_bf16x into a sentinel-filled out (every element must be written)."""
    M, K = X.shape
    C = W.shape[0] if layout else W.shape[1]
    ws_bytes = _query(X, W, C, pr)
    assert ws_bytes > 0
    out = torch.full((M, C), SENTINEL, dtype=torch.float32, device=DEV)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    _lib.call("grl_linear_fwd_bf16x", X.data_ptr(), max(X.stride(0), K), W.data_ptr(), layout,
              b.data_ptr() if b is not None else None, out.data_ptr(), M, K, C, int(relu), pr, ws.data_ptr(), ws_bytes,
              None)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("epi", ["store", "bias_relu"])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("M,K,C,pr", SHAPES)
def test_bits_are_the_fp32_entrys_on_the_widened_x(M, K, C, pr, layout, epi, grl_option):
    grl_option("gemm_x6", 1)
    grl_option("linear_bf16x", 1)
    X, W0, W1, b = _operands(M, K, C)
    W = W1 if layout else W0
    bias, relu = (b, True) if epi == "bias_relu" else (None, False)
    _assert_runs(X, W, C, pr)
    want = linear_fwd_ex(X.float(), W, layout, bias, relu, pr)
    got = _run(X, W, layout, bias, relu, pr)
    assert bool(torch.isfinite(got).all()) and not bool((got == SENTINEL).any()) and bool(got.abs().sum() > 0)
    assert torch.equal(_i32(got), _i32(want)), f"{int((_i32(got) != _i32(want)).sum())} of {got.numel()} differ"
    assert torch.equal(_i32(_run(X, W, layout, bias, relu, pr)), _i32(got))  # two calls, equal bits
    via_ops = linear_fwd_bf16x(X, W, layout, bias, relu, pr)
    assert via_ops is not None and torch.equal(_i32(via_ops), _i32(got))


def test_independent_anchor_against_float64(grl_option):
    """Within the project's x6 bound, 1e-5 of the sum of |terms|, of the float64 product."""
    grl_option("gemm_x6", 1)
    grl_option("linear_bf16x", 1)
    M, K, C, pr = SHAPES[0]
    X, W0, _, b = _operands(M, K, C)
    _assert_runs(X, W0, C, pr)
    got = _run(X, W0, 0, b, False, pr).double().cpu()
    X64, W64, b64 = X.double().cpu(), W0.double().cpu(), b.double().cpu()
    ref = X64 @ W64 + b64
    terms = X64.abs() @ W64.abs() + b64.abs()
    assert bool(((got - ref).abs() <= 1e-5 * terms).all()), float(((got - ref).abs() / terms).max())


@pytest.mark.parametrize("layout", [0, 1])
def test_a_column_slice_of_a_nan_padded_table(layout, grl_option):
    """X 32 columns into a table K + 64 wide whose other columns hold NaN bits:
    a stray read poisons out; the table is unchanged afterwards."""
    grl_option("gemm_x6", 1)
    grl_option("linear_bf16x", 1)
    M, K, C, pr = SHAPES[0]
    X, W0, W1, b = _operands(M, K, C)
    W = W1 if layout else W0
    table = torch.full((M, K + 64), float("nan"), dtype=BF16, device=DEV)
    table[:, 32:32 + K] = X
    before = _bits16(table).clone()
    Xv = table[:, 32:32 + K]
    assert Xv.stride(0) == K + 64 and Xv.data_ptr() % 16 == 0 and not Xv.is_contiguous()
    _assert_runs(Xv, W, C, pr)
    got = _run(Xv, W, layout, b, True, pr)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(_i32(got), _i32(_run(X, W, layout, b, True, pr)))
    assert torch.equal(_bits16(table), before)


# ---- single products ---------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_single_products(layout, grl_option):
    """One-hot X rows (X[m, k(m)] a full-range bf16, the rest +0) and a
    full-mantissa fp32 W: every out[m, c] is ONE product X[m, k(m)] W[k(m), c]
    -- the three plane products a b2 + a b1 + a b0, every other term an exact
    zero -- held to xi.BARE = 2^-22 of the float64 product, so a dropped,
    duplicated or misplaced plane of W, or an A chunk landed in the wrong row
    or half, shows.  k(m) visits every K16 step and both 8-k halves from rows
    of both full row tiles' two wave rows and of the ragged third tile."""
    grl_option("gemm_x6", 1)
    grl_option("linear_bf16x", 1)
    M, K, C, pr = 530, 64, 72, PR
    rng = np.random.default_rng(5)
    k_of_m = xi.sweep(M, K, 5)
    m = np.arange(M)
    for tile, wave_row in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0)):
        sel = (m // 256 == tile) & (m % 256 // 128 == wave_row)
        assert {(k // 16, k % 16 // 8) for k in k_of_m[sel]} == {(s, hh) for s in range(K // 16) for hh in (0, 1)}
    Xn = np.zeros((M, K), np.float32)
    Xn[m, k_of_m] = xi.bf16_rne(xi.full_values(rng, M))
    Wn = xi.full_values(rng, (K, C))
    X = torch.from_numpy(Xn).to(DEV).to(BF16)
    assert torch.equal(X.float().cpu(), torch.from_numpy(Xn))  # bf16 values already: nothing was rounded
    W = torch.from_numpy(Wn.T.copy() if layout else Wn).to(DEV)
    _assert_runs(X, W, C, pr)
    got = _run(X, W, layout, None, False, pr).cpu().numpy()
    a = Xn[m, k_of_m][:, None].astype(np.float64)
    ref = a * Wn[k_of_m].astype(np.float64)
    xi.check_bound(got, ref, ref, xi.BARE, f"single products, w_layout {layout}")


# ---- row_linear ----------------------------------------------------------------
def _row_linear_case(x_is_bf16, X, W, b, g, pr):
    """(out, dX as bf16, dW, db, the forward's peak-allocation delta)."""
    x = (X if x_is_bf16 else X.float()).detach().clone().requires_grad_(True)
    w, bb = W.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    out = row_linear(x, w, bb, relu=True, path_rows=pr)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated(DEV) - base
    out.backward(g)
    dX = x.grad if x_is_bf16 else x.grad.to(BF16)
    assert dX.dtype == BF16 and w.grad.dtype == torch.float32
    return out.detach(), dX, w.grad, bb.grad, delta


def test_row_linear_reads_a_bf16_x_as_stored(grl_option):
    grl_option("gemm_x6", 1)
    grl_option("linear_bf16x", 1)
    M, K, C, pr = 5000, 512, 128, PR
    gen = torch.Generator(device=DEV).manual_seed(7)
    X = _sprinkled(M, K, gen)
    W = torch.randn(C, K, device=DEV, generator=gen) / K ** 0.5
    b = torch.randn(C, device=DEV, generator=gen)
    g = torch.randn(M, C, device=DEV, generator=gen)
    _assert_runs(X, W, C, pr)
    want = _row_linear_case(False, X, W, b, g, pr)
    got = _row_linear_case(True, X, W, b, g, pr)
    for name, a, r in zip(("out", "dX", "dW", "db"), got, want):
        assert a.shape == r.shape and a.dtype == r.dtype, name
        same = torch.equal(_bits16(a), _bits16(r)) if a.dtype == BF16 else torch.equal(_i32(a), _i32(r))
        assert same, name
    assert bool(got[0].abs().sum() > 0) and bool(got[1].float().abs().sum() > 0)
    # no widened copy: out (2.56 MB) + W's planes (0.79 MB) against the 10.24 MB an fp32 X takes
    assert got[4] < M * K * 4, got[4]
    # the option off: the widened path runs (its copy shows) and gives the same bits
    grl_option("linear_bf16x", 0)
    assert _query(X, W, C, pr) == 0
    off = _row_linear_case(True, X, W, b, g, pr)
    assert off[4] >= M * K * 4, off[4]
    for name, a, r in zip(("out", "dX", "dW", "db"), off, want):
        same = torch.equal(_bits16(a), _bits16(r)) if a.dtype == BF16 else torch.equal(_i32(a), _i32(r))
        assert same, name + " (linear_bf16x 0)"


# ---- the model -------------------------------------------------------------------
def _model_logits(N, option):
    from gnn.models import GraphCNNDropEdge
    from grl import TypedGraph

    D = 16
    torch.manual_seed(0)
    model = GraphCNNDropEdge(D, 5, 2, net_size=256, use_attention=False, dropedge_seed=7).to(DEV)
    graph = TypedGraph.synthetic(N, 4.0, 2, seed=1, device=DEV)
    V = torch.randn(1, N, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    model.activation_dtype = BF16
    model.eval()
    with _lib.options(linear_bf16x=option), torch.no_grad():
        return model([V, graph])


@pytest.mark.parametrize("N,above", [(123_000, True), (5000, False)])
def test_model_logits_do_not_depend_on_the_option(N, above, grl_option):
    """emb2 over the bf16 cat[g1, g3] (K = 512, C = 128: the x6 floor is
    122,071 nodes): read as stored with linear_bf16x = 1 above the floor,
    widened below it and with the option 0 -- the same logits bit for bit."""
    grl_option("gemm_x6", 1)
    grl_option("linear_bf16x", 1)
    probe = torch.empty(N, 512, dtype=BF16, device=DEV)
    W = torch.empty(128, 512, device=DEV)
    assert (_query(probe, W, 128, 0) > 0) == above
    on, off = _model_logits(N, 1), _model_logits(N, 0)
    assert on.dtype == torch.float32 and on.shape == (1, N, 5) and bool(torch.isfinite(on).all())
    assert torch.equal(_i32(on), _i32(off))
