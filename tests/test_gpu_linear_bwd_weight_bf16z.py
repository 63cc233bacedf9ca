"""GPU: the weight gradient dW = Z^T g with BOTH operands bf16 and read as
stored (grl_linear_bwd_weight_bf16zg; gemm_x1t_kernel).

Both operands are one plane of the split-bf16 scheme: the kernel issues the one
plane product a0 b where gemm_x6t_kernel issues six, five of them on all-zero
planes, over the same K16 steps, splits and slab order.  So the checks are on
BITS against grl_linear_bwd_weight on Z.float(), g.float(); the shapes are
test_gpu_linear_bwd_weight_bf16.py's (a ragged last K16 step, ragged row and
column tiles with clamped loads, the one-split store epilogue).  Each case
first asserts through the workspace query that the kernel under test runs."""
import functools

import numpy as np
import pytest
import torch

import x6_isolate as xi
from grl import _lib
from grl.ops import linear_bwd_weight, linear_bwd_weight_bf16z

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SENTINEL = 0x5A5A

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
    return _lib.lib().grl_linear_bwd_weight_bf16zg_workspace_query(Z.data_ptr(), Z.stride(0), g.data_ptr(), g.stride(0),
                                                                  Z.shape[0], Z.shape[1], g.shape[1])


def _sprinkled(M, C, gen):
    """randn rounded to bf16 with exact +0 and -0 sprinkled in."""
    t = torch.randn(M, C, device=DEV, generator=gen).to(BF16)
    u = torch.rand(M, C, device=DEV, generator=gen)
    t = torch.where(u < 0.05, torch.zeros((), dtype=BF16, device=DEV), t)
    t = torch.where((u >= 0.05) & (u < 0.10), -torch.zeros((), dtype=BF16, device=DEV), t)
    assert bool((_bits16(t) == -32768).any()) and bool((_bits16(t) == 0).any())
    return t


@functools.lru_cache(maxsize=None)
def _operands(M, K, C):
    """Z, g and the fp32 entry's (dW, db) on the widened operands: made once, read-only."""
    gen = torch.Generator(device=DEV).manual_seed(M + K + C)
    Z, g = _sprinkled(M, K, gen), _sprinkled(M, C, gen)
    return Z, g, linear_bwd_weight(Z.float(), g.float(), None, True)


@pytest.mark.parametrize("M,K,C", SHAPES)
def test_bits_are_the_fp32_entrys_on_the_widened_operands(M, K, C, grl_option):
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16z", 1)
    assert 2 * M * K * C >= 1.6e10
    Z, g, (dW_ref, db_ref) = _operands(M, K, C)
    assert _query(Z, g) == _lib.lib().grl_linear_bwd_weight_workspace_size(M, K, C) > 0  # the kernel under test runs
    res = linear_bwd_weight_bf16z(Z, g, True)
    assert res is not None
    dW, db = res
    assert dW.shape == (K, C) and db.shape == (C,) and dW.dtype == db.dtype == torch.float32
    assert bool(torch.isfinite(dW).all()) and bool(dW.abs().sum() > 0)
    assert torch.equal(_i32(dW), _i32(dW_ref)), f"dW: {int((_i32(dW) != _i32(dW_ref)).sum())} elements differ"
    assert torch.equal(_i32(db), _i32(db_ref)), "db"
    dW2, db2 = linear_bwd_weight_bf16z(Z, g, True)  # two calls, equal bits
    assert torch.equal(_i32(dW2), _i32(dW)) and torch.equal(_i32(db2), _i32(db))
    dW3, none = linear_bwd_weight_bf16z(Z, g, False)  # db = NULL is accepted
    assert none is None and torch.equal(_i32(dW3), _i32(dW))


@pytest.mark.parametrize("M,K,C", SHAPES[:2])
def test_strided_operands(M, K, C, grl_option):
    """Column slices of wider tables: g in a sentinel table (untouched), Z
    inside NaN padding that would poison a stray read."""
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16z", 1)
    Z, g, (dW_ref, db_ref) = _operands(M, K, C)
    table = torch.full((M, C + 64), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)
    table[:, 32:32 + C] = g
    gv = table[:, 32:32 + C]
    Zw = torch.full((M, K + 24), float("nan"), dtype=BF16, device=DEV)
    Zw[:, 8:8 + K] = Z
    Zv = Zw[:, 8:8 + K]
    assert gv.stride(0) == C + 64 and gv.data_ptr() % 8 == 0 and Zv.stride(0) == K + 24 and Zv.data_ptr() % 8 == 0
    assert _query(Zv, gv) > 0
    dW, db = linear_bwd_weight_bf16z(Zv, gv, True)
    assert torch.equal(_i32(dW), _i32(dW_ref)) and torch.equal(_i32(db), _i32(db_ref))
    assert bool((_bits16(table[:, :32]) == SENTINEL).all()) and bool((_bits16(table[:, 32 + C:]) == SENTINEL).all())
    assert torch.equal(_bits16(table[:, 32:32 + C]), _bits16(g))


# ---- single products ---------------------------------------------------------
BWD_SHAPE = (17_443, 1792, 256)  # test_gpu_x6_planes.py's: just above the floor, M 3 past a multiple of 16


def _rows_over(n, M):
    """n rows spread evenly over [0, M), the first three moved to the last three rows."""
    r = (np.arange(n, dtype=np.int64) * M) // n
    r[:3] = [M - 1, M - 2, M - 3]
    assert len(np.unique(r)) == n and len(np.unique(r // 256)) == -(-M // 256) and (r >= M // 16 * 16).sum() == 3
    return r


def _full16(shape, gen):
    """randn * 2^randint(-8, 9) rounded to bf16 (never 0)."""
    scale = torch.pow(2.0, torch.randint(-8, 9, shape, device=DEV, generator=gen).float())
    v = torch.randn(shape, device=DEV, generator=gen) * scale
    return torch.where(v == 0, torch.full_like(v, 1.0), v).to(BF16)


@pytest.mark.parametrize("variant", ["z_one_hot", "g_one_hot"])
def test_single_products(variant, grl_option):
    """Every dW[k, c] is ONE product Z[r, k] g[r, c] of two bf16 values (all
    other terms add exact zeros), held to xi.BARE of the float64 product: two
    8-bit significands multiply exactly in fp32, so any misplaced fragment
    shows."""
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16z", 1)
    M, K, C = BWD_SHAPE
    assert M % 16 == 3 and 2 * M * K * C >= 1.6e10
    gen = torch.Generator(device=DEV).manual_seed(11)
    if variant == "z_one_hot":  # dW[k, c] = Z[r(k), k] g[r(k), c]
        g = _full16((M, C), gen)
        r = torch.from_numpy(_rows_over(K, M)).to(DEV)
        k = torch.arange(K, device=DEV)
        Z = torch.zeros(M, K, dtype=BF16, device=DEV)
        Z[r, k] = _full16((K,), gen)
        a, b = Z[r, k].float()[:, None], g[r].float()
    else:  # dW[k, c] = Z[r(c), k] g[r(c), c]
        Z = _full16((M, K), gen)
        r = torch.from_numpy(_rows_over(C, M)).to(DEV)
        c = torch.arange(C, device=DEV)
        g = torch.zeros(M, C, dtype=BF16, device=DEV)
        g[r, c] = _full16((C,), gen)
        a, b = Z[r].float().t(), g[r, c].float()[None, :]
    assert _query(Z, g) > 0
    dW, db = linear_bwd_weight_bf16z(Z, g, True)
    ref = (a.double() * b.double()).cpu().numpy()
    worst = xi.check_bound(dW.cpu().numpy(), ref, ref, xi.BARE, f"dW, {variant}")
    ref = g.double().sum(0)
    xi.check_bound(db.cpu().numpy(), ref.cpu().numpy(), g.double().abs().sum(0).cpu().numpy(), 1e-5, "db")
    # the MFMA kernel ran: with gemm_x6 = 0 the entry is not eligible at all
    grl_option("gemm_x6", 0)
    assert _query(Z, g) == 0 and linear_bwd_weight_bf16z(Z, g, False) is None
    grl_option("gemm_x6", 1)
    print(f"gemm_x1t dW {variant}: worst error {worst:.3f} x 2^-22 |a b|")


@pytest.mark.parametrize("case", ["z_off_the_8B_grid", "g_off_the_8B_grid", "ldz_not_a_multiple_of_4",
                                  "C_not_a_multiple_of_4", "M_below_the_floor", "dw_bf16z_0", "gemm_x6_0"])
def test_fallbacks_return_none(case, grl_option):
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16z", 1)
    M, K, C = SHAPES[0]
    Z, g, _ = _operands(M, K, C)
    if case == "z_off_the_8B_grid":
        Z = torch.empty(M * K + 1, dtype=BF16, device=DEV)[1:].view(M, K)
    elif case == "g_off_the_8B_grid":
        g = torch.empty(M * C + 1, dtype=BF16, device=DEV)[1:].view(M, C)
    elif case == "ldz_not_a_multiple_of_4":
        Z = torch.empty(M, K + 2, dtype=BF16, device=DEV)[:, :K]
    elif case == "C_not_a_multiple_of_4":
        g = torch.empty(M, C + 2, dtype=BF16, device=DEV)[:, :C - 2]
    elif case == "M_below_the_floor":
        Z, g = Z[:17_000], g[:17_000]
    elif case == "dw_bf16z_0":
        grl_option("dw_bf16z", 0)
    else:
        grl_option("gemm_x6", 0)
    assert _query(Z, g) == 0 and linear_bwd_weight_bf16z(Z, g, True) is None


def test_wrapper_refuses_what_the_entry_cannot_read_and_m_zero():
    Z, g, _ = _operands(*SHAPES[0])
    with pytest.raises(_lib.GrlError, match="bfloat16"):
        linear_bwd_weight_bf16z(Z.float(), g, True)
    with pytest.raises(_lib.GrlError, match="unit column stride"):
        linear_bwd_weight_bf16z(Z[:, ::2], g, True)
    with pytest.raises(_lib.GrlError, match="row stride"):
        linear_bwd_weight_bf16z(Z, g[:1].expand(g.shape[0], g.shape[1]), True)
    K, C = 64, 32
    dW = torch.full((K, C), 7.0, device=DEV)
    db = torch.full((C,), 7.0, device=DEV)
    _lib.call("grl_linear_bwd_weight_bf16zg", None, K, None, C, dW.data_ptr(), db.data_ptr(), 0, K, C, None, 0, None)
    torch.cuda.synchronize()
    assert not dW.any() and not db.any()  # M == 0 writes zeros
