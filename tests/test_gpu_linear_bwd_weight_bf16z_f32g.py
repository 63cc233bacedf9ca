"""GPU: the weight gradient dW = Z^T g over a Z stored as bf16 and an fp32 g
(grl_linear_bwd_weight_bf16z; gemm_x3ta_kernel).

A bf16 Z is one plane of the split-bf16 scheme: the kernel stages it as loaded
and issues the three plane products a b2, a b1, a b0 where gemm_x6t_kernel
issues six, three of them on all-zero planes, over the same K16 steps, splits
and slab order.  So the checks are on BITS against grl_linear_bwd_weight on
Z.float(); the shapes are test_gpu_linear_bwd_weight_bf16.py's, the smallest
above the x6t floor 2 M K C >= 1.6e10 that reach the ragged last K16 step,
ragged row and column tiles with clamped loads, and the one-split store
epilogue.  Each case first asserts through the workspace query that the kernel
under test runs."""
import functools

import numpy as np
import pytest
import torch

import x6_isolate as xi
from grl import _lib
from grl.ops import linear_bwd_weight, linear_bwd_weight_bf16z_f32g

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SENTINEL = 0x5A5A  # a finite bf16 bit pattern

SHAPES = [
    (20_011, 1792, 256),  # M % 16 == 11: a ragged last K16 step; ~70 splits
    (60_001, 1400, 100),  # ragged dW row tiles, a ragged column tile with clamped loads
    (250, 8192, 4096),    # one split at 256 CUs: the store epilogue, no slab reduce; M % 16 == 10
]


def _i32(t):
    return t.contiguous().view(torch.int32)


def _bits16(t):
    return t.view(torch.int16)


def _query(Z, g):
    return _lib.lib().grl_linear_bwd_weight_bf16z_workspace_query(Z.data_ptr(), Z.stride(0), g.data_ptr(), Z.shape[0],
                                                                 Z.shape[1], g.shape[1])


@functools.lru_cache(maxsize=None)
def _operands(M, K, C):
    """Z = randn.to(bf16) with a sprinkling of exact +0 and -0, g = randn, and
    the fp32 entry's (dW, db) on the widened Z: made once, read-only."""
    gen = torch.Generator(device=DEV).manual_seed(M + K + C)
    Z = torch.randn(M, K, device=DEV, generator=gen).to(BF16)
    u = torch.rand(M, K, device=DEV, generator=gen)
    Z = torch.where(u < 0.05, torch.zeros((), dtype=BF16, device=DEV), Z)
    Z = torch.where((u >= 0.05) & (u < 0.10), -torch.zeros((), dtype=BF16, device=DEV), Z)
    del u
    assert bool((_bits16(Z) == -32768).any()) and bool((_bits16(Z) == 0).any())  # -0 and +0 are there
    g = torch.randn(M, C, device=DEV, generator=gen)
    ref = linear_bwd_weight(Z.float(), g, None, True)
    return Z, g, ref


@pytest.mark.parametrize("M,K,C", SHAPES)
def test_bits_are_the_fp32_entrys_on_the_widened_z(M, K, C, grl_option):
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16z_f32g", 1)
    assert 2 * M * K * C >= 1.6e10
    Z, g, (dW_ref, db_ref) = _operands(M, K, C)
    assert _query(Z, g) == _lib.lib().grl_linear_bwd_weight_workspace_size(M, K, C) > 0  # the kernel under test runs
    res = linear_bwd_weight_bf16z_f32g(Z, g, True)
    assert res is not None
    dW, db = res
    assert dW.shape == (K, C) and db.shape == (C,) and dW.dtype == db.dtype == torch.float32
    assert bool(torch.isfinite(dW).all()) and bool(dW.abs().sum() > 0)
    assert torch.equal(_i32(dW), _i32(dW_ref)), f"dW: {int((_i32(dW) != _i32(dW_ref)).sum())} elements differ"
    assert torch.equal(_i32(db), _i32(db_ref)), "db"
    dW2, db2 = linear_bwd_weight_bf16z_f32g(Z, g, True)  # two calls, equal bits
    assert torch.equal(_i32(dW2), _i32(dW)) and torch.equal(_i32(db2), _i32(db))
    dW3, none = linear_bwd_weight_bf16z_f32g(Z, g, False)  # db = NULL is accepted
    assert none is None and torch.equal(_i32(dW3), _i32(dW))


@pytest.mark.parametrize("M,K,C", SHAPES[:2])
def test_strided_z(M, K, C, grl_option):
    """Z a column slice of a wider sentinel-filled bf16 table (ldz = K + 64, 32
    columns in): the contiguous call's bits, and the table's other columns are
    untouched (Z is only read)."""
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16z_f32g", 1)
    Z, g, (dW_ref, db_ref) = _operands(M, K, C)
    table = torch.full((M, K + 64), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)
    table[:, 32:32 + K] = Z
    Zv = table[:, 32:32 + K]
    assert Zv.stride(0) == K + 64 and Zv.data_ptr() % 8 == 0 and not Zv.is_contiguous()
    assert _query(Zv, g) > 0
    dW, db = linear_bwd_weight_bf16z_f32g(Zv, g, True)
    assert torch.equal(_i32(dW), _i32(dW_ref)) and torch.equal(_i32(db), _i32(db_ref))
    assert bool((_bits16(table[:, :32]) == SENTINEL).all()) and bool((_bits16(table[:, 32 + K:]) == SENTINEL).all())
    assert torch.equal(_bits16(table[:, 32:32 + K]), _bits16(Z))


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


@pytest.mark.parametrize("variant", ["z_one_hot", "g_one_hot"])
def test_single_products(variant, grl_option):
    """Every dW[k, c] is ONE product Z[r, k] g[r, c] (all other terms add exact
    zeros), held to xi.BARE = 2^-22 of the float64 product: since b0 + b1 + b2
    == g and Z is one plane, the three products alone sit far inside it, and a
    dropped or misplaced a b2 or a b1 (2^-16, 2^-8 of the term) breaks it."""
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16z_f32g", 1)
    M, K, C = BWD_SHAPE
    assert M % 16 == 3 and 2 * M * K * C >= 1.6e10
    gen = torch.Generator(device=DEV).manual_seed(12)
    if variant == "z_one_hot":  # dW[k, c] = Z[r(k), k] g[r(k), c]: a one-hot bf16 Z, a full-mantissa fp32 g
        g = _full((M, C), gen)
        r = torch.from_numpy(_rows_over(K, M)).to(DEV)
        k = torch.arange(K, device=DEV)
        Z = torch.zeros(M, K, dtype=BF16, device=DEV)
        Z[r, k] = _full16((K,), gen)
        a, b = Z[r, k].float()[:, None], g[r]
    else:  # dW[k, c] = Z[r(c), k] g[r(c), c]: a full-range bf16 Z, a one-hot fp32 g
        Z = _full16((M, K), gen)
        r = torch.from_numpy(_rows_over(C, M)).to(DEV)
        c = torch.arange(C, device=DEV)
        g = torch.zeros(M, C, device=DEV)
        g[r, c] = _full((C,), gen)
        a, b = Z[r].float().t(), g[r, c][None, :]
    assert _query(Z, g) > 0
    dW, db = linear_bwd_weight_bf16z_f32g(Z, g, True)
    ref = (a.double() * b.double()).cpu().numpy()
    worst = xi.check_bound(dW.cpu().numpy(), ref, ref, xi.BARE, f"dW, {variant}")
    ref = g.double().sum(0)  # the fp32 column sum, as test_gpu_x6_planes.py holds it: 1e-5 of sum |terms|
    xi.check_bound(db.cpu().numpy(), ref.cpu().numpy(), g.double().abs().sum(0).cpu().numpy(), 1e-5, "db")
    # the MFMA kernel ran: the fp32 GEMM (gemm_x6 = 0), whose single products are correctly rounded, gives other bits
    grl_option("gemm_x6", 0)
    assert _query(Z, g) == 0
    other = linear_bwd_weight(Z.float(), g, None, False)[0]
    grl_option("gemm_x6", 1)
    assert not torch.equal(other, dW), "the fp32 GEMM's bits -- gemm_x3ta_kernel did not run"
    print(f"gemm_x3ta dW {variant}: worst error {worst:.3f} x 2^-22 |a b|")


# ---- fallbacks, refusals, M == 0 -------------------------------------------------
@pytest.mark.parametrize("case", ["z_off_the_8B_grid", "C_not_a_multiple_of_4", "M_below_the_floor",
                                  "dw_bf16z_f32g_0", "gemm_x6_0"])
def test_fallbacks_return_none(case, grl_option):
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16z_f32g", 1)
    M, K, C = SHAPES[0]
    Z, g, _ = _operands(M, K, C)
    if case == "z_off_the_8B_grid":
        wide = torch.zeros(M, K + 8, dtype=BF16, device=DEV)
        wide[:, 1:1 + K] = Z
        Z = wide[:, 1:1 + K]
        assert Z.data_ptr() % 8 == 2
    elif case == "C_not_a_multiple_of_4":
        g = g[:, :C - 2].contiguous()
    elif case == "M_below_the_floor":
        Z, g = Z[:17_000], g[:17_000]
        assert 2 * 17_000 * K * C < 1.6e10
    elif case == "dw_bf16z_f32g_0":
        grl_option("dw_bf16z_f32g", 0)
    else:
        grl_option("gemm_x6", 0)
    assert _query(Z, g) == 0
    assert linear_bwd_weight_bf16z_f32g(Z, g, True) is None


def test_wrapper_refuses_what_the_entry_cannot_read():
    M, K, C = 64, 32, 16
    Z = torch.zeros(M, K, dtype=BF16, device=DEV)
    g = torch.zeros(M, C, device=DEV)
    assert linear_bwd_weight_bf16z_f32g(Z, g, True) is None  # well-formed, far below the floor
    for bad in (Z.float(), Z[0], Z.t().contiguous().t(), Z[:1].expand(M, K)):
        with pytest.raises(_lib.GrlError, match="linear_bwd_weight_bf16z_f32g: X must be"):
            linear_bwd_weight_bf16z_f32g(bad, g, True)
    for bad in (g.to(BF16), g[:M - 1], g.t().contiguous().t(), g[0], torch.zeros(M, C + 8, device=DEV)[:, :C]):
        with pytest.raises(_lib.GrlError, match="linear_bwd_weight_bf16z_f32g: g must be"):
            linear_bwd_weight_bf16z_f32g(Z, bad, True)


def test_empty_operands():
    """M == 0: dW = 0 and db = 0 (an empty node-range shard); db = NULL accepted."""
    K, C = 64, 32
    lib = _lib.lib()
    from grl.graph import current_stream_handle
    dW = torch.full((K, C), 7.0, device=DEV)
    db = torch.full((C,), 7.0, device=DEV)
    st = current_stream_handle(DEV)
    assert lib.grl_linear_bwd_weight_bf16z(None, K, None, dW.data_ptr(), db.data_ptr(), 0, K, C, None, 0,
                                           st) == _lib.GRL_OK
    torch.cuda.synchronize()
    assert not bool(dW.any()) and not bool(db.any())
    dW.fill_(7.0)
    assert lib.grl_linear_bwd_weight_bf16z(None, K, None, dW.data_ptr(), None, 0, K, C, None, 0, st) == _lib.GRL_OK
    torch.cuda.synchronize()
    assert not bool(dW.any())
