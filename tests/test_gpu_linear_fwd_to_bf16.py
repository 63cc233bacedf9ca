"""GPU: the x6 forward GEMM storing bf16 rows (grl_linear_fwd_to_bf16;
gemm_x6_kernel's EPI_BF16 epilogue).

The main loop is gemm_x6_kernel's own; the epilogue applies bias and ReLU as
EPI_BIAS does, lane pairs trade one value of each register pair and every lane
stores one dword of two adjacent columns, each value rounded once to nearest
even.  So the checks are on BITS against grl_linear_fwd_ex(...) followed by
.to(torch.bfloat16) with the same path_rows.  path_rows puts the small M on the
x6 path, so the shapes are test_gpu_linear_fwd_bf16x.py's: a ragged second row
tile with an odd last row pair, the whole-tile epilogue, one row (every odd
lane's row out of range) and a 4-column last tile.  Each case first asserts
that the kernel under test runs."""
import functools

import pytest
import torch

from grl import _lib
from grl.ops import linear_fwd_ex, linear_fwd_to_bf16

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SENTINEL = 0x5A5A  # a finite bf16 bit pattern (no rounded randn product carries it: 1.5e16)
PR = 1 << 23

# (M, K, C, path_rows)
SHAPES = [
    (300, 48, 40, PR),    # a ragged second row tile, rows 256..299; a ragged column tile
    (256, 16, 256, PR),   # the whole-row-tile epilogue, nk == 1
    (1, 32, 8, 1 << 25),  # one row: every odd lane's row is out of range (2 R K C >= 1.6e10 needs R >= 2^25 here)
    (513, 64, 260, PR),   # three row tiles, the last of one row; two column tiles, the second 4 columns wide
]


def _bits16(t):
    return t.view(torch.int16)


def _query(X, W, C, out, pr):
    M, K = X.shape
    return _lib.lib().grl_linear_fwd_to_bf16_workspace_query(X.data_ptr(), max(X.stride(0), K), W.data_ptr(),
                                                             out.data_ptr(), max(out.stride(0), C), M, K, C, pr)


def _assert_runs(X, W, C, out, pr):
    """The x6 path for these sizes, and the entry under test eligible."""
    M, K = X.shape
    lib = _lib.lib()
    assert lib.grl_linear_fwd_path(M, K, C, pr) == 1
    assert _query(X, W, C, out, pr) == lib.grl_linear_fwd_ex_workspace_size(M, K, C, pr) > 0


@functools.lru_cache(maxsize=None)
def _operands(M, K, C):
    """X, W [K, C], W^T [C, K] and the bias: made once, read-only."""
    gen = torch.Generator(device=DEV).manual_seed(M + K + C)
    X = torch.randn(M, K, device=DEV, generator=gen)
    W = torch.randn(K, C, device=DEV, generator=gen) / K ** 0.5
    b = torch.randn(C, device=DEV, generator=gen)
    return X, W, W.t().contiguous(), b


def _sentinel(M, C):
    return torch.full((M, C), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)


def _check(got, want):
    assert got.dtype == BF16 and got.shape == want.shape
    assert not bool((_bits16(got) == SENTINEL).any()), "an element was not written"
    diff = int((_bits16(got) != _bits16(want)).sum())
    assert diff == 0, f"{diff} of {got.numel()} differ"


@pytest.mark.parametrize("epi", ["store", "bias_relu"])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("M,K,C,pr", SHAPES)
def test_bits_are_the_fp32_entrys_rounded_once(M, K, C, pr, layout, epi, grl_option):
    grl_option("gemm_x6", 1)
    grl_option("linear_out_bf16", 1)
    X, W0, W1, b = _operands(M, K, C)
    W = W1 if layout else W0
    bias, relu = (b, True) if epi == "bias_relu" else (None, False)
    out = _sentinel(M, C)
    _assert_runs(X, W, C, out, pr)
    want = linear_fwd_ex(X, W, layout, bias, relu, pr).to(BF16)
    got = linear_fwd_to_bf16(X, W, layout, bias, relu, pr, out=out)
    assert got is out
    torch.cuda.synchronize()
    _check(got, want)
    assert bool(got.float().abs().sum() > 0)
    if relu:
        assert not bool((got < 0).any()) and (M * C < 1024 or bool((got == 0).any()))
    fresh = linear_fwd_to_bf16(X, W, layout, bias, relu, pr)  # an out of its own; two calls, equal bits
    assert fresh is not None and fresh.is_contiguous() and torch.equal(_bits16(fresh), _bits16(got))


@pytest.mark.parametrize("M,K,C,pr", SHAPES)
def test_out_is_a_column_slice_of_a_wider_table(M, K, C, pr, grl_option):
    """out 32 columns into a sentinel-filled bf16 table C + 64 wide: every
    element of the slice written, the neighbours untouched."""
    grl_option("gemm_x6", 1)
    grl_option("linear_out_bf16", 1)
    X, W0, _, b = _operands(M, K, C)
    table = _sentinel(M, C + 64)
    out = table[:, 32:32 + C]
    assert out.data_ptr() % 4 == 0 and (M == 1 or (out.stride(0) == C + 64 and not out.is_contiguous()))
    _assert_runs(X, W0, C, out, pr)
    want = linear_fwd_ex(X, W0, 0, b, True, pr).to(BF16)
    assert linear_fwd_to_bf16(X, W0, 0, b, True, pr, out=out) is out
    torch.cuda.synchronize()
    _check(table[:, 32:32 + C], want)
    assert bool((_bits16(table[:, :32]) == SENTINEL).all()) and bool((_bits16(table[:, 32 + C:]) == SENTINEL).all())


@pytest.mark.parametrize("M", [255, 257, 301])
def test_an_odd_row_count(M, grl_option):
    """M odd inside a whole column tile (C = 256): the last row is an even
    lane's row whose odd partner's row is out of range -- in the first row
    tile, as the only row of the second, and as the last of a ragged second."""
    grl_option("gemm_x6", 1)
    grl_option("linear_out_bf16", 1)
    K, C, pr = 32, 256, PR
    X, W0, W1, b = _operands(M, K, C)
    guard = _sentinel(M + 2, C)  # two sentinel rows behind the last: a store past the row bound shows
    out = guard[:M]
    _assert_runs(X, W1, C, out, pr)
    want = linear_fwd_ex(X, W1, 1, b, False, pr).to(BF16)
    linear_fwd_to_bf16(X, W1, 1, b, False, pr, out=out)
    torch.cuda.synchronize()
    _check(out, want)
    assert bool((_bits16(guard[M:]) == SENTINEL).all())


@pytest.mark.parametrize("case", ["linear_out_bf16_0", "gemm_x6_0", "odd_ldo", "out_off_the_dword_grid"])
def test_fallbacks_return_none(case, grl_option):
    grl_option("gemm_x6", 1)
    grl_option("linear_out_bf16", 1)
    M, K, C, pr = SHAPES[0]
    X, W0, _, b = _operands(M, K, C)
    out = _sentinel(M, C)
    if case == "linear_out_bf16_0":
        grl_option("linear_out_bf16", 0)
    elif case == "gemm_x6_0":
        grl_option("gemm_x6", 0)
    elif case == "odd_ldo":
        out = _sentinel(M, C + 1)[:, :C]
        assert out.stride(0) % 2 == 1
    else:
        out = _sentinel(M, C + 2)[:, 1:1 + C]
        assert out.data_ptr() % 4 == 2 and out.stride(0) % 2 == 0
    keep = out.clone()
    assert _query(X, W0, C, out, pr) == 0
    assert linear_fwd_to_bf16(X, W0, 0, b, True, pr, out=out) is None
    torch.cuda.synchronize()
    assert torch.equal(_bits16(out), _bits16(keep))  # nothing was written
    if case in ("linear_out_bf16_0", "gemm_x6_0"):
        assert linear_fwd_to_bf16(X, W0, 0, b, True, pr) is None
    # grl_linear_fwd_ex answers as before: the caller's route
    assert linear_fwd_ex(X, W0, 0, b, True, pr).to(BF16).shape == (M, C)


def test_wrapper_refuses_what_the_entry_cannot_take():
    M, K, C = 64, 32, 16
    X = torch.zeros(M, K, device=DEV)
    W = torch.zeros(K, C, device=DEV)
    assert linear_fwd_to_bf16(X, W, 0, None, False) is None  # well-formed, far below the floor
    for bad in (X.to(BF16), X[0], X.t().contiguous().t()):
        with pytest.raises(_lib.GrlError, match="linear_fwd_to_bf16: X must be"):
            linear_fwd_to_bf16(bad, W, 0, None, False)
    for bad in (W.to(BF16), W[:, :8], W[:K - 1]):
        with pytest.raises(_lib.GrlError, match="linear_fwd_to_bf16: W must be"):
            linear_fwd_to_bf16(X, bad, 0, None, False)
    for bad in (torch.zeros(M, C, device=DEV), torch.zeros(M, C + 2, dtype=BF16, device=DEV),
                torch.zeros(C, M, dtype=BF16, device=DEV).t()):
        with pytest.raises(_lib.GrlError, match="linear_fwd_to_bf16: out must be"):
            linear_fwd_to_bf16(X, W, 0, None, False, out=bad)
