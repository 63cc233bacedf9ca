"""CPU-only: the rule that sends a GraphConv forward to the one-kernel path,
read through the two workspace queries (grl_graphconv_fwd_workspace_query and
grl_graphconv_fwd_bf16_workspace_query).  Both are host arithmetic on the
graph's header fields and the addresses' alignment; no pointer is dereferenced.

One rule serves both table types.  It differs by the element size alone: X is
aligned to a lane's 4 columns (16 B of fp32, 8 B of bf16) and a row's bytes
fit 32 bits (ldx < 2^30 floats, < 2^31 bf16).  The expected answers are those
of the two separate rules this one replaced."""
import ctypes

import pytest

from grl import _lib

ROWS, TYPES, F, C = 20011, 6, 256, 256  # 2 * 20011 * 1792 * 256 flops: above the x6 GEMM's 1.6e10 floor
ONE = 7 * 256 * 1536 + 256              # W's planes ((1 + 6) * F rows, 8 blocks of 32 columns x 3 planes x 2 B) + the status
TWO = ROWS * 7 * 256 * 4                # at least Z whole
QUERIES = {"fp32": "grl_graphconv_fwd_workspace_query", "bf16": "grl_graphconv_fwd_bf16_workspace_query"}

# ldx -> the answers for X = 0x1000, 0x1008, 0x1004, 0x1002
X_ADDRS = (0x1000, 0x1008, 0x1004, 0x1002)
TABLE = {
    "fp32": {256: "one two two two", 258: "two two two two", 260: "one two two two", 2**30: "two two two two",
             2**31 - 4: "two two two two", 2**31: "two two two two"},
    "bf16": {256: "one one two two", 258: "two two two two", 260: "one one two two", 2**30: "one one two two",
             2**31 - 4: "one one two two", 2**31: "two two two two"},
}
CASES = [(t, ldx, x, want) for t, rows in TABLE.items() for ldx, wants in rows.items()
         for x, want in zip(X_ADDRS, wants.split())]


def query(table, ldx=256, X=0x1000, W=0x2000, c=C):
    g = _lib.GrlTypedCsr()
    g.num_rows, g.num_types, g.has_self = ROWS, TYPES, 1
    return getattr(_lib.lib(), QUERIES[table])(ctypes.byref(g), X, ldx, F, W, c)


def check(got, want):
    if want == "one":
        assert got == ONE
    else:
        assert got >= TWO


def test_constants():
    assert ONE == 2752768 and TWO == ROWS * 7 * 256 * 4 and 2 * ROWS * 7 * F * C > 1.6e10


@pytest.mark.parametrize("table,ldx,X,want", CASES, ids=[f"{t}-ldx{ldx}-X{x:#x}" for t, ldx, x, _ in CASES])
def test_row_stride_and_table_alignment(table, ldx, X, want):
    check(query(table, ldx=ldx, X=X), want)


@pytest.mark.parametrize("table", ["fp32", "bf16"])
def test_unaligned_w_and_odd_c_take_the_chain(table):
    check(query(table), "one")
    check(query(table, W=0x2008), "two")
    check(query(table, c=254), "two")
