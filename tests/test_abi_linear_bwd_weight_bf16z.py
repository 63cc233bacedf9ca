"""CPU-only: the weight gradient over a bf16 Z and a bf16 output gradient
(grl_linear_bwd_weight_bf16zg and its workspace query): exported, declared in
include/grl.h and bound; the dw_bf16z path option; every GRL_E_INVALID,
GRL_E_UNSUPPORTED and GRL_E_WORKSPACE case decided on the host; the
eligibility rule read through the query -- grl_linear_bwd_weight's split-bf16
shape rule, Z and g 8 B-aligned (ldz % 4 == 0, ldg % 4 == 0) and the option on
-- whose nonzero answer is grl_linear_bwd_weight_workspace_size.  No pointer is
dereferenced and no device work is issued.

And the numerical argument of DESIGN.md §4.21 on the numpy model of the plane
products (x6_isolate): for an a and a b that are one bf16 plane each, the
single product (0,0) gives the bits of the three (2,0), (1,0), (0,0) and of all
six."""
import os
import re

import numpy as np
import pytest

import x6_isolate as xi
from grl import _lib

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "grl.h")
FN, QUERY = "grl_linear_bwd_weight_bf16zg", "grl_linear_bwd_weight_bf16zg_workspace_query"

M, K, C = 20011, 1792, 256  # above the split-bf16 kernels' 1.6e10-flop floor
BELOW = 17438               # below it: 2 * 17438 * 1792 * 256 < 1.6e10
Z, G, DW, DB, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000  # never dereferenced: every call fails a host check


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", src))


def query(z=Z, ldz=K, g=G, ldg=C, m=M, k=K, c=C):
    return getattr(_lib.lib(), QUERY)(z, ldz, g, ldg, m, k, c)


def run(z=Z, ldz=K, g=G, ldg=C, dw=DW, db=None, m=M, k=K, c=C, ws=None, ws_bytes=0):
    rc = getattr(_lib.lib(), FN)(z, ldz, g, ldg, dw, db, m, k, c, ws, ws_bytes, None)
    return rc, _lib.lib().grl_last_error()


def size(m=M, k=K, c=C):
    return _lib.lib().grl_linear_bwd_weight_workspace_size(m, k, c)


@pytest.mark.parametrize("name", [FN, QUERY])
def test_symbols_are_exported_declared_and_bound(name):
    assert hasattr(_lib.lib(), name)
    assert name in declared_functions()
    assert name in _lib.SIGNATURES


def test_signatures_are_the_bf16g_entrys():
    # Z a pointer either way: the same argument lists
    assert _lib.SIGNATURES[FN] == _lib.SIGNATURES["grl_linear_bwd_weight_bf16g"]
    assert _lib.SIGNATURES[QUERY] == _lib.SIGNATURES["grl_linear_bwd_weight_bf16g_workspace_query"]


def test_constants():
    assert 2 * M * K * C >= 1.6e10 > 2 * BELOW * K * C and M >= 16 and K % 4 == 0 and C % 4 == 0


def test_the_option_round_trips_and_has_bounds(grl_option):
    assert _lib.get_option("dw_bf16z") in (0, 1)
    for v in (0, 1):
        grl_option("dw_bf16z", v)
        assert _lib.get_option("dw_bf16z") == v
    for bad in (-1, 2):
        with pytest.raises(_lib.GrlError, match="outside"):
            _lib.set_option("dw_bf16z", bad)
    assert _lib.get_option("dw_bf16z") == 1  # a refused value changes nothing


def test_argument_errors_are_refused_on_the_host(grl_option):
    grl_option("dw_bf16z", 1)
    grl_option("gemm_x6", 1)
    name = FN.encode()
    for kw in ({"m": -1}, {"k": -4}, {"c": -4}):
        rc, msg = run(**kw)
        assert rc == _lib.GRL_E_INVALID and b"negative" in msg and name in msg, kw
    rc, msg = run(ldz=K - 4)
    assert rc == _lib.GRL_E_INVALID and b"ldz" in msg and name in msg
    rc, msg = run(ldg=C - 4)
    assert rc == _lib.GRL_E_INVALID and b"ldg" in msg and name in msg
    for kw in ({"z": None}, {"g": None}, {"dw": None}):
        rc, msg = run(**kw)
        assert rc == _lib.GRL_E_INVALID and b"NULL pointer" in msg and name in msg, kw
    for kw in ({"g": G + 1}, {"z": Z + 1}):  # an odd address
        rc, msg = run(**kw)
        assert rc == _lib.GRL_E_INVALID and b"2-B aligned" in msg and name in msg, kw
    rc, msg = run(m=0, dw=None)  # M == 0 writes dW = 0: it needs a dW
    assert rc == _lib.GRL_E_INVALID and b"NULL pointer" in msg
    # K == 0 or C == 0: nothing to do, whatever the pointers
    assert run(k=0, ldz=0, z=None, g=None, dw=None)[0] == _lib.GRL_OK
    assert run(c=0, ldg=0, z=None, g=None, dw=None)[0] == _lib.GRL_OK


def test_ineligible_calls_are_unsupported_and_eligible_ones_ask_for_the_workspace(grl_option):
    grl_option("dw_bf16z", 1)
    grl_option("gemm_x6", 1)
    name = FN.encode()
    need = size()
    assert query() == need > 0
    rc, msg = run()  # eligible: the next check is the workspace
    assert rc == _lib.GRL_E_WORKSPACE and name in msg
    rc, msg = run(ws=WS, ws_bytes=need - 1)
    assert rc == _lib.GRL_E_WORKSPACE and name in msg
    rc, _ = run(ws=None, ws_bytes=need)
    assert rc == _lib.GRL_E_WORKSPACE
    # one broken condition each: the flop floor, M >= 16 (above the floor), K % 4, C % 4, Z's 8 B (twice), ldz % 4,
    # g's 8 B (twice), ldg % 4
    for kw in ({"m": BELOW}, {"m": 12, "k": 32768, "c": 32768, "ldz": 32768, "ldg": 32768},
               {"k": K + 2, "ldz": K + 4}, {"c": C - 2}, {"z": Z + 4}, {"z": Z + 2}, {"ldz": K + 2}, {"g": G + 4},
               {"g": G + 2}, {"ldg": C + 2}):
        assert query(**kw) == 0, kw
        rc, msg = run(**kw)
        assert rc == _lib.GRL_E_UNSUPPORTED and name in msg, kw
    grl_option("dw_bf16z", 0)
    assert query() == 0
    rc, msg = run()
    assert rc == _lib.GRL_E_UNSUPPORTED and b"dw_bf16z" in msg
    grl_option("dw_bf16z", 1)
    assert query() == need
    grl_option("gemm_x6", 0)  # the shape rule's own option
    assert query() == 0
    rc, msg = run()
    assert rc == _lib.GRL_E_UNSUPPORTED and b"gemm_x6" in msg


def test_the_query_is_the_fp32_entrys_workspace_size_where_eligible(grl_option):
    grl_option("dw_bf16z", 1)
    grl_option("gemm_x6", 1)
    for m, k, c in ((M, K, C), (60001, 1400, 100), (250, 8192, 4096), (1_000_000, 1792, 256), (16, 32768, 16384)):
        assert 2 * m * k * c >= 1.6e10
        assert query(m=m, k=k, c=c, ldz=k, ldg=c) == size(m, k, c) > 0, (m, k, c)
    # strided operands: column slices of wider tables on the 8 B grid
    assert query(g=G + 2 * 32, ldg=C + 64) == size()
    assert query(g=G + 8, ldg=C + 4) == size()
    assert query(z=Z + 8, ldz=K + 24) == size()


def test_the_query_is_zero_on_bad_arguments():
    assert query(z=None) == 0 and query(g=None) == 0
    assert query(m=0) == 0 and query(m=-1) == 0
    assert query(k=0, ldz=0) == 0 and query(c=0, ldg=0) == 0
    assert query(ldz=K - 4) == 0 and query(ldg=C - 4) == 0


# ---- the numerical argument ----------------------------------------------------
ONE = ((0, 0),)                   # x1_mfma
THREE = ((2, 0), (1, 0), (0, 0))  # x3_mfma's order


def test_one_product_is_the_three_and_the_six_on_one_plane_operands_bitwise():
    """One accumulator fed T terms, as a dW element is over its K16 steps: a
    and b bf16 values (some of them -0.0 and +0.0, whole chains of -0).  a's and
    b's planes 1 and 2 are +0, their products +-0, and an accumulator that
    starts at +0 never holds -0, so dropping them changes no bit."""
    rng = np.random.default_rng(21)
    n, T = 1 << 14, 24
    a = xi.bf16_rne(xi.full_values(rng, (T, n)))
    b = xi.bf16_rne(rng.standard_normal((T, n)).astype(np.float32))
    for v in (a, b):
        zero = rng.random((T, n)) < 0.2
        v[zero] = np.where(rng.random(zero.sum()) < 0.5, np.float32(-0.0), np.float32(0.0))
    a[:, :64] = np.float32(-0.0)    # whole chains of -0 terms: the accumulator must stay +0
    b[:, 32:96] = np.float32(-0.0)  # ... on either side, and (-0)(-0) = +0 where both are
    for v in (a, b):
        assert np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
        v0, v1, v2 = xi.split3(v)
        assert np.array_equal(v0.view(np.uint32), v.view(np.uint32))  # one plane: the value's own bits (-0 kept)
        assert not v1.view(np.uint32).any() and not v2.view(np.uint32).any()  # the other two: +0
    acc6 = acc3 = acc1 = None
    for t in range(T):
        acc6 = xi.six_product(a[t], b[t], xi.ORDER, acc6)
        acc3 = xi.six_product(a[t], b[t], THREE, acc3)
        acc1 = xi.six_product(a[t], b[t], ONE, acc1)
        assert np.array_equal(acc1.view(np.uint32), acc3.view(np.uint32)), t
        assert np.array_equal(acc1.view(np.uint32), acc6.view(np.uint32)), t
    assert not acc1[:96].view(np.uint32).any()  # +0, not -0
    assert ONE == tuple(o for o in xi.ORDER if o == (0, 0))
    # a single term is the float64 product of the two bf16 values: 8-bit significands multiply exactly in fp32
    xi.check_products(xi.six_product(a[0], b[0], ONE), a[0], b[0], xi.BARE, "one product")
