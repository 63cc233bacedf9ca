"""CPU-only: the forward GEMM over a bf16 activation table
(grl_linear_fwd_bf16x and its workspace query): exported,
declared in include/grl.h and bound; the linear_bf16x path option; every
GRL_E_INVALID, GRL_E_UNSUPPORTED and GRL_E_WORKSPACE case decided on the host;
the eligibility rule read through the query -- grl_linear_fwd_ex's x6 path for
(M, path_rows, K, C) with C % 4 == 0 and a 16 B-aligned W, X 16 B-aligned with
ldx % 8 == 0, the option on -- whose nonzero answer is
grl_linear_fwd_ex_workspace_size.  No pointer is dereferenced and no device
work is issued.

And the numerical argument (x6.h at x3a_mfma) on the numpy model of the plane
products (x6_isolate): for an a that is one bf16 plane, the three products
(0,2), (0,1), (0,0) in that order give the bits of all six on the widened a."""
import os
import re

import numpy as np
import pytest

import x6_isolate as xi
from grl import _lib

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "grl.h")
FN, QUERY = "grl_linear_fwd_bf16x", "grl_linear_fwd_bf16x_workspace_query"

M, K, C = 20011, 1792, 256  # above the split-bf16 kernels' 1.6e10-flop floor
BELOW = 17438               # below it: 2 * 17438 * 1792 * 256 < 1.6e10
X, W, B, OUT, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000  # never dereferenced: every call fails a host check


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", src))


def query(x=X, ldx=None, w=W, m=M, k=K, c=C, pr=0):
    return getattr(_lib.lib(), QUERY)(x, k if ldx is None else ldx, w, m, k, c, pr)


def run(x=X, ldx=None, w=W, layout=1, b=B, out=OUT, m=M, k=K, c=C, relu=1, pr=0, ws=None, ws_bytes=0):
    rc = getattr(_lib.lib(), FN)(x, k if ldx is None else ldx, w, layout, b, out, m, k, c, relu, pr, ws, ws_bytes, None)
    return rc, _lib.lib().grl_last_error()


def size(m=M, k=K, c=C, pr=0):
    return _lib.lib().grl_linear_fwd_ex_workspace_size(m, k, c, pr)


@pytest.mark.parametrize("name", [FN, QUERY])
def test_symbols_are_exported_declared_and_bound(name):
    assert hasattr(_lib.lib(), name)
    assert name in declared_functions()
    assert name in _lib.SIGNATURES


def test_signatures():
    res, args = _lib.SIGNATURES[FN]
    tres, targs = _lib.SIGNATURES["grl_linear_fwd_ex"]
    assert res == tres and list(args) == list(targs)  # the fp32 entry's arguments, X in Z's place
    res, args = _lib.SIGNATURES[QUERY]
    assert res == _lib._c_size and len(args) == 7


def test_constants():
    assert 2 * M * K * C >= 1.6e10 > 2 * BELOW * K * C and K % 16 == 0 and C % 4 == 0


def test_the_option_round_trips_and_has_bounds(grl_option):
    default = _lib.get_option("linear_bf16x")
    assert default in (0, 1)
    for v in (0, 1):
        grl_option("linear_bf16x", v)
        assert _lib.get_option("linear_bf16x") == v
    for bad in (-1, 2):
        with pytest.raises(_lib.GrlError, match="outside"):
            _lib.set_option("linear_bf16x", bad)
    assert _lib.get_option("linear_bf16x") == 1  # a refused value changes nothing
    with _lib.options(linear_bf16x=0):
        assert _lib.get_option("linear_bf16x") == 0
    assert _lib.get_option("linear_bf16x") == 1


def test_argument_errors_are_refused_on_the_host(grl_option):
    grl_option("linear_bf16x", 1)
    grl_option("gemm_x6", 1)
    name = FN.encode()
    for kw in ({"m": -1}, {"k": -16, "ldx": 0}, {"c": -4}, {"pr": -1}):
        rc, msg = run(**kw)
        assert rc == _lib.GRL_E_INVALID and b"negative" in msg and name in msg, kw
    rc, msg = run(ldx=K - 8)
    assert rc == _lib.GRL_E_INVALID and b"ldx" in msg and name in msg
    for layout in (-1, 2):
        rc, msg = run(layout=layout)
        assert rc == _lib.GRL_E_INVALID and b"w_layout" in msg and name in msg
    for kw in ({"x": None}, {"w": None}, {"out": None}):
        rc, msg = run(**kw)
        assert rc == _lib.GRL_E_INVALID and b"NULL pointer" in msg and name in msg, kw
    rc, msg = run(x=X + 1)
    assert rc == _lib.GRL_E_INVALID and b"2-B aligned" in msg and name in msg
    # M == 0 or C == 0: nothing to do, whatever the pointers
    assert run(m=0, x=None, w=None, out=None)[0] == _lib.GRL_OK
    assert run(c=0, x=None, w=None, out=None)[0] == _lib.GRL_OK
    # ... but the sizes and w_layout are checked first
    assert run(m=0, ldx=K - 8)[0] == _lib.GRL_E_INVALID and run(c=0, layout=3)[0] == _lib.GRL_E_INVALID


# one broken condition each: K % 16, C % 4, ldx % 8, X on the 8 B grid but off the 16 B one, W off the 16 B grid,
# (M, path_rows) below the floor (twice: M itself, and a small M with a path_rows below it)
INELIGIBLE = ({"k": 1800}, {"k": 1796, "ldx": 1800}, {"c": 254}, {"ldx": K + 4}, {"x": X + 8}, {"w": W + 8},
              {"m": BELOW}, {"m": 100, "pr": BELOW})


def test_ineligible_calls_are_unsupported_and_eligible_ones_ask_for_the_workspace(grl_option):
    grl_option("linear_bf16x", 1)
    grl_option("gemm_x6", 1)
    name = FN.encode()
    need = size()
    assert query() == need > 0
    rc, msg = run()  # eligible: the next check is the workspace
    assert rc == _lib.GRL_E_WORKSPACE and name in msg
    rc, msg = run(ws=WS, ws_bytes=need - 1)
    assert rc == _lib.GRL_E_WORKSPACE and name in msg
    rc, msg = run(ws=None, ws_bytes=need)
    assert rc == _lib.GRL_E_WORKSPACE and name in msg
    for kw in INELIGIBLE:
        assert query(**kw) == 0, kw
        rc, msg = run(ws=WS, ws_bytes=1 << 40, **kw)
        assert rc == _lib.GRL_E_UNSUPPORTED and name in msg, kw
    grl_option("linear_bf16x", 0)
    assert query() == 0
    rc, msg = run(ws=WS, ws_bytes=need)
    assert rc == _lib.GRL_E_UNSUPPORTED and b"linear_bf16x" in msg and name in msg
    grl_option("linear_bf16x", 1)
    assert query() == need
    grl_option("gemm_x6", 0)  # the shape rule's own option
    assert query() == 0
    rc, msg = run(ws=WS, ws_bytes=need)
    assert rc == _lib.GRL_E_UNSUPPORTED and b"gemm_x6" in msg and name in msg


def test_the_query_is_the_fp32_entrys_workspace_size_where_eligible(grl_option):
    grl_option("linear_bf16x", 1)
    grl_option("gemm_x6", 1)
    lib = _lib.lib()
    for m, k, c, pr in ((M, K, C, 0), (1_000_000, 512, 128, 0), (1_000_000, 1792, 256, 0), (1, 32, 8, 1 << 30),
                        (300, 48, 40, 1 << 23), (5000, 512, 128, 1 << 23), (123_000, 512, 128, 0)):
        assert lib.grl_linear_fwd_path(m, k, c, pr) == 1
        assert query(m=m, k=k, c=c, pr=pr) == size(m, k, c, pr) == 3 * (-(-c // 256) * 256) * k * 2 + 256, (m, k, c, pr)
    # emb2's floor at net_size 256 (K = 512, C = 128): 122,071 nodes
    assert query(m=122_071, k=512, c=128) > 0 and query(m=122_070, k=512, c=128) == 0
    # a column slice of a wider table on the 16 B grid with the row stride on the 8-element grid
    assert query(x=X + 2 * 32, ldx=K + 64) == size()
    assert query(x=X + 16, ldx=K + 8) == size()


def test_the_query_is_zero_on_bad_arguments():
    assert query(x=None) == 0 and query(w=None) == 0
    assert query(m=0) == 0 and query(m=-1) == 0 and query(pr=-1) == 0
    assert query(k=0, ldx=0) == 0 and query(c=0) == 0
    assert query(ldx=K - 8) == 0


# ---- the numerical argument ----------------------------------------------------
THREE_A = ((0, 2), (0, 1), (0, 0))  # x3a_mfma's order: x6_mfma's without the products on a's zero planes


def test_three_products_are_the_six_on_a_one_plane_a_bitwise():
    """One accumulator fed T terms, as an output element is over its K16
    steps: a a bf16 value (some of them -0.0 and +0.0), b full-mantissa.  a's
    planes 1 and 2 are +0, their products +-0, and an accumulator that starts
    at +0 never holds -0, so dropping them changes no bit."""
    rng = np.random.default_rng(24)
    n, T = 1 << 14, 24
    a = xi.bf16_rne(rng.standard_normal((T, n)).astype(np.float32))
    b = xi.full_values(rng, (T, n))
    zero = rng.random((T, n)) < 0.2
    a[zero] = np.where(rng.random(zero.sum()) < 0.5, np.float32(-0.0), np.float32(0.0))
    a[:, :64] = np.float32(-0.0)  # whole chains of -0 terms: the accumulator must stay +0
    assert np.signbit(a[a == 0]).any() and not np.signbit(a[a == 0]).all()
    a0, a1, a2 = xi.split3(a)
    assert np.array_equal(a0.view(np.uint32), a.view(np.uint32))  # one plane: a's own bits (-0 kept)
    assert not a1.view(np.uint32).any() and not a2.view(np.uint32).any()  # the other two: +0
    acc6 = acc3 = None
    for t in range(T):
        acc6 = xi.six_product(a[t], b[t], xi.ORDER, acc6)
        acc3 = xi.six_product(a[t], b[t], THREE_A, acc3)
        assert np.array_equal(acc3.view(np.uint32), acc6.view(np.uint32)), t
    assert not acc3[:64].view(np.uint32).any()  # +0, not -0
    assert THREE_A == tuple(o for o in xi.ORDER if o[0] == 0)


def test_a_dropped_or_duplicated_product_breaks_the_single_product_bound():
    rng = np.random.default_rng(25)
    n = 1 << 14
    a = xi.bf16_rne(xi.full_values(rng, n))  # non-zero bf16 values
    b = xi.full_values(rng, n)
    # a single term is within the project's bound of the float64 product (b0 + b1 + b2 == b exactly)
    xi.check_products(xi.six_product(a, b, THREE_A), a, b, xi.BARE, "three products")
    for broken in (((0, 1), (0, 0)), ((0, 2), (0, 0)), ((0, 2), (0, 2), (0, 1), (0, 0)),
                   ((0, 2), (0, 1), (0, 1), (0, 0))):
        assert xi.violating_share(xi.six_product(a, b, broken), a, b) > 0.5, broken
