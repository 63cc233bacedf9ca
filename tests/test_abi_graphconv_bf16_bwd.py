"""CPU-only: the bf16 data gradient of the one-kernel GraphConv layer
(grl_graphconv_bwd_data_bf16 and its workspace query) and the one-pass bf16
ReLU mask (grl_relu_grad_bf16): exported, declared in include/grl.h and
bound; the data gradient's own argument errors (NULL dX, lddx < F, ldg < C, an
odd address for a 2-byte type) are GRL_E_INVALID decided on the host; a shape
below the x6 floor is GRL_E_UNSUPPORTED; and the path rule read through the
workspace query -- the fp32 entry's rule with G 8 B-aligned (ldg % 4 == 0), dX
4 B-aligned (lddx even) and the graphconv_bwd_bf16 path option on.  No
pointer is dereferenced and no device work is issued."""
import ctypes
import os
import re

import pytest

from grl import _lib

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "grl.h")
BWD, QUERY, RELU = "grl_graphconv_bwd_data_bf16", "grl_graphconv_bwd_data_bf16_workspace_query", "grl_relu_grad_bf16"

ROWS, TYPES, C, F = 20011, 6, 256, 256  # above the x6 GEMM's 1.6e10-flop floor (test_abi_graphconv_path_rule.py)
BELOW = 17438                           # below it: 2 * 17438 * 7 * 256 * 256 < 1.6e10
ONE = 7 * 256 * 1536 + 256              # W's planes + the status word: the one-kernel answer


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", src))


def graph(num_rows=ROWS, num_types=TYPES, has_self=1):
    g = _lib.GrlTypedCsr()
    g.num_rows, g.num_types, g.has_self = num_rows, num_types, has_self
    g.rowptr = 0x3000  # non-NULL, never dereferenced: every call below fails a host check first
    return g


def bwd(g, G=0x1000, ldg=C, dX=0x4000, lddx=F, g_rows=0, G_agg=None, ws=None, ws_bytes=0):
    rc = getattr(_lib.lib(), BWD)(ctypes.byref(g), None, G, ldg, g_rows, C, 0x2000, F, dX, lddx, G_agg, None, ws,
                                  ws_bytes, None)
    return rc, _lib.lib().grl_last_error()


def query(g=None, G=0x1000, ldg=C, W=0x2000, dX=0x4000, lddx=F, c=C, f=F):
    g = graph() if g is None else g
    return getattr(_lib.lib(), QUERY)(ctypes.byref(g), G, ldg, c, W, f, dX, lddx)


def fp32_query(g=None, G=0x1000, ldg=C, W=0x2000, c=C, f=F):
    g = graph() if g is None else g
    return _lib.lib().grl_graphconv_bwd_data_workspace_query(ctypes.byref(g), G, ldg, c, W, f)


@pytest.mark.parametrize("name", [BWD, QUERY, RELU])
def test_symbols_are_exported_declared_and_bound(name):
    assert hasattr(_lib.lib(), name)
    assert name in declared_functions()
    assert name in _lib.SIGNATURES


def test_signatures_are_the_fp32_entries_with_the_strides():
    res, args = _lib.SIGNATURES[BWD]
    tres, targs = _lib.SIGNATURES["grl_graphconv_bwd_data"]
    assert res == tres  # the fp32 entry's arguments with lddx after dX
    assert list(args[:9]) + list(args[10:]) == list(targs) and args[9] == _lib._c_i64
    res, args = _lib.SIGNATURES[QUERY]
    tres, targs = _lib.SIGNATURES["grl_graphconv_bwd_data_workspace_query"]
    assert res == tres and list(args) == list(targs) + [_lib._c_vp, _lib._c_i64]
    res, args = _lib.SIGNATURES[RELU]
    assert res == _lib._c_i32 and len(args) == 13


def test_constants():
    assert ONE == 2752768 and 2 * ROWS * 7 * C * F > 1.6e10 > 2 * BELOW * 7 * C * F


def test_own_argument_errors_are_refused_on_the_host():
    name = BWD.encode()
    rc, msg = bwd(graph(), dX=None)
    assert rc == _lib.GRL_E_INVALID and b"NULL pointer" in msg and name in msg
    rc, msg = bwd(graph(), lddx=F - 2)
    assert rc == _lib.GRL_E_INVALID and b"lddx" in msg and name in msg
    rc, msg = bwd(graph(num_rows=0), lddx=F - 2)  # refused before the empty graph's early return
    assert rc == _lib.GRL_E_INVALID and b"lddx" in msg
    rc, msg = bwd(graph(), ldg=C - 4)
    assert rc == _lib.GRL_E_INVALID and b"ldg" in msg and name in msg
    rc, msg = bwd(graph(), dX=0x4001)
    assert rc == _lib.GRL_E_INVALID and b"2-B aligned" in msg and name in msg
    rc, msg = bwd(graph(), G=0x1001)
    assert rc == _lib.GRL_E_INVALID and b"2-B aligned" in msg and name in msg
    rc, _ = bwd(graph(num_rows=0))  # no rows: nothing to do
    assert rc == _lib.GRL_OK


def test_the_fp32_entrys_checks_still_apply():
    lib = _lib.lib()
    rc = getattr(lib, BWD)(None, None, 0x1000, C, 0, C, 0x2000, F, 0x4000, F, None, None, None, 0, None)
    assert rc == _lib.GRL_E_INVALID and b"NULL" in lib.grl_last_error()
    rc, msg = bwd(graph(num_types=0))
    assert rc == _lib.GRL_E_INVALID and b"num_types" in msg
    rc, msg = bwd(graph(), g_rows=ROWS + 1)
    assert rc == _lib.GRL_E_INVALID and b"g_rows" in msg
    rc, msg = bwd(graph(), G=None, g_rows=1)  # a NULL G is an empty shard's only
    assert rc == _lib.GRL_E_INVALID and b"NULL pointer" in msg


def test_below_the_x6_floor_is_unsupported_and_above_it_asks_for_the_workspace():
    assert query(graph(num_rows=BELOW)) == 0 and fp32_query(graph(num_rows=BELOW)) == 0
    rc, msg = bwd(graph(num_rows=BELOW))
    assert rc == _lib.GRL_E_UNSUPPORTED and BWD.encode() in msg
    assert query() == ONE
    rc, msg = bwd(graph())  # eligible: the next check is the workspace
    assert rc == _lib.GRL_E_WORKSPACE and BWD.encode() in msg
    rc, _ = bwd(graph(), ws=0x8008, ws_bytes=ONE)  # not 16 B-aligned
    assert rc == _lib.GRL_E_WORKSPACE
    rc, _ = bwd(graph(), ws=0x8000, ws_bytes=ONE - 1)
    assert rc == _lib.GRL_E_WORKSPACE


def test_the_query_is_the_fp32_querys_value_where_the_rows_take_the_loads_and_stores(grl_option):
    assert query() == ONE == fp32_query()
    assert query(lddx=F + 128, dX=0x4000 + 2 * 64) == ONE   # a column slice of a wider table
    assert query(ldg=2 * C, G=0x1000 + 2 * C) == ONE        # G a column slice, too
    assert query(dX=0x4004, lddx=F + 2) == ONE
    assert query(G=0x1008, ldg=C + 4) == ONE
    assert query(dX=0x4002) == 0        # dX % 4 == 2: no dword stores
    assert query(lddx=F + 1) == 0       # an odd row stride
    assert query(G=0x1004) == 0         # G % 8 != 0: no 8 B loads
    assert query(G=0x1002) == 0
    assert query(ldg=C + 2) == 0        # ldg % 4 != 0
    assert query(W=0x2008) == 0 == fp32_query(W=0x2008)  # the fp32 rule still decides first
    g = graph()
    g.self_row0 = 64
    assert query(g) == 0
    grl_option("graphconv_bwd_bf16", 0)
    assert query() == 0 and fp32_query() == ONE
    rc, msg = bwd(graph())
    assert rc == _lib.GRL_E_UNSUPPORTED and b"graphconv_bwd_bf16" in msg
    grl_option("graphconv_bwd_bf16", 1)
    assert query() == ONE
    grl_option("graphconv_fused", 0)  # the shape rule's own option
    assert query() == 0


def test_workspace_query_is_zero_on_bad_arguments():
    assert getattr(_lib.lib(), QUERY)(None, 0x1000, C, C, 0x2000, F, 0x4000, F) == 0
    assert query(graph(num_rows=0)) == 0
    assert query(dX=None) == 0
    assert query(lddx=F - 2) == 0 and query(ldg=C - 4) == 0
    assert query(c=0) == 0 and query(f=0) == 0
    assert query(c=96, ldg=96) == 0  # not a gathered width the kernel has


def test_the_option_is_listed_with_its_bounds():
    assert _lib.get_option("graphconv_bwd_bf16") in (0, 1)
    with pytest.raises(_lib.GrlError, match="outside"):
        _lib.set_option("graphconv_bwd_bf16", 2)


def test_relu_grad_bf16_empty_operands_and_host_checks():
    fn = getattr(_lib.lib(), RELU)
    # M == 0: OK with a NULL workspace when db is NULL; C == 0: OK
    assert fn(None, 8, None, 8, None, 8, None, None, 0, 8, None, 0, None) == _lib.GRL_OK
    assert fn(None, 0, None, 0, None, 0, None, None, 5, 0, None, 0, None) == _lib.GRL_OK
    assert fn(None, 8, None, 8, None, 8, None, None, -1, 8, None, 0, None) == _lib.GRL_E_INVALID
    assert fn(None, 8, 0x2000, 8, None, 8, None, None, 5, 8, None, 0, None) == _lib.GRL_E_INVALID  # NULL g
    assert b"NULL pointer" in _lib.lib().grl_last_error()
    assert fn(0x1000, 6, 0x2000, 8, None, 0, None, None, 5, 8, None, 0, None) == _lib.GRL_E_INVALID  # ldg < C
    assert fn(0x1000, 8, 0x2000, 8, 0x3000, 6, None, None, 5, 8, None, 0, None) == _lib.GRL_E_INVALID  # lde < C
    assert fn(0x1001, 8, 0x2000, 8, None, 0, None, None, 5, 8, None, 0, None) == _lib.GRL_E_INVALID  # an odd address
    # db wants the workspace of grl_relu_grad
    need = _lib.lib().grl_relu_grad_workspace_size(5, 8)
    assert fn(0x1000, 8, 0x2000, 8, None, 0, None, 0x5000, 5, 8, 0x6000, need - 1, None) == _lib.GRL_E_WORKSPACE
    assert fn(0x1000, 8, 0x2000, 8, None, 0, None, 0x5000, 5, 8, None, 0, None) == _lib.GRL_E_WORKSPACE
