"""CPU-only: the bf16-output GraphConv forward entries
(grl_graphconv_fwd_bf16_to_bf16, grl_graphconv_fwd_train_bf16_to_bf16 and
their workspace query): exported, declared in include/grl.h and bound; their
own argument errors (NULL out, ldo < C, an odd address for a 2-byte type) are
GRL_E_INVALID decided on the host; and the path rule read through the
workspace query -- the bf16-table rule AND out 4 B-aligned with an even row
stride, else the SpMM + linear chain with an fp32 [num_rows, C] scratch more.
No pointer is dereferenced and no device work is issued."""
import ctypes
import os
import re

import pytest

from grl import _lib

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "grl.h")
FWD, TRAIN = "grl_graphconv_fwd_bf16_to_bf16", "grl_graphconv_fwd_train_bf16_to_bf16"
QUERY = "grl_graphconv_fwd_bf16_to_bf16_workspace_query"
TWINS = {FWD: "grl_graphconv_fwd_bf16", TRAIN: "grl_graphconv_fwd_train_bf16",
         QUERY: "grl_graphconv_fwd_bf16_workspace_query"}

ROWS, TYPES, F, C = 20011, 6, 256, 256  # above the x6 GEMM's 1.6e10-flop floor (test_abi_graphconv_path_rule.py)
ONE = 7 * 256 * 1536 + 256              # W's planes + the status word: the one-kernel answer
SCRATCH = (ROWS * C * 4 + 255) // 256 * 256  # the linear's fp32 [ROWS, C] of the two-kernel form


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


def fwd(g, out=0x4000, ldo=C, X=0x1000):
    rc = getattr(_lib.lib(), FWD)(ctypes.byref(g), X, F, F, 0x2000, None, C, 0, out, ldo, None, None, 0, None)
    return rc, _lib.lib().grl_last_error()


def train(g, out=0x4000, ldo=C, X=0x1000):
    rc = getattr(_lib.lib(), TRAIN)(ctypes.byref(g), X, F, F, 0x2000, None, C, 0, out, ldo, 0x5000, None, None, 0,
                                    None)
    return rc, _lib.lib().grl_last_error()


def query(g=None, X=0x1000, ldx=F, W=0x2000, out=0x4000, ldo=C, f=F, c=C):
    g = graph() if g is None else g
    return getattr(_lib.lib(), QUERY)(ctypes.byref(g), X, ldx, f, W, c, out, ldo)


def bf16_query(g=None, X=0x1000, ldx=F, f=F, c=C):
    g = graph() if g is None else g
    return _lib.lib().grl_graphconv_fwd_bf16_workspace_query(ctypes.byref(g), X, ldx, f, 0x2000, c)


@pytest.mark.parametrize("name", [FWD, TRAIN, QUERY])
def test_symbols_are_exported_declared_and_bound(name):
    assert hasattr(_lib.lib(), name)
    assert name in declared_functions()
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    tres, targs = _lib.SIGNATURES[TWINS[name]]
    assert res == tres
    if name == QUERY:  # the _bf16 query's arguments, then out and ldo
        assert list(args) == list(targs) + [_lib._c_vp, _lib._c_i64]
    else:  # the _bf16 entry's arguments with ldo after out
        assert list(args[:9]) + list(args[10:]) == list(targs) and args[9] == _lib._c_i64


@pytest.mark.parametrize("entry,name", [(fwd, FWD), (train, TRAIN)])
def test_own_argument_errors_are_refused_on_the_host(entry, name):
    rc, msg = entry(graph(), out=None)
    assert rc == _lib.GRL_E_INVALID and b"NULL pointer" in msg and name.encode() in msg
    rc, msg = entry(graph(), ldo=C - 2)
    assert rc == _lib.GRL_E_INVALID and b"ldo" in msg and name.encode() in msg
    rc, msg = entry(graph(num_rows=0), ldo=C - 2)  # refused before the empty graph's early return
    assert rc == _lib.GRL_E_INVALID and b"ldo" in msg
    rc, msg = entry(graph(), out=0x4001)
    assert rc == _lib.GRL_E_INVALID and b"2-B aligned" in msg and name.encode() in msg
    rc, msg = entry(graph(), X=0x1001)
    assert rc == _lib.GRL_E_INVALID and b"2-B aligned" in msg and name.encode() in msg
    rc, _ = entry(graph(num_rows=0))  # no rows: nothing to do
    assert rc == _lib.GRL_OK


def test_the_bf16_entries_checks_still_apply():
    lib = _lib.lib()
    rc = getattr(lib, FWD)(None, 0x1000, F, F, 0x2000, None, C, 0, 0x4000, C, None, None, 0, None)
    assert rc == _lib.GRL_E_INVALID and b"NULL" in lib.grl_last_error()
    rc = getattr(lib, FWD)(ctypes.byref(graph()), 0x1000, F - 4, F, 0x2000, None, C, 0, 0x4000, C, None, None, 0, None)
    assert rc == _lib.GRL_E_INVALID and b"ldx" in lib.grl_last_error()
    rc = getattr(lib, FWD)(ctypes.byref(graph(num_types=0)), 0x1000, F, F, 0x2000, None, C, 0, 0x4000, C, None, None,
                           0, None)
    assert rc == _lib.GRL_E_INVALID and b"num_types" in lib.grl_last_error()


def test_workspace_query_is_zero_on_bad_arguments():
    assert getattr(_lib.lib(), QUERY)(None, 0x1000, F, F, 0x2000, C, 0x4000, C) == 0
    assert query(graph(num_rows=0)) == 0
    assert query(ldo=C - 2) == 0
    assert query(f=0) == 0 and query(c=0) == 0


def test_constants():
    assert ONE == 2752768 and 2 * ROWS * 7 * F * C > 1.6e10 and SCRATCH >= ROWS * C * 4


def test_the_one_kernel_answers_the_planes():
    assert query() == ONE == bf16_query()
    assert query(ldo=2 * C) == ONE and query(out=0x4000 + 2 * C, ldo=2 * C) == ONE  # the two slices of a [N, 2C] table
    assert query(ldo=C + 2, out=0x4004) == ONE


def test_out_rows_off_the_dword_grid_take_the_chain_with_the_scratch(grl_option):
    """Same shape and table; out 2 B- but not 4 B-aligned, or an odd row
    stride: no dword stores, so the two-kernel form, whose size is the _bf16
    entry's two-kernel size (read with graphconv_fused = 0) plus the fp32
    [ROWS, C] the linear writes."""
    grl_option("graphconv_fused", 0)
    two = bf16_query()
    assert two >= ROWS * 7 * F * 4
    assert query() == two + SCRATCH  # the option alone
    grl_option("graphconv_fused", 1)
    assert bf16_query() == ONE
    assert query(out=0x4002) == two + SCRATCH
    assert query(ldo=C + 1) == two + SCRATCH
    assert query(out=0x4002, ldo=C + 1) == two + SCRATCH
    # the table's own rule still decides first (test_abi_graphconv_path_rule.py)
    assert query(X=0x1004) == two + SCRATCH == bf16_query(X=0x1004) + SCRATCH
    assert query(W=0x2008) == two + SCRATCH


def test_a_shape_below_the_x6_floor_takes_the_chain_with_the_scratch():
    g = graph(num_rows=300)
    two = bf16_query(g, f=64, ldx=64, c=32)
    assert two >= 300 * 7 * 64 * 4
    assert query(g, f=64, ldx=64, c=32, ldo=32) == two + (300 * 32 * 4 + 255) // 256 * 256
