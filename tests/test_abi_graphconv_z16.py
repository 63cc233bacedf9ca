"""CPU-only: the bf16-output GraphConv training forward with a bf16 Z
(grl_graphconv_fwd_train_bf16_z16 and its workspace query): exported, declared
in include/grl.h and bound; its own argument errors (the sibling entry's, plus a
NULL or odd Z) are GRL_E_INVALID decided on the host; a short workspace is
GRL_E_WORKSPACE; and the path rule read through the query -- the sibling's
one-kernel rule AND Z 8 B-aligned, else the SpMM + linear chain with an fp32 Z
scratch and an fp32 [num_rows, C] scratch in the workspace.  No pointer is
dereferenced and no device work is issued."""
import ctypes
import os
import re

import pytest

from grl import _lib

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "grl.h")
TRAIN, QUERY = "grl_graphconv_fwd_train_bf16_z16", "grl_graphconv_fwd_train_bf16_z16_workspace_query"
SIB, SIB_QUERY = "grl_graphconv_fwd_train_bf16_to_bf16", "grl_graphconv_fwd_bf16_to_bf16_workspace_query"

ROWS, TYPES, F, C = 20011, 6, 256, 256  # above the x6 GEMM's 1.6e10-flop floor
K = 7 * F
ONE = 7 * 256 * 1536 + 256              # W's planes + the status word: the one-kernel answer


def up(n):
    return (n + 255) // 256 * 256


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


def train(g, out=0x4000, ldo=C, X=0x1000, Z=0x5000, ldx=F, ws=None, ws_bytes=0):
    rc = getattr(_lib.lib(), TRAIN)(ctypes.byref(g), X, ldx, F, 0x2000, None, C, 0, out, ldo, Z, None, ws, ws_bytes,
                                    None)
    return rc, _lib.lib().grl_last_error()


def query(g=None, X=0x1000, ldx=F, W=0x2000, out=0x4000, ldo=C, Z=0x5000, f=F, c=C):
    g = graph() if g is None else g
    return getattr(_lib.lib(), QUERY)(ctypes.byref(g), X, ldx, f, W, c, out, ldo, Z)


def two_kernel(rows=ROWS, k=K, c=C):
    return up(rows * k * 4) + up(rows * c * 4) + _lib.lib().grl_linear_fwd_ex_workspace_size(rows, k, c, 0)


@pytest.mark.parametrize("name", [TRAIN, QUERY])
def test_symbols_are_exported_declared_and_bound(name):
    assert hasattr(_lib.lib(), name)
    assert name in declared_functions()
    assert name in _lib.SIGNATURES


def test_signatures_relate_to_the_siblings():
    assert _lib.SIGNATURES[TRAIN] == _lib.SIGNATURES[SIB]  # Z a pointer either way
    res, args = _lib.SIGNATURES[QUERY]
    tres, targs = _lib.SIGNATURES[SIB_QUERY]
    assert res == tres and list(args) == list(targs) + [_lib._c_vp]  # the sibling's query, then Z


def test_own_argument_errors_are_refused_on_the_host():
    name = TRAIN.encode()
    for kw in ({"out": None}, {"Z": None}):
        rc, msg = train(graph(), **kw)
        assert rc == _lib.GRL_E_INVALID and b"NULL pointer" in msg and name in msg, kw
    rc, msg = train(graph(), ldo=C - 2)
    assert rc == _lib.GRL_E_INVALID and b"ldo" in msg and name in msg
    rc, msg = train(graph(num_rows=0), ldo=C - 2)  # refused before the empty graph's early return
    assert rc == _lib.GRL_E_INVALID and b"ldo" in msg
    for kw in ({"out": 0x4001}, {"X": 0x1001}, {"Z": 0x5001}):
        rc, msg = train(graph(), **kw)
        assert rc == _lib.GRL_E_INVALID and b"2-B aligned" in msg and name in msg, kw
    rc, msg = train(graph(), ldx=F - 4)
    assert rc == _lib.GRL_E_INVALID and b"ldx" in msg
    rc, msg = train(graph(num_types=0))
    assert rc == _lib.GRL_E_INVALID and b"num_types" in msg
    rc = getattr(_lib.lib(), TRAIN)(None, 0x1000, F, F, 0x2000, None, C, 0, 0x4000, C, 0x5000, None, None, 0, None)
    assert rc == _lib.GRL_E_INVALID and b"NULL" in _lib.lib().grl_last_error()
    rc, _ = train(graph(num_rows=0))  # no rows: nothing to do
    assert rc == _lib.GRL_OK


def test_a_short_workspace_is_refused(grl_option):
    name = TRAIN.encode()
    rc, msg = train(graph())  # one-kernel shape, no workspace: the two-kernel form's size is what is missing
    assert rc == _lib.GRL_E_WORKSPACE and name in msg
    rc, msg = train(graph(), ws=0x100000, ws_bytes=ONE - 1)
    assert rc == _lib.GRL_E_WORKSPACE and name in msg
    grl_option("graphconv_fused", 0)
    rc, msg = train(graph(), ws=0x100000, ws_bytes=two_kernel() - 1)
    assert rc == _lib.GRL_E_WORKSPACE and name in msg


def test_workspace_query_is_zero_on_bad_arguments():
    assert getattr(_lib.lib(), QUERY)(None, 0x1000, F, F, 0x2000, C, 0x4000, C, 0x5000) == 0
    assert query(graph(num_rows=0)) == 0
    assert query(ldo=C - 2) == 0
    assert query(f=0) == 0 and query(c=0) == 0


def test_constants():
    assert ONE == 2752768 and 2 * ROWS * K * C > 1.6e10 and ONE < ROWS * K * 2


def test_the_one_kernel_answers_the_planes():
    assert query() == ONE
    assert query(ldo=2 * C) == ONE and query(out=0x4000 + 2 * C, ldo=2 * C) == ONE
    assert query(Z=0x5008) == ONE  # 8 B is all a Z row's stores need


def test_elsewhere_the_chain_with_both_scratches(grl_option):
    two = two_kernel()
    assert two >= ROWS * K * 4 + ROWS * C * 4
    for kw in ({"Z": 0x5004}, {"Z": 0x5002}, {"out": 0x4002}, {"ldo": C + 1}, {"X": 0x1004}, {"W": 0x2008}):
        assert query(**kw) == two, kw
    grl_option("graphconv_fused", 0)  # the option alone forces the fallback
    assert query() == two
    grl_option("graphconv_fused", 1)
    assert query() == ONE
    g = graph(num_rows=300)  # below the x6 floor
    assert query(g, f=64, ldx=64, c=32, ldo=32) == two_kernel(300, 7 * 64, 32)
