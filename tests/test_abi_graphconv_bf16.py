"""CPU-only: the bf16-table GraphConv forward entries
(grl_graphconv_fwd_bf16, grl_graphconv_fwd_train_bf16 and their workspace
query) are exported, declared in include/grl.h, bound with the fp32 entries'
argument lists, and validate their arguments on the host with the fp32
entries' checks and error codes.  No device work is issued."""
import ctypes
import os
import re

import pytest

from grl import _lib

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "grl.h")
FWD, TRAIN, QUERY = "grl_graphconv_fwd_bf16", "grl_graphconv_fwd_train_bf16", "grl_graphconv_fwd_bf16_workspace_query"
TWINS = {FWD: "grl_graphconv_fwd", TRAIN: "grl_graphconv_fwd_train", QUERY: "grl_graphconv_fwd_workspace_query"}


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", src))


def graph(num_rows=0, num_types=6, has_self=1):
    g = _lib.GrlTypedCsr()
    g.num_rows, g.num_types, g.has_self = num_rows, num_types, has_self  # no rows: the pointers are never looked at
    return g


def fwd(g, ldx=8, F=8, C=4, ptrs=False):
    p = 16 if ptrs else None  # a non-NULL address that a failed check never dereferences
    rc = getattr(_lib.lib(), FWD)(ctypes.byref(g) if g is not None else None, p, ldx, F, p, None, C, 0, p, None, None, 0,
                                  None)
    return rc, _lib.lib().grl_last_error()


def train(g, ldx=8, F=8, C=4, ptrs=False):
    p = 16 if ptrs else None
    rc = getattr(_lib.lib(), TRAIN)(ctypes.byref(g) if g is not None else None, p, ldx, F, p, None, C, 0, p, p, None,
                                    None, 0, None)
    return rc, _lib.lib().grl_last_error()


@pytest.mark.parametrize("name", [FWD, TRAIN, QUERY])
def test_symbols_are_exported_declared_and_bound(name):
    assert hasattr(_lib.lib(), name)
    assert name in declared_functions()
    assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES[TWINS[name]]  # the fp32 entry's arguments: X a pointer either way


@pytest.mark.parametrize("entry,name", [(fwd, FWD), (train, TRAIN)])
def test_invalid_arguments_are_refused_on_the_host(entry, name):
    rc, msg = entry(None)
    assert rc == _lib.GRL_E_INVALID and name.encode() in msg and b"NULL" in msg
    rc, msg = entry(graph(num_types=0))
    assert rc == _lib.GRL_E_INVALID and b"num_types" in msg and name.encode() in msg
    rc, msg = entry(graph(), ldx=4, F=8)  # ldx < F
    assert rc == _lib.GRL_E_INVALID and b"ldx" in msg and name.encode() in msg
    rc, msg = entry(graph(), C=0)
    assert rc == _lib.GRL_E_INVALID and b"C > 0" in msg and name.encode() in msg
    rc, msg = entry(graph(num_rows=10))  # rows, but no X / W / out (/ Z)
    assert rc == _lib.GRL_E_INVALID and b"NULL pointer" in msg and name.encode() in msg
    rc, _ = entry(graph())  # no rows: nothing to do, no pointer needed
    assert rc == _lib.GRL_OK


def test_the_checks_are_the_fp32_entries():
    """The same arguments give the same status through the fp32 entry."""
    lib = _lib.lib()
    for g, ldx, F, C in ((None, 8, 8, 4), (graph(num_types=0), 8, 8, 4), (graph(), 4, 8, 4), (graph(), 8, 8, 0),
                         (graph(num_rows=10), 8, 8, 4), (graph(), 8, 8, 4)):
        ref = ctypes.byref(g) if g is not None else None
        rc32 = lib.grl_graphconv_fwd(ref, None, ldx, F, None, None, C, 0, None, None, None, 0, None)
        assert fwd(g, ldx, F, C)[0] == rc32
        rc32 = lib.grl_graphconv_fwd_train(ref, None, ldx, F, None, None, C, 0, None, None, None, None, 0, None)
        assert train(g, ldx, F, C)[0] == rc32


def test_workspace_query_is_zero_on_bad_arguments():
    q = getattr(_lib.lib(), QUERY)
    assert q(None, None, 8, 8, None, 4) == 0
    assert q(ctypes.byref(graph()), None, 8, 8, None, 4) == 0  # no rows
    assert q(ctypes.byref(graph(num_rows=10, num_types=0)), None, 8, 8, None, 4) == 0
    assert q(ctypes.byref(graph(num_rows=10)), None, 8, 0, None, 4) == 0
    assert q(ctypes.byref(graph(num_rows=10)), None, 8, 8, None, 0) == 0


def test_workspace_query_of_a_small_graph_is_the_two_kernel_size():
    """A graph below the x6 GEMM's floor takes the SpMM + linear chain: Z whole
    plus the linear's workspace, what the fp32 query answers for it."""
    lib = _lib.lib()
    g = graph(num_rows=300)
    got = getattr(lib, QUERY)(ctypes.byref(g), 16, 64, 64, 16, 32)
    assert got == lib.grl_graphconv_fwd_workspace_query(ctypes.byref(g), 16, 64, 64, 16, 32)
    assert got >= 300 * 7 * 64 * 4
