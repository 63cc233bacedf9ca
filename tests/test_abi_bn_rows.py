"""CPU-only: the batch-norm-over-rows entries (grl_bn_rows_*) are exported,
declared in include/grl.h and bound; their host-side argument errors are
GRL_E_INVALID with a message naming the entry and the fault, before any
pointer is dereferenced or any device work is issued; an empty table is
GRL_OK with no launch; the workspace query depends on (rows, cols) only."""
import os
import re

import pytest

from grl import _lib

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "grl.h")
WS, TRAIN, EVAL, BWD = ("grl_bn_rows_workspace_size", "grl_bn_rows_fwd_train", "grl_bn_rows_fwd_eval",
                        "grl_bn_rows_bwd")
X, Y, DY, DX, M, S, W = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
INVALID, OK = _lib.GRL_E_INVALID, _lib.GRL_OK


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", src))


def err():
    return _lib.lib().grl_last_error()


def ws_size(rows, cols):
    return _lib.lib().grl_bn_rows_workspace_size(rows, cols)


@pytest.mark.parametrize("name", [WS, TRAIN, EVAL, BWD])
def test_symbols_are_exported_declared_and_bound(name):
    assert hasattr(_lib.lib(), name)
    assert name in declared_functions()
    assert name in _lib.SIGNATURES


def train(x=X, ldx=8, rows=5, cols=8, y=Y, ldy=8, mean=M, invstd=S, ws=W, ws_bytes=None, gamma=None, beta=None):
    if ws_bytes is None:
        ws_bytes = ws_size(max(rows, 0), max(cols, 0))
    return _lib.lib().grl_bn_rows_fwd_train(x, ldx, rows, cols, gamma, beta, 1e-5, 0.2, 0.1, None, None, y, ldy, mean,
                                            invstd, ws, ws_bytes, None)


def evaluate(x=X, ldx=8, rows=5, cols=8, rm=M, rv=S, y=Y, ldy=8):
    return _lib.lib().grl_bn_rows_fwd_eval(x, ldx, rows, cols, None, None, rm, rv, 1e-5, 0.2, y, ldy, None)


def bwd(dy=DY, lddy=8, y=Y, ldy=8, x=X, ldx=8, rows=5, cols=8, mean=M, invstd=S, dx=DX, lddx=8, ws=W, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = ws_size(max(rows, 0), max(cols, 0))
    return _lib.lib().grl_bn_rows_bwd(dy, lddy, y, ldy, x, ldx, rows, cols, None, mean, invstd, 0.2, dx, lddx, None,
                                      None, ws, ws_bytes, None)


def test_empty_tables_are_ok_without_a_launch():
    for fn in (train, evaluate, bwd):
        assert fn(rows=0) == OK
        assert fn(cols=0) == OK
    # ... before any pointer is looked at
    assert train(x=None, y=None, mean=None, invstd=None, ws=None, rows=0) == OK
    assert evaluate(x=None, y=None, rm=None, rv=None, cols=0) == OK
    assert bwd(dy=None, y=None, x=None, dx=None, mean=None, invstd=None, ws=None, rows=0) == OK
    assert ws_size(0, 8) == 0 and ws_size(8, 0) == 0


@pytest.mark.parametrize("fn,name", [(train, TRAIN), (evaluate, EVAL), (bwd, BWD)])
def test_negative_sizes_and_short_strides(fn, name):
    assert fn(rows=-1) == INVALID and name.encode() in err() and b"negative size" in err()
    assert fn(cols=-8) == INVALID and b"negative size" in err()
    assert fn(ldx=7) == INVALID and name.encode() in err() and b"strides" in err()
    assert fn(ldy=7) == INVALID and b"strides" in err()
    assert fn(ldx=7, rows=0) == INVALID  # refused before the early return, as the dropout entries do


def test_backward_strides():
    assert bwd(lddy=7) == INVALID and b"strides" in err()
    assert bwd(lddx=7) == INVALID and b"strides" in err()


def test_null_pointers():
    for kw in ({"x": None}, {"y": None}, {"mean": None}, {"invstd": None}):
        assert train(**kw) == INVALID and TRAIN.encode() in err() and b"NULL pointer" in err(), kw
    for kw in ({"x": None}, {"y": None}, {"rm": None}, {"rv": None}):
        assert evaluate(**kw) == INVALID and EVAL.encode() in err() and b"NULL pointer" in err(), kw
    for kw in ({"dy": None}, {"y": None}, {"x": None}, {"dx": None}, {"mean": None}, {"invstd": None}):
        assert bwd(**kw) == INVALID and BWD.encode() in err() and b"NULL pointer" in err(), kw


def test_training_needs_two_rows():
    assert train(rows=1) == INVALID and TRAIN.encode() in err() and b"at least 2 rows" in err()
    assert train(rows=1, cols=0) == OK  # nothing to normalise


def test_short_workspace():
    need = ws_size(5, 8)
    assert need > 0
    for fn, name in ((train, TRAIN), (bwd, BWD)):
        assert fn(ws_bytes=need - 1) == INVALID and name.encode() in err() and b"workspace too small" in err()
        assert fn(ws=None, ws_bytes=0) == INVALID and b"workspace" in err()
        assert fn(ws=W + 4) == INVALID and b"workspace" in err()  # fp64 partials: 8-B aligned


def test_workspace_query_depends_on_rows_and_cols_only(monkeypatch):
    shapes = [(2, 1), (5, 6), (1024, 32), (1025, 32), (4099, 256), (300, 1028), (1 << 20, 256), (1 << 20, 512)]
    first = [ws_size(r, c) for r, c in shapes]
    assert all(b > 0 and b % 8 == 0 for b in first)
    for k, v in (("HIP_VISIBLE_DEVICES", "3"), ("ROCR_VISIBLE_DEVICES", "1"), ("GRL_BN_BLOCKS", "7")):
        monkeypatch.setenv(k, v)
    assert [ws_size(r, c) for r, c in shapes] == first
    # the partials of every row block and the backward's two mean vectors, fp64: growing with the rows up to
    # the block cap, then flat
    assert ws_size(1 << 20, 256) == ws_size(1 << 21, 256)
    assert ws_size(512, 32) < ws_size(513, 32) < ws_size(1025, 32)
    assert ws_size(1 << 20, 256) <= 8 << 20
