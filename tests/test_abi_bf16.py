"""CPU-only: grl_typed_spmm_fwd_bf16 (the typed SpMM over a bf16 feature
table) is exported, bound, and validates its arguments on the host like
grl_typed_spmm_fwd_slice.  No device work is issued."""
import ctypes

from grl import _lib

NAME = "grl_typed_spmm_fwd_bf16"


def call(g, ldx, F, ldz, zseg, self_col0=0):
    rc = getattr(_lib.lib(), NAME)(ctypes.byref(g) if g is not None else None, None, ldx, F, self_col0, None, ldz,
                                   zseg, None, None)
    return rc, _lib.lib().grl_last_error()


def empty_graph(num_types=6, has_self=1):
    g = _lib.GrlTypedCsr()
    g.num_rows, g.num_types, g.has_self = 0, num_types, has_self  # no rows: the pointers are never looked at
    return g


def test_symbol_is_exported_and_bound():
    assert hasattr(_lib.lib(), NAME)
    assert NAME in _lib.SIGNATURES
    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES["grl_typed_spmm_fwd_slice"]  # the slice form's arguments


def test_null_graph_names_the_function():
    rc, msg = call(None, 8, 8, 56, 8)
    assert rc == _lib.GRL_E_INVALID and NAME.encode() in msg and b"NULL" in msg


def test_zero_rows_is_ok_without_pointers():
    rc, _ = call(empty_graph(), 8, 8, 56, 8)
    assert rc == _lib.GRL_OK


def test_shape_validation_is_host_side():
    rc, msg = call(empty_graph(num_types=0), 8, 8, 56, 8)
    assert rc == _lib.GRL_E_INVALID and b"num_types" in msg and NAME.encode() in msg
    rc, msg = call(empty_graph(), 4, 8, 56, 8)  # ldx < F
    assert rc == _lib.GRL_E_INVALID and b"ldx" in msg and NAME.encode() in msg
    rc, msg = call(empty_graph(), 8, 8, 56, 4)  # zseg < F
    assert rc == _lib.GRL_E_INVALID and b"zseg" in msg and NAME.encode() in msg
    rc, msg = call(empty_graph(), 8, 8, 6 * 16 + 7, 16)  # 7 segments of stride 16, the last 8 wide: ldz >= 104
    assert rc == _lib.GRL_E_INVALID and b"ldz" in msg and NAME.encode() in msg
    rc, _ = call(empty_graph(), 8, 8, 6 * 16 + 8, 16)
    assert rc == _lib.GRL_OK
    rc, msg = call(empty_graph(), 8, 8, 56, 8, self_col0=-1)
    assert rc == _lib.GRL_E_INVALID and b"self_col0" in msg


def test_rows_without_pointers_are_refused():
    g = empty_graph()
    g.num_rows = 10
    rc, msg = call(g, 8, 8, 56, 8)
    assert rc == _lib.GRL_E_INVALID and b"NULL pointer" in msg and NAME.encode() in msg
