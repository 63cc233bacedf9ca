"""CPU-only: grl_typed_spmm_fwd_bf16_to_bf16 (bf16 table in, bf16 Z out) and
grl_typed_spmm_bwd_bf16 (bf16 dZ gathered, bf16 dX out) are exported, bound,
and validate their arguments on the host with the checks of
grl_typed_spmm_fwd_bf16 and grl_typed_spmm_bwd_slice, under their own names.
No device work is issued."""
import ctypes

from grl import _lib

FWD = "grl_typed_spmm_fwd_bf16_to_bf16"
BWD = "grl_typed_spmm_bwd_bf16"


def last():
    return _lib.lib().grl_last_error()


def fwd(g, ldx, F, ldz, zseg, self_col0=0, X=None, Z=None):
    rc = getattr(_lib.lib(), FWD)(ctypes.byref(g) if g is not None else None, X, ldx, F, self_col0, Z, ldz, zseg, None,
                                  None)
    return rc, last()


def bwd(g, F_total, col0, F, lddx, dZ=None, dX=None):
    rc = getattr(_lib.lib(), BWD)(ctypes.byref(g) if g is not None else None, dZ, F_total, col0, F, dX, lddx, None,
                                  None)
    return rc, last()


def empty_csr(num_types=6, has_self=1):
    g = _lib.GrlTypedCsr()
    g.num_rows, g.num_types, g.has_self = 0, num_types, has_self  # no rows: the pointers are never looked at
    return g


def empty_csc(num_types=6, has_self=1):
    g = _lib.GrlTypedCsc()
    g.num_rows, g.self_rows, g.num_types, g.has_self = 0, 0, num_types, has_self
    return g


def test_symbols_are_exported_and_bound():
    for name, like in ((FWD, "grl_typed_spmm_fwd_bf16"), (BWD, "grl_typed_spmm_bwd_slice")):
        assert hasattr(_lib.lib(), name)
        assert name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[like]  # the slice forms' arguments


def test_null_graph_names_the_function():
    rc, msg = fwd(None, 8, 8, 56, 8)
    assert rc == _lib.GRL_E_INVALID and FWD.encode() in msg and b"NULL" in msg
    rc, msg = bwd(None, 8, 0, 8, 8)
    assert rc == _lib.GRL_E_INVALID and BWD.encode() in msg and b"NULL" in msg


def test_zero_rows_is_ok_without_pointers():
    assert fwd(empty_csr(), 8, 8, 56, 8)[0] == _lib.GRL_OK
    assert bwd(empty_csc(), 8, 0, 8, 8)[0] == _lib.GRL_OK


def test_forward_shape_validation_is_host_side():
    rc, msg = fwd(empty_csr(num_types=0), 8, 8, 56, 8)
    assert rc == _lib.GRL_E_INVALID and b"num_types" in msg and FWD.encode() in msg
    rc, msg = fwd(empty_csr(), 4, 8, 56, 8)  # ldx < F
    assert rc == _lib.GRL_E_INVALID and b"ldx" in msg and FWD.encode() in msg
    rc, msg = fwd(empty_csr(), 8, 8, 56, 4)  # zseg < F
    assert rc == _lib.GRL_E_INVALID and b"zseg" in msg and FWD.encode() in msg
    rc, msg = fwd(empty_csr(), 8, 8, 6 * 16 + 7, 16)  # 7 segments of stride 16, the last 8 wide: ldz >= 104
    assert rc == _lib.GRL_E_INVALID and b"ldz" in msg and FWD.encode() in msg
    assert fwd(empty_csr(), 8, 8, 6 * 16 + 8, 16)[0] == _lib.GRL_OK
    rc, msg = fwd(empty_csr(), 8, 8, 56, 8, self_col0=-1)
    assert rc == _lib.GRL_E_INVALID and b"self_col0" in msg and FWD.encode() in msg


def test_backward_shape_validation_is_host_side():
    rc, msg = bwd(empty_csc(num_types=0), 8, 0, 8, 8)
    assert rc == _lib.GRL_E_INVALID and b"num_types" in msg and BWD.encode() in msg
    rc, msg = bwd(empty_csc(), 8, 0, 8, 4)  # lddx < F
    assert rc == _lib.GRL_E_INVALID and b"lddx" in msg and BWD.encode() in msg
    rc, msg = bwd(empty_csc(), 16, 9, 8, 8)  # columns [9, 17) of 16
    assert rc == _lib.GRL_E_INVALID and b"outside" in msg and BWD.encode() in msg
    rc, msg = bwd(empty_csc(), 16, -1, 8, 8)
    assert rc == _lib.GRL_E_INVALID and b"outside" in msg and BWD.encode() in msg
    assert bwd(empty_csc(), 16, 8, 8, 8)[0] == _lib.GRL_OK
    g = empty_csc()
    g.self_rows = 1  # more self rows than rows
    rc, msg = bwd(g, 8, 0, 8, 8)
    assert rc == _lib.GRL_E_INVALID and b"self_rows" in msg and BWD.encode() in msg


def test_rows_without_pointers_are_refused():
    g = empty_csr()
    g.num_rows = 10
    rc, msg = fwd(g, 8, 8, 56, 8)
    assert rc == _lib.GRL_E_INVALID and b"NULL pointer" in msg and FWD.encode() in msg
    c = empty_csc()
    c.num_rows = c.self_rows = 10
    rc, msg = bwd(c, 8, 0, 8, 8)
    assert rc == _lib.GRL_E_INVALID and b"NULL pointer" in msg and BWD.encode() in msg


def test_odd_pointers_are_refused():
    """bf16 elements are 2 B: an odd address is refused on the host before any launch (the graph's own
    pointers are never dereferenced by the check)."""
    buf = (ctypes.c_uint16 * 64)()
    a = ctypes.addressof(buf)
    ptr = (ctypes.c_int32 * 16)()
    g = empty_csr()
    g.num_rows, g.rowptr, g.nnz = 1, ctypes.addressof(ptr), 0
    for X, Z in ((a + 1, a + 64), (a, a + 65)):
        rc, msg = fwd(g, 8, 8, 56, 8, X=X, Z=Z)
        assert rc == _lib.GRL_E_INVALID and b"2 B-aligned" in msg and FWD.encode() in msg
    c = empty_csc()
    c.num_rows, c.self_rows, c.colptr, c.nnz = 1, 1, ctypes.addressof(ptr), 0
    for dZ, dX in ((a + 1, a + 64), (a, a + 65)):
        rc, msg = bwd(c, 8, 0, 8, 8, dZ=dZ, dX=dX)
        assert rc == _lib.GRL_E_INVALID and b"2 B-aligned" in msg and BWD.encode() in msg
