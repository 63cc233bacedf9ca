"""CPU-only: the two entries of row_linear's backward over a bf16 table
 -- grl_linear_bwd_weight_bf16z (dW from a bf16 Z and an fp32
g; gemm_x3ta_kernel) and grl_linear_fwd_to_bf16 (the x6 forward GEMM storing
bf16 rows; gemm_x6_kernel's EPI_BF16), each with its workspace query: exported,
declared in include/grl.h and bound; the dw_bf16z_f32g and linear_out_bf16 path
options; every GRL_E_INVALID, GRL_E_UNSUPPORTED and GRL_E_WORKSPACE case
decided on the host; the eligibility rules read through the queries, whose
nonzero answers are grl_linear_bwd_weight_workspace_size and
grl_linear_fwd_ex_workspace_size.  The dW entry goes through the bad-call table
the entries of its host path share (test_abi_shared_host_paths.DW_CASES) with
the codes the other bf16 entries give.  No pointer is dereferenced and no
device work is issued.

The numerical argument of the dW kernel -- x3a_mfma's three products are the
six on a one-plane a, bit for bit -- is held on the numpy model in
test_abi_linear_fwd_bf16x.py and is not restated here."""
import os
import re

import pytest

import test_abi_shared_host_paths as shared
from grl import _lib

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "grl.h")
DW, DW_QUERY = "grl_linear_bwd_weight_bf16z", "grl_linear_bwd_weight_bf16z_workspace_query"
FWD, FWD_QUERY = "grl_linear_fwd_to_bf16", "grl_linear_fwd_to_bf16_workspace_query"

M, K, C = 20011, 1792, 256  # above the split-bf16 kernels' 1.6e10-flop floor
BELOW = 17438               # below it: 2 * 17438 * 1792 * 256 < 1.6e10
Z, G, W, B, OUT, DWP, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000  # never dereferenced
OK, INVALID, WORKSPACE, UNSUPPORTED = _lib.GRL_OK, _lib.GRL_E_INVALID, _lib.GRL_E_WORKSPACE, _lib.GRL_E_UNSUPPORTED


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", src))


@pytest.mark.parametrize("name", [DW, DW_QUERY, FWD, FWD_QUERY])
def test_symbols_are_exported_declared_and_bound(name):
    assert hasattr(_lib.lib(), name)
    assert name in declared_functions()
    assert name in _lib.SIGNATURES


def test_signatures():
    # the dW entry: the bf16g entry's arguments without ldg (an fp32 g is dense); its query likewise
    res, args = _lib.SIGNATURES[DW]
    gres, gargs = _lib.SIGNATURES["grl_linear_bwd_weight_bf16g"]
    assert res == gres and list(args) == list(gargs[:3]) + list(gargs[4:])
    res, args = _lib.SIGNATURES[DW_QUERY]
    gres, gargs = _lib.SIGNATURES["grl_linear_bwd_weight_bf16g_workspace_query"]
    assert res == gres and list(args) == list(gargs[:3]) + list(gargs[4:])
    # the forward entry: grl_linear_fwd_ex's arguments with ldo behind out
    res, args = _lib.SIGNATURES[FWD]
    eres, eargs = _lib.SIGNATURES["grl_linear_fwd_ex"]
    assert res == eres and list(args) == list(eargs[:6]) + [_lib._c_i64] + list(eargs[6:])
    res, args = _lib.SIGNATURES[FWD_QUERY]
    assert res == _lib._c_size and len(args) == 9


def test_constants():
    assert 2 * M * K * C >= 1.6e10 > 2 * BELOW * K * C and M >= 16 and K % 16 == 0 and C % 4 == 0


@pytest.mark.parametrize("option", ["dw_bf16z_f32g", "linear_out_bf16"])
def test_the_options_round_trip_and_have_bounds(option, grl_option):
    default = _lib.get_option(option)
    assert default in (0, 1)
    for v in (0, 1):
        grl_option(option, v)
        assert _lib.get_option(option) == v
    for bad in (-1, 2):
        with pytest.raises(_lib.GrlError, match="outside"):
            _lib.set_option(option, bad)
    assert _lib.get_option(option) == 1  # a refused value changes nothing
    with _lib.options(**{option: 0}):
        assert _lib.get_option(option) == 0
    assert _lib.get_option(option) == 1


# ---- grl_linear_bwd_weight_bf16z ---------------------------------------------------
def dw_query(z=Z, ldz=K, g=G, m=M, k=K, c=C):
    return getattr(_lib.lib(), DW_QUERY)(z, ldz, g, m, k, c)


def dw_run(z=Z, ldz=K, g=G, dw=DWP, db=None, m=M, k=K, c=C, ws=None, ws_bytes=0):
    lib = _lib.lib()
    if ws_bytes == shared.SHORT:
        ws_bytes = lib.grl_linear_bwd_weight_workspace_size(m, k, c) - 1
        assert ws_bytes > 0
    rc = getattr(lib, DW)(z, ldz, g, dw, db, m, k, c, ws, ws_bytes, None)
    return rc, lib.grl_last_error()


def dw_size(m=M, k=K, c=C):
    return _lib.lib().grl_linear_bwd_weight_workspace_size(m, k, c)


def test_the_dw_entry_answers_the_shared_bad_call_table(grl_option):
    """Every row of the table the dW entries share, with the code the two bf16
    entries give (they agree on every row) and the entry's name in the message;
    the one row about ldg has no argument here (an fp32 g is dense)."""
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16z_f32g", 1)
    assert (M, K, C) == (shared.M, shared.K, shared.C)
    seen = 0
    for case, kw, expect in shared.DW_CASES:
        want = {expect[e] for e in shared.DW_ENTRIES[1:]}
        assert len(want) == 1, case  # the bf16 entries agree
        kw = dict(kw)
        if "ldg" in kw:
            if kw["ldg"] != 0:  # "ldg < C": no such argument
                assert case == "ldg < C"
                continue
            del kw["ldg"]  # (C == 0: the dense g's stride is C itself)
        rc, msg = dw_run(**kw)
        assert rc == want.pop(), (case, rc, msg)
        if rc != OK:
            assert DW.encode() + b":" in msg, (case, msg)
        seen += 1
    assert seen == len(shared.DW_CASES) - 1


def test_dw_argument_errors_carry_their_words(grl_option):
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16z_f32g", 1)
    name = DW.encode()
    for kw in ({"m": -1}, {"k": -4}, {"c": -4}):
        rc, msg = dw_run(**kw)
        assert rc == INVALID and b"negative" in msg and name in msg, kw
    rc, msg = dw_run(ldz=K - 4)
    assert rc == INVALID and b"ldz" in msg and name in msg
    for kw in ({"z": None}, {"g": None}, {"dw": None}, {"m": 0, "dw": None}):
        rc, msg = dw_run(**kw)
        assert rc == INVALID and b"NULL pointer" in msg and name in msg, kw
    rc, msg = dw_run(z=Z + 1)  # an odd bf16 address
    assert rc == INVALID and b"2-B aligned" in msg and name in msg


def test_dw_ineligible_calls_are_unsupported_and_eligible_ones_ask_for_the_workspace(grl_option):
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16z_f32g", 1)
    name = DW.encode()
    need = dw_size()
    assert dw_query() == need > 0
    for kw in ({}, {"ws": WS, "ws_bytes": need - 1}, {"ws": None, "ws_bytes": need}):
        rc, msg = dw_run(**kw)  # eligible: the next check is the workspace
        assert rc == WORKSPACE and name in msg, kw
    # one broken condition each: the flop floor, M >= 16 (above the floor), K % 4, C % 4, Z's 8 B (twice), ldz % 4,
    # g's 16 B (twice)
    for kw in ({"m": BELOW}, {"m": 12, "k": 32768, "c": 32768, "ldz": 32768}, {"k": K + 2, "ldz": K + 4}, {"c": C - 2},
               {"z": Z + 4}, {"z": Z + 2}, {"ldz": K + 2}, {"g": G + 8}, {"g": G + 4}):
        assert dw_query(**kw) == 0, kw
        rc, msg = dw_run(ws=WS, ws_bytes=1 << 40, **kw)
        assert rc == UNSUPPORTED and name in msg, kw
    # the three ways the issue names: the option, gemm_x6, the flop floor -- each names the option
    grl_option("dw_bf16z_f32g", 0)
    assert dw_query() == 0
    rc, msg = dw_run(ws=WS, ws_bytes=need)
    assert rc == UNSUPPORTED and b"dw_bf16z_f32g" in msg and name in msg
    grl_option("dw_bf16z_f32g", 1)
    assert dw_query() == need
    grl_option("gemm_x6", 0)  # the shape rule's own option
    assert dw_query() == 0
    rc, msg = dw_run(ws=WS, ws_bytes=need)
    assert rc == UNSUPPORTED and b"dw_bf16z_f32g" in msg and b"gemm_x6" in msg and name in msg
    grl_option("gemm_x6", 1)
    assert 2 * BELOW * K * C < 1.6e10 and dw_query(m=BELOW) == 0
    rc, msg = dw_run(m=BELOW, ws=WS, ws_bytes=need)
    assert rc == UNSUPPORTED and b"dw_bf16z_f32g" in msg and name in msg
    # the other entries' options do not reach this one
    grl_option("dw_bf16z", 0)
    grl_option("dw_bf16g", 0)
    assert dw_query() == need


def test_the_dw_query_is_the_fp32_entrys_workspace_size_where_eligible(grl_option):
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16z_f32g", 1)
    for m, k, c in ((M, K, C), (60001, 1400, 100), (250, 8192, 4096), (1_000_000, 512, 128), (1_000_000, 1792, 256),
                    (16, 32768, 16384)):
        assert 2 * m * k * c >= 1.6e10
        assert dw_query(m=m, k=k, c=c, ldz=k) == dw_size(m, k, c) > 0, (m, k, c)
    # emb2's floor at net_size 256 (K = 512, C = 128): 122,071 nodes
    assert dw_query(m=122_071, k=512, c=128, ldz=512) > 0 and dw_query(m=122_070, k=512, c=128, ldz=512) == 0
    # a strided Z: a column slice of a wider table on the 8 B grid
    assert dw_query(z=Z + 2 * 32, ldz=K + 64) == dw_size()
    assert dw_query(z=Z + 8, ldz=K + 4) == dw_size()


def test_the_dw_query_is_zero_on_bad_arguments():
    assert dw_query(z=None) == 0 and dw_query(g=None) == 0
    assert dw_query(m=0) == 0 and dw_query(m=-1) == 0
    assert dw_query(k=0, ldz=0) == 0 and dw_query(c=0) == 0
    assert dw_query(ldz=K - 4) == 0


# ---- grl_linear_fwd_to_bf16 ----------------------------------------------------------
def fwd_query(z=Z, ldz=None, w=W, out=OUT, ldo=None, m=M, k=K, c=C, pr=0):
    return getattr(_lib.lib(), FWD_QUERY)(z, k if ldz is None else ldz, w, out, c if ldo is None else ldo, m, k, c, pr)


def fwd_run(z=Z, ldz=None, w=W, layout=1, b=B, out=OUT, ldo=None, m=M, k=K, c=C, relu=1, pr=0, ws=None, ws_bytes=0):
    rc = getattr(_lib.lib(), FWD)(z, k if ldz is None else ldz, w, layout, b, out, c if ldo is None else ldo, m, k, c,
                                  relu, pr, ws, ws_bytes, None)
    return rc, _lib.lib().grl_last_error()


def fwd_size(m=M, k=K, c=C, pr=0):
    return _lib.lib().grl_linear_fwd_ex_workspace_size(m, k, c, pr)


def test_fwd_argument_errors_are_refused_on_the_host(grl_option):
    """grl_linear_fwd_bf16x's bad calls, then the three about out."""
    grl_option("linear_out_bf16", 1)
    grl_option("gemm_x6", 1)
    name = FWD.encode()
    for kw in ({"m": -1}, {"k": -16, "ldz": 0}, {"c": -4, "ldo": 0}, {"pr": -1}):
        rc, msg = fwd_run(**kw)
        assert rc == INVALID and b"negative" in msg and name in msg, kw
    rc, msg = fwd_run(ldz=K - 8)
    assert rc == INVALID and b"ldz" in msg and name in msg
    for layout in (-1, 2):
        rc, msg = fwd_run(layout=layout)
        assert rc == INVALID and b"w_layout" in msg and name in msg
    for kw in ({"z": None}, {"w": None}, {"out": None}):
        rc, msg = fwd_run(**kw)
        assert rc == INVALID and b"NULL pointer" in msg and name in msg, kw
    # M == 0 or C == 0: nothing to do, whatever the pointers
    assert fwd_run(m=0, z=None, w=None, out=None)[0] == OK
    assert fwd_run(c=0, z=None, w=None, out=None)[0] == OK
    # ... but the sizes and w_layout are checked first
    assert fwd_run(m=0, ldz=K - 8)[0] == INVALID and fwd_run(c=0, layout=3)[0] == INVALID
    # out: rows that overlap, an odd address; an odd ldo is well-formed and outside the path
    rc, msg = fwd_run(ldo=C - 2)
    assert rc == INVALID and b"ldo" in msg and name in msg
    assert fwd_run(m=0, ldo=C - 2)[0] == INVALID
    rc, msg = fwd_run(out=OUT + 1)
    assert rc == INVALID and b"2-B aligned" in msg and name in msg
    assert fwd_query(ldo=C + 1) == 0
    rc, msg = fwd_run(ldo=C + 1, ws=WS, ws_bytes=1 << 40)
    assert rc == UNSUPPORTED and b"ldo" in msg and name in msg


# one broken condition each: K % 16, C % 4, ldz % 4, Z off the 16 B grid, W off it, out on the 2 B grid but off
# the 4 B one, an odd ldo, (M, path_rows) below the floor (M itself, and a small M with a path_rows below it)
FWD_INELIGIBLE = ({"k": 1800}, {"c": 254}, {"ldz": K + 2}, {"z": Z + 8}, {"w": W + 8}, {"out": OUT + 2},
                  {"ldo": C + 3}, {"m": BELOW}, {"m": 100, "pr": BELOW})


def test_fwd_ineligible_calls_are_unsupported_and_eligible_ones_ask_for_the_workspace(grl_option):
    grl_option("linear_out_bf16", 1)
    grl_option("gemm_x6", 1)
    name = FWD.encode()
    need = fwd_size()
    assert fwd_query() == need > 0
    for kw in ({}, {"ws": WS, "ws_bytes": need - 1}, {"ws": None, "ws_bytes": need}, {"ws": WS + 8, "ws_bytes": need}):
        rc, msg = fwd_run(**kw)  # eligible: the next check is the workspace
        assert rc == WORKSPACE and name in msg, kw
    for kw in FWD_INELIGIBLE:
        assert fwd_query(**kw) == 0, kw
        rc, msg = fwd_run(ws=WS, ws_bytes=1 << 40, **kw)
        assert rc == UNSUPPORTED and name in msg, kw
    # the three ways the issue names: the option, gemm_x6, the flop floor (no path_rows) -- each names the option
    grl_option("linear_out_bf16", 0)
    assert fwd_query() == 0
    rc, msg = fwd_run(ws=WS, ws_bytes=need)
    assert rc == UNSUPPORTED and b"linear_out_bf16" in msg and name in msg
    grl_option("linear_out_bf16", 1)
    assert fwd_query() == need
    grl_option("gemm_x6", 0)  # the shape rule's own option
    assert fwd_query() == 0
    rc, msg = fwd_run(ws=WS, ws_bytes=need)
    assert rc == UNSUPPORTED and b"linear_out_bf16" in msg and b"gemm_x6" in msg and name in msg
    grl_option("gemm_x6", 1)
    assert fwd_query(m=BELOW) == 0
    rc, msg = fwd_run(m=BELOW, ws=WS, ws_bytes=need)
    assert rc == UNSUPPORTED and b"linear_out_bf16" in msg and name in msg
    # grl_linear_fwd_ex answers unchanged whatever the option: its size rule does not read it
    grl_option("linear_out_bf16", 0)
    assert fwd_size() == need and _lib.lib().grl_linear_fwd_path(M, K, C, 0) == 1


def test_the_fwd_query_is_the_fp32_entrys_workspace_size_where_eligible(grl_option):
    grl_option("linear_out_bf16", 1)
    grl_option("gemm_x6", 1)
    lib = _lib.lib()
    # (the data gradient of emb2 at 1M nodes: g [M, 128] x W [128, 512])
    for m, k, c, pr in ((M, K, C, 0), (1_000_000, 128, 512, 0), (1, 32, 8, 1 << 25), (300, 48, 40, 1 << 23),
                        (256, 16, 256, 1 << 23), (513, 64, 260, 1 << 23), (123_003, 128, 512, 0)):
        assert lib.grl_linear_fwd_path(m, k, c, pr) == 1
        assert fwd_query(m=m, k=k, c=c, pr=pr) == fwd_size(m, k, c, pr) == 3 * (-(-c // 256) * 256) * k * 2 + 256, \
            (m, k, c, pr)
    # a column slice of a wider bf16 table on the 4 B grid with an even row stride; a strided Z
    assert fwd_query(out=OUT + 2 * 32, ldo=C + 64) == fwd_size()
    assert fwd_query(out=OUT + 4, ldo=C + 2) == fwd_size()
    assert fwd_query(z=Z + 16, ldz=K + 4) == fwd_size()


def test_the_fwd_query_is_zero_on_bad_arguments():
    assert fwd_query(z=None) == 0 and fwd_query(w=None) == 0 and fwd_query(out=None) == 0
    assert fwd_query(m=0) == 0 and fwd_query(m=-1) == 0 and fwd_query(pr=-1) == 0
    assert fwd_query(k=0, ldz=0) == 0 and fwd_query(c=0, ldo=0) == 0
    assert fwd_query(ldz=K - 8) == 0 and fwd_query(ldo=C - 2) == 0
