"""CPU-only: the entries that share a host path answer the same bad calls the
same way.  grl_linear_bwd_weight, _bf16g and _bf16zg run through one host
function (linear.hip: linear_bwd_weight_run), grl_node_attention_fwd_rows and
_fwd_bf16kv_rows through one size / range check and one key-split helper
(attention.hip).  One table of bad calls goes through every entry of a family;
each must answer its own return code, recorded from the library before the
host paths were folded, and name itself in the message.  Every call here is
decided on the host: no pointer is dereferenced and no device work is issued.
"""
import pytest

from grl import _lib

OK, INVALID, WORKSPACE = _lib.GRL_OK, _lib.GRL_E_INVALID, _lib.GRL_E_WORKSPACE

# ---- the dW entries --------------------------------------------------------------
M, K, C = 20011, 1792, 256  # inside the split-bf16 dW rule: 2 M K C >= 1.6e10, M >= 16, K % 4 == C % 4 == 0
Z, G, DW, WS = 0x10000, 0x20000, 0x30000, 0x50000  # never dereferenced
SHORT = "one byte short"  # a workspace of grl_linear_bwd_weight_workspace_size(M, K, C) - 1 bytes

DW_ENTRIES = ("grl_linear_bwd_weight", "grl_linear_bwd_weight_bf16g", "grl_linear_bwd_weight_bf16zg")


def ALL(code):
    return dict.fromkeys(DW_ENTRIES, code)


def BF16(code):
    return dict.fromkeys(DW_ENTRIES[1:], code)


# (case, arguments that differ from a good call, {entry: code}); an entry without the argument is left out
DW_CASES = [
    ("negative M", {"m": -1}, ALL(INVALID)),
    ("negative K", {"k": -4}, ALL(INVALID)),
    ("negative C", {"c": -4}, ALL(INVALID)),
    ("ldz < K", {"ldz": K - 4}, ALL(INVALID)),
    ("ldg < C", {"ldg": C - 4}, BF16(INVALID)),  # the fp32 entry's g is dense: no ldg
    ("NULL dW with M == 0", {"m": 0, "dw": None}, ALL(INVALID)),
    ("NULL Z", {"z": None}, ALL(INVALID)),
    ("NULL g", {"g": None}, ALL(INVALID)),
    ("NULL dW", {"dw": None}, ALL(INVALID)),
    ("no workspace", {}, ALL(WORKSPACE)),
    ("workspace one byte short", {"ws": WS, "ws_bytes": SHORT}, ALL(WORKSPACE)),
    ("NULL workspace of the full size", {"ws_bytes": 1 << 40}, ALL(WORKSPACE)),
    ("K == 0, NULL pointers", {"k": 0, "ldz": 0, "z": None, "g": None, "dw": None}, ALL(OK)),
    ("C == 0, NULL pointers", {"c": 0, "ldg": 0, "z": None, "g": None, "dw": None}, ALL(OK)),
]


def run_dw(entry, z=Z, ldz=K, g=G, ldg=None, dw=DW, db=None, m=M, k=K, c=C, ws=None, ws_bytes=0):
    lib = _lib.lib()
    if ws_bytes == SHORT:
        ws_bytes = lib.grl_linear_bwd_weight_workspace_size(m, k, c) - 1
        assert ws_bytes > 0
    if entry == "grl_linear_bwd_weight":  # (Z, ldz, g, relu_out, ...): g dense (no ldg to pass), an optional mask
        rc = getattr(lib, entry)(z, ldz, g, None, dw, db, m, k, c, ws, ws_bytes, None)
    else:
        rc = getattr(lib, entry)(z, ldz, g, c if ldg is None else ldg, dw, db, m, k, c, ws, ws_bytes, None)
    return rc, lib.grl_last_error()


@pytest.mark.parametrize("entry", DW_ENTRIES)
def test_the_dw_entries_answer_the_same_bad_calls(entry, grl_option):
    grl_option("gemm_x6", 1)
    grl_option("dw_bf16g", 1)
    grl_option("dw_bf16z", 1)
    seen = 0
    for case, kw, expect in DW_CASES:
        if entry not in expect:
            continue
        rc, msg = run_dw(entry, **kw)
        assert rc == expect[entry], (entry, case, rc, msg)
        if rc != OK:
            assert entry.encode() + b":" in msg, (entry, case, msg)
        seen += 1
    assert seen == len(DW_CASES) - (entry == DW_ENTRIES[0])  # the fp32 entry skips "ldg < C" alone


# ---- the attention forward entries -------------------------------------------------
N = 300
Q_, K_, H_, V_, GAMMA, OUT, ONORM, RMAX, RSUM = (0x10000 * i for i in range(1, 10))  # never dereferenced
# entry -> the name its messages and its trace range carry
ATTN_ENTRIES = {"grl_node_attention_fwd_rows": b"grl_node_attention_fwd:",
                "grl_node_attention_fwd_bf16kv_rows": b"grl_node_attention_fwd_bf16kv:"}
ATTN_CASES = [
    ("negative q_begin", {"q0": -1}, INVALID),
    ("q_end past N", {"q1": N + 1}, INVALID),
    ("q_begin past q_end", {"q0": 200, "q1": 100}, INVALID),
    ("an empty range past N", {"q0": N + 1, "q1": N + 1}, INVALID),
    ("row_max without row_sum", {"rsum": None}, INVALID),
    ("row_sum without row_max", {"rmax": None}, INVALID),
    ("q_begin == q_end, NULL tables", {"q0": 100, "q1": 100, "k": None, "h": None}, OK),
    ("q_begin == q_end == N, NULL tables", {"q0": N, "q1": N, "k": None, "h": None}, OK),
]


def run_attn(entry, q=Q_, k=K_, h=H_, v=V_, gamma=GAMMA, out=OUT, onorm=ONORM, rmax=RMAX, rsum=RSUM, B=2, dk=16,
             dv=128, q0=0, q1=N):
    lib = _lib.lib()
    rc = getattr(lib, entry)(q, k, h, v, gamma, out, onorm, rmax, rsum, B, N, dk, dv, q0, q1, None, 0, None)
    return rc, lib.grl_last_error()


@pytest.mark.parametrize("entry", sorted(ATTN_ENTRIES))
def test_the_attention_forward_entries_answer_the_same_bad_calls(entry, grl_option):
    grl_option("attn_x6", 1)
    for case, kw, expect in ATTN_CASES:
        rc, msg = run_attn(entry, **kw)
        assert rc == expect, (entry, case, rc, msg)
        if rc != OK:
            assert ATTN_ENTRIES[entry] in msg, (entry, case, msg)
    # the words the two share
    assert b"outside" in run_attn(entry, q0=-1)[1]
    assert b"both or none" in run_attn(entry, rmax=None)[1]
