"""CPU-only: the entries that share a host path answer the same bad calls the
same way.  grl_linear_bwd_weight, _bf16g and _bf16zg run through one host
function (linear.hip: linear_bwd_weight_run), grl_node_attention_fwd_rows and
_fwd_bf16kv_rows through one size / range check and one key-split helper
(attention.hip).  One table of bad calls goes through every entry of a family;
each must answer its own return code, recorded from the library before the
host paths were folded, and name itself in the message.  Every call here is
decided on the host: no pointer is dereferenced and no device work is issued.

The GraphConv layer's entries likewise (graphconv.hip): the seven
grl_graphconv_fwd* entries run through graphconv_fwd_run, the two
grl_graphconv_bwd_data* entries through graphconv_bwd_data_run, and every
workspace query answers from the same fwd_chain_layout the entries take their
pointers from.  QUERY_TABLE holds what the six queries answered before the
fold, as numbers: the layout struct must give the old sums.
"""
import ctypes

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


# ---- the GraphConv forward entries ---------------------------------------------------
UNSUPPORTED = _lib.GRL_E_UNSUPPORTED
ROWS, TYPES, GF, GC = 20011, 6, 256, 256  # above the x6 GEMM's flop floor (test_abi_graphconv_bf16_bwd.py): one kernel
BELOW = 17438                             # below it
GX, GW, GB, GOUT, GZ, GWS = 0x10000, 0x20000, 0x30000, 0x40000, 0x60000, 0x80000  # never dereferenced

# entry -> (takes ldo: a bf16 out, its Z: None / "fp32" / "bf16", its workspace query)
FWD_ENTRIES = {
    "grl_graphconv_fwd": (False, None, "grl_graphconv_fwd_workspace_query"),
    "grl_graphconv_fwd_bf16": (False, None, "grl_graphconv_fwd_bf16_workspace_query"),
    "grl_graphconv_fwd_bf16_to_bf16": (True, None, "grl_graphconv_fwd_bf16_to_bf16_workspace_query"),
    "grl_graphconv_fwd_train": (False, "fp32", None),
    "grl_graphconv_fwd_train_bf16": (False, "fp32", None),
    "grl_graphconv_fwd_train_bf16_to_bf16": (True, "fp32", "grl_graphconv_fwd_bf16_to_bf16_workspace_query"),
    "grl_graphconv_fwd_train_bf16_z16": (True, "bf16", "grl_graphconv_fwd_train_bf16_z16_workspace_query"),
}


def FWD(code, ldo=None, z=None):
    """{entry: code} over the forward entries (with a bf16 out: ldo; that write Z: z=True; a bf16 Z: z="bf16")."""
    return {e: code for e, (has_ldo, zkind, _) in FWD_ENTRIES.items()
            if (ldo is None or has_ldo == ldo) and (z is None or (zkind == z if isinstance(z, str) else bool(zkind) == z))}


# the entries that refuse a short workspace themselves, before any device work: those over a bf16 table that
# place something of their own in it.  (The fp32-out training entries hand theirs to the linear after the SpMM
# is launched, and grl_graphconv_fwd works in row chunks: left out but for the cases FP32_INFER lists.)
REFUSE = ("grl_graphconv_fwd_bf16", "grl_graphconv_fwd_bf16_to_bf16", "grl_graphconv_fwd_train_bf16_to_bf16",
          "grl_graphconv_fwd_train_bf16_z16")
FP32_INFER = "grl_graphconv_fwd"
HEAVY = {"split_heavy": 1}  # a graph with a heavy-row split plan: no one kernel, no row chunks


def ONLY(entries, code):
    return dict.fromkeys((entries,) if isinstance(entries, str) else entries, code)


# (case, arguments that differ from a good call, {entry: code}); an entry without the argument is left out
FWD_CASES = [
    ("NULL graph", {"g": None}, FWD(INVALID)),
    ("num_types 0", {"g": {"num_types": 0}}, FWD(INVALID)),
    ("num_types 64", {"g": {"num_types": 64}}, FWD(INVALID)),
    ("F == 0", {"f": 0}, FWD(INVALID)),
    ("ldx < F", {"ldx": GF - 4}, FWD(INVALID)),
    ("NULL X", {"x": None}, FWD(INVALID)),
    ("NULL W", {"w": None}, FWD(INVALID)),
    ("NULL out", {"out": None}, FWD(INVALID)),
    ("NULL Z", {"z": None}, FWD(INVALID, z=True)),
    ("C == 0", {"c": 0}, FWD(INVALID)),
    ("segments * F past int32", {"g": {"num_types": 63}, "f": 1 << 25, "ldx": 1 << 25}, FWD(INVALID)),
    ("workspace not 16-B aligned", {"ws": GWS + 8, "ws_bytes": 1 << 40}, FWD(INVALID)),
    ("ldo < C", {"ldo": GC - 2}, FWD(INVALID, ldo=True)),
    ("odd X", {"x": GX + 1}, FWD(INVALID, ldo=True)),  # (the fp32-out entries make no 2-B check: not decided on the host)
    ("odd out", {"out": GOUT + 1}, FWD(INVALID, ldo=True)),
    ("odd Z", {"z": GZ + 1}, FWD(INVALID, z="bf16")),
    ("no rows, NULL tables", {"g": {"num_rows": 0}, "x": None, "w": None, "out": None, "z": None}, FWD(OK)),
    ("no rows, ldo < C", {"g": {"num_rows": 0}, "ldo": GC - 2}, FWD(INVALID, ldo=True)),  # refused before the return
    ("no workspace", {}, {**ONLY(REFUSE, WORKSPACE), **ONLY(FP32_INFER, WORKSPACE)}),
    ("workspace one byte short", {"ws": GWS, "ws_bytes": SHORT}, ONLY(REFUSE, WORKSPACE)),
    ("no workspace, two kernels", {"fused": 0}, {**ONLY(REFUSE, WORKSPACE), **ONLY(FP32_INFER, WORKSPACE)}),
    ("workspace one byte short, two kernels", {"fused": 0, "ws": GWS, "ws_bytes": SHORT}, ONLY(REFUSE, WORKSPACE)),
    ("a split plan, one byte short", {"g": HEAVY, "ws": GWS, "ws_bytes": SHORT},
     {**ONLY(REFUSE, WORKSPACE), **ONLY(FP32_INFER, WORKSPACE)}),
    ("below the x6 floor, one byte short", {"g": {"num_rows": BELOW}, "ws": GWS, "ws_bytes": SHORT},
     {**ONLY(REFUSE, WORKSPACE), **ONLY(FP32_INFER, WORKSPACE)}),
]


def gc_graph(num_rows=ROWS, num_types=TYPES, has_self=1, split_heavy=0):
    g = _lib.GrlTypedCsr()
    g.num_rows, g.num_types, g.has_self = num_rows, num_types, has_self
    g.rowptr = 0x3000  # non-NULL, never dereferenced
    if split_heavy:  # the plan is host memory the library reads num_heavy from; kept alive on the graph
        g._plan = _lib.GrlSplitPlan(num_heavy=split_heavy)
        g.split = ctypes.pointer(g._plan)
    return g


def fwd_query(entry, g, x=GX, ldx=GF, f=GF, w=GW, c=GC, out=GOUT, ldo=None, z=GZ):
    """The entry's workspace query.  grl_graphconv_fwd_train_bf16_to_bf16 has none of its own: where it takes one
    kernel its bytes are the inference entry's (W's planes); its chain keeps Z out of the workspace, so there it is
    the linear's own workspace behind the linear's 256-B aligned fp32 [num_rows, C] (grl.ops.graph_conv_fwd_train)."""
    lib = _lib.lib()
    has_ldo, zkind, query = FWD_ENTRIES[entry]
    args = [ctypes.byref(g), x, ldx, f, w, c] + ([out, c if ldo is None else ldo] if has_ldo else [])
    q = getattr(lib, query)(*args, *([z] if zkind == "bf16" else []))
    if entry == "grl_graphconv_fwd_train_bf16_to_bf16" and q >= g.num_rows * (g.num_types + g.has_self) * f * 4:
        k = (g.num_types + g.has_self) * f
        q = (g.num_rows * c * 4 + 255) // 256 * 256 + lib.grl_linear_fwd_ex_workspace_size(g.num_rows, k, c, 0)
    return q


def run_fwd(entry, g={}, x=GX, ldx=GF, f=GF, w=GW, c=GC, out=GOUT, ldo=None, z=GZ, ws=None, ws_bytes=0):
    lib = _lib.lib()
    has_ldo, zkind, _ = FWD_ENTRIES[entry]
    g = None if g is None else gc_graph(**g)
    if ws_bytes == SHORT:
        ws_bytes = fwd_query(entry, g, x, ldx, f, w, c, out, ldo, z) - 1
        assert ws_bytes > 0
    args = [None if g is None else ctypes.byref(g), x, ldx, f, w, GB, c, 1, out]
    args += ([c if ldo is None else ldo] if has_ldo else []) + ([z] if zkind else [])
    rc = getattr(lib, entry)(*args, None, ws, ws_bytes, None)
    return rc, lib.grl_last_error()


@pytest.mark.parametrize("entry", sorted(FWD_ENTRIES))
def test_the_graphconv_forward_entries_answer_the_same_bad_calls(entry, grl_option):
    seen = 0
    for case, kw, expect in FWD_CASES:
        if entry not in expect:
            continue
        kw = dict(kw)
        grl_option("graphconv_fused", kw.pop("fused", 1))
        rc, msg = run_fwd(entry, **kw)
        assert rc == expect[entry], (entry, case, rc, msg)
        if rc != OK:
            assert entry.encode() + b":" in msg, (entry, case, msg)
        if rc == WORKSPACE:
            assert b"workspace" in msg, (entry, case, msg)
        seen += 1
    has_ldo, zkind, _ = FWD_ENTRIES[entry]
    assert seen == 12 + 4 * has_ldo + bool(zkind) + (zkind == "bf16") + 6 * (entry in REFUSE) + 4 * (entry == FP32_INFER)
    if entry == FP32_INFER:  # the words its callers match
        assert b"split plan" in run_fwd(entry, g=HEAVY, ws=GWS, ws_bytes=SHORT)[1]


# ---- the GraphConv data-gradient entries --------------------------------------------------
BWD_ENTRIES = ("grl_graphconv_bwd_data", "grl_graphconv_bwd_data_bf16")
BWD_ONE = 7 * 256 * 1536 + 256  # W's planes + the status word: what both queries answer for the good call
# (case, arguments that differ from a good call, (the fp32 entry's code, the bf16 entry's); None: no such argument)
BWD_CASES = [
    ("NULL graph", {"g": None}, (INVALID, INVALID)),
    ("num_types 0", {"g": {"num_types": 0}}, (INVALID, INVALID)),
    ("g_rows past num_rows", {"g_rows": ROWS + 1}, (INVALID, INVALID)),
    ("NULL G with rows to read", {"G": None, "g_rows": 1}, (INVALID, INVALID)),  # a NULL G is an empty shard's only
    ("NULL dX", {"dX": None}, (INVALID, INVALID)),
    ("ldg < C", {"ldg": GC - 4}, (INVALID, INVALID)),
    ("lddx < F", {"lddx": GF - 2}, (None, INVALID)),
    ("no rows, lddx < F", {"g": {"num_rows": 0}, "lddx": GF - 2}, (None, INVALID)),  # refused before the return
    ("odd dX", {"dX": 0x4001}, (WORKSPACE, INVALID)),    # fp32: dX's address is not looked at; the workspace is next
    ("odd G", {"G": 0x1001}, (UNSUPPORTED, INVALID)),    # fp32: outside the rule (G rows 16 B-aligned)
    ("G_agg not 16-B aligned", {"G_agg": 0x7008}, (WORKSPACE, INVALID)),  # fp32: no such check
    ("no rows", {"g": {"num_rows": 0}}, (OK, OK)),
    ("below the x6 floor", {"g": {"num_rows": BELOW}}, (UNSUPPORTED, UNSUPPORTED)),
    ("graphconv_bwd_bf16 off", {"bwd_bf16": 0}, (WORKSPACE, UNSUPPORTED)),
    ("no workspace", {}, (WORKSPACE, WORKSPACE)),
    ("workspace not 16-B aligned", {"ws": 0x8008, "ws_bytes": BWD_ONE}, (WORKSPACE, WORKSPACE)),
    ("workspace one byte short", {"ws": 0x8000, "ws_bytes": BWD_ONE - 1}, (WORKSPACE, WORKSPACE)),
]
BWD_WORDS = [("NULL dX", b"NULL pointer"), ("lddx < F", b"lddx"), ("ldg < C", b"ldg"), ("g_rows past num_rows", b"g_rows"),
             ("num_types 0", b"num_types"), ("odd dX", b"2-B aligned"), ("graphconv_bwd_bf16 off", b"graphconv_bwd_bf16")]


def run_bwd(entry, g={}, G=0x1000, ldg=GC, dX=0x4000, lddx=GF, g_rows=0, G_agg=None, ws=None, ws_bytes=0):
    lib = _lib.lib()
    g = None if g is None else ctypes.byref(gc_graph(**g))
    args = [g, None, G, ldg, g_rows, GC, GW, GF, dX] + ([lddx] if entry.endswith("_bf16") else [])
    rc = getattr(lib, entry)(*args, G_agg, None, ws, ws_bytes, None)
    return rc, lib.grl_last_error()


@pytest.mark.parametrize("entry", BWD_ENTRIES)
def test_the_graphconv_data_gradient_entries_answer_the_same_bad_calls(entry, grl_option):
    bf16 = entry.endswith("_bf16")
    msgs = {}
    for case, kw, expect in BWD_CASES:
        if expect[bf16] is None:
            continue
        kw = dict(kw)
        grl_option("graphconv_bwd_bf16", kw.pop("bwd_bf16", 1))
        rc, msg = run_bwd(entry, **kw)
        assert rc == expect[bf16], (entry, case, rc, msg)
        if rc != OK:
            assert entry.encode() + b":" in msg, (entry, case, msg)
        msgs[case] = (rc, msg)
    assert len(msgs) == len(BWD_CASES) - (0 if bf16 else 2)
    for case, word in BWD_WORDS:  # the words of the checks an entry makes
        if case in msgs and (msgs[case][0] == INVALID or (bf16 and case == "graphconv_bwd_bf16 off")):
            assert word in msgs[case][1], (entry, case, msgs[case])


# ---- the six workspace queries, against the numbers they gave before the fold --------------
QUERIES = ("grl_graphconv_fwd_workspace_query", "grl_graphconv_fwd_bf16_workspace_query",
           "grl_graphconv_fwd_bf16_to_bf16_workspace_query", "grl_graphconv_fwd_train_bf16_z16_workspace_query",
           "grl_graphconv_bwd_data_workspace_query", "grl_graphconv_bwd_data_bf16_workspace_query")


def query_values(rows, c, f, xoff, ooff, zoff, fused):
    """The six queries for a graph of `rows` rows (6 types and the self term), widths c and f, the table / gradient
    xoff bytes, out / dX ooff bytes and Z zoff bytes off a 64 KiB boundary, rows c / f apart.  (The forward gathers f
    columns into c; the data gradient c into f.)"""
    lib = _lib.lib()
    _lib.set_option("graphconv_fused", fused)
    g = ctypes.byref(gc_graph(num_rows=rows))
    x, out, z = GX + xoff, GOUT + ooff, GZ + zoff
    return (lib.grl_graphconv_fwd_workspace_query(g, x, f, f, GW, c),
            lib.grl_graphconv_fwd_bf16_workspace_query(g, x, f, f, GW, c),
            lib.grl_graphconv_fwd_bf16_to_bf16_workspace_query(g, x, f, f, GW, c, out, c),
            lib.grl_graphconv_fwd_train_bf16_z16_workspace_query(g, x, f, f, GW, c, out, c, z),
            lib.grl_graphconv_bwd_data_workspace_query(g, x, c, c, GW, f),
            lib.grl_graphconv_bwd_data_bf16_workspace_query(g, x, c, c, GW, f, out, f))


# (rows, C, F, xoff, ooff, zoff, graphconv_fused): the answers of QUERIES, in that order
QUERY_TABLE = [
    ((0, 256, 256, 0, 0, 0, 1), (0, 0, 0, 0, 0, 0)),
    ((300, 32, 64, 0, 0, 0, 1), (1075456, 1075456, 1113856, 1113856, 0, 0)),
    ((300, 32, 256, 0, 0, 0, 1), (4301056, 4301056, 4339456, 4339456, 0, 0)),
    ((300, 64, 64, 0, 0, 0, 1), (1613056, 1613056, 1689856, 1689856, 0, 0)),
    ((300, 64, 256, 0, 0, 0, 1), (6451456, 6451456, 6528256, 6528256, 0, 0)),
    ((300, 256, 64, 0, 0, 0, 1), (4838656, 4838656, 5145856, 5145856, 0, 0)),
    ((300, 256, 256, 0, 0, 0, 1), (19353856, 19353856, 19661056, 19661056, 0, 0)),
    ((300, 512, 64, 0, 0, 0, 1), (9139456, 9139456, 9753856, 9753856, 0, 0)),
    ((300, 512, 256, 0, 0, 0, 1), (36557056, 36557056, 37171456, 37171456, 0, 0)),
    ((17438, 32, 64, 0, 0, 0, 1), (46873600, 46873600, 49105664, 49105664, 0, 0)),
    ((17438, 32, 256, 0, 0, 0, 1), (142852352, 142852352, 145084416, 145084416, 0, 0)),
    ((17438, 64, 64, 0, 0, 0, 1), (62498048, 62498048, 66962176, 66962176, 0, 0)),
    ((17438, 64, 256, 0, 0, 0, 1), (160708864, 160708864, 165172992, 165172992, 0, 0)),
    ((17438, 256, 64, 0, 0, 0, 1), (31248896, 31248896, 49105408, 49105408, 0, 0)),
    ((17438, 256, 256, 0, 0, 0, 1), (124995584, 124995584, 142852096, 142852096, 0, 0)),
    ((17438, 512, 64, 0, 0, 0, 1), (31248896, 31248896, 66961920, 66961920, 0, 0)),
    ((17438, 512, 256, 0, 0, 0, 1), (5505280, 5505280, 5505280, 5505280, 5505280, 5505280)),
    ((20011, 32, 64, 0, 0, 0, 1), (53789824, 53789824, 56351360, 56351360, 0, 0)),
    ((20011, 32, 256, 0, 0, 0, 1), (161368960, 161368960, 163930496, 163930496, 0, 0)),
    ((20011, 64, 64, 0, 0, 0, 1), (71719680, 71719680, 76842496, 76842496, 0, 0)),
    ((20011, 64, 256, 0, 0, 0, 1), (179298816, 179298816, 184421632, 184421632, 0, 0)),
    ((20011, 256, 64, 0, 0, 0, 1), (35859712, 35859712, 56350976, 56350976, 0, 0)),
    ((20011, 256, 256, 0, 0, 0, 1), (2752768, 2752768, 2752768, 2752768, 2752768, 2752768)),
    ((20011, 512, 64, 0, 0, 0, 1), (35859712, 35859712, 76842240, 76842240, 0, 0)),
    ((20011, 512, 256, 0, 0, 0, 1), (5505280, 5505280, 5505280, 5505280, 5505280, 5505280)),
    ((20011, 256, 256, 4, 0, 0, 1), (146191616, 146191616, 166682880, 166682880, 0, 0)),
    ((20011, 256, 256, 8, 0, 0, 1), (146191616, 2752768, 2752768, 2752768, 0, 2752768)),
    ((20011, 256, 256, 0, 2, 0, 1), (2752768, 2752768, 166682880, 166682880, 2752768, 0)),
    ((20011, 256, 256, 0, 0, 2, 1), (2752768, 2752768, 2752768, 166682880, 2752768, 2752768)),
    ((20011, 256, 256, 0, 0, 8, 1), (2752768, 2752768, 2752768, 2752768, 2752768, 2752768)),
    ((20011, 256, 256, 0, 0, 0, 0), (146191616, 146191616, 166682880, 166682880, 0, 0)),
    ((20011, 512, 64, 0, 0, 0, 0), (35859712, 35859712, 76842240, 76842240, 0, 0)),
    ((20011, 32, 256, 0, 0, 0, 0), (161368960, 161368960, 163930496, 163930496, 0, 0)),
    ((20011, 64, 64, 0, 0, 0, 0), (71719680, 71719680, 76842496, 76842496, 0, 0)),
    ((300, 32, 64, 0, 0, 0, 0), (1075456, 1075456, 1113856, 1113856, 0, 0)),
    ((17438, 256, 256, 0, 0, 0, 0), (124995584, 124995584, 142852096, 142852096, 0, 0)),
    ((20011, 256, 256, 4, 0, 0, 0), (146191616, 146191616, 166682880, 166682880, 0, 0)),
    ((20011, 256, 256, 0, 2, 0, 0), (146191616, 146191616, 166682880, 166682880, 0, 0)),
    ((20011, 256, 256, 0, 0, 2, 0), (146191616, 146191616, 166682880, 166682880, 0, 0)),
]


def test_the_workspace_queries_answer_the_numbers_from_before_the_fold(grl_option):
    grl_option("graphconv_fused", 1)  # (restored afterwards; query_values sets it per row)
    grl_option("graphconv_bwd_bf16", 1)
    assert len(QUERY_TABLE) >= 36
    assert {r[0][0] for r in QUERY_TABLE} == {0, 300, 17438, 20011} and {r[0][6] for r in QUERY_TABLE} == {0, 1}
    for args, want in QUERY_TABLE:
        assert query_values(*args) == want, (args, dict(zip(QUERIES, query_values(*args))))
