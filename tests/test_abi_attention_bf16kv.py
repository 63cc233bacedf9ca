"""CPU-only: the attention forward over key / value tables stored as bf16
(grl_node_attention_fwd_bf16kv_rows, its _path rule and its workspace query):
exported, declared in include/grl.h and bound with the declared arity; the
_path truth table (dk in {16, 32}, dv in {32, 64, 128, 256}, attn_x6 = 1);
every argument error that is decided on the host.  No pointer is dereferenced
and no device work is issued.

And the numerical argument of DESIGN.md §4.22 on the numpy model of the plane
products (x6_isolate): for an a that is one bf16 plane and a split b, the three
products (0,2), (0,1), (0,0) give the bits of all six on an accumulator that
starts at +0."""
import os
import re

import numpy as np
import pytest

import x6_isolate as xi
from grl import _lib

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "grl.h")
PATH = "grl_node_attention_fwd_bf16kv_path"
SIZE = "grl_node_attention_fwd_bf16kv_workspace_size"
ROWS = "grl_node_attention_fwd_bf16kv_rows"
FP32_ROWS = "grl_node_attention_fwd_rows"

Q, K16, H16, V, GAMMA, OUT, ONORM, RMAX, RSUM = (0x10000 * i for i in range(1, 10))  # never dereferenced


def header_text():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def declared_arity(name):
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", header_text())
    assert m, name
    return len([p for p in m.group(1).split(",") if p.strip()])


def path(dk, dv, B=1, N=1000):
    return getattr(_lib.lib(), PATH)(B, N, dk, dv)


def run(q=Q, k=K16, h=H16, v=V, gamma=GAMMA, out=OUT, onorm=ONORM, rmax=RMAX, rsum=RSUM, B=2, N=300, dk=16, dv=128,
        q0=0, q1=None, ws=None, ws_bytes=0):
    rc = getattr(_lib.lib(), ROWS)(q, k, h, v, gamma, out, onorm, rmax, rsum, B, N, dk, dv, q0,
                                   N if q1 is None else q1, ws, ws_bytes, None)
    return rc, _lib.lib().grl_last_error()


@pytest.mark.parametrize("name", [PATH, SIZE, ROWS])
def test_symbols_are_exported_declared_and_bound(name):
    assert hasattr(_lib.lib(), name)
    assert name in _lib.SIGNATURES
    assert declared_arity(name) == len(_lib.SIGNATURES[name][1])


def test_signatures_relate_to_the_fp32_entrys():
    assert _lib.SIGNATURES[ROWS] == _lib.SIGNATURES[FP32_ROWS]  # K and H pointers either way
    assert _lib.SIGNATURES[SIZE] == _lib.SIGNATURES["grl_node_attention_workspace_size"]
    res, args = _lib.SIGNATURES[PATH]
    assert res == _lib._c_i32 and list(args) == list(_lib.SIGNATURES[SIZE][1])


def test_path_truth_table(grl_option):
    grl_option("attn_x6", 1)
    for dk in (16, 32):
        for dv in (32, 64, 128, 256):
            assert path(dk, dv) == 1, (dk, dv)
            assert path(dk, dv, B=64, N=74) == 1  # no row threshold
    for dk in (0, 8, 9, 64):
        assert path(dk, 128) == 0, dk
    for dv in (1, 96, 97, 100, 512):
        assert path(16, dv) == 0, dv
    grl_option("attn_x6", 0)
    for dk in (16, 32):
        for dv in (32, 64, 128, 256):
            assert path(dk, dv) == 0, (dk, dv)
    grl_option("attn_x6", 1)
    assert path(16, 128) == 1


def test_the_workspace_query_is_zero_without_a_path(grl_option):
    size = getattr(_lib.lib(), SIZE)
    grl_option("attn_x6", 1)
    assert size(0, 100, 16, 128) == 0 and size(1, 0, 16, 128) == 0 and size(-1, 100, 16, 128) == 0
    assert size(1, 1000, 9, 128) == 0 and size(1, 1000, 16, 100) == 0
    grl_option("attn_x6", 0)
    assert size(1, 1000, 16, 128) == 0


def test_argument_errors_are_refused_on_the_host(grl_option):
    grl_option("attn_x6", 1)
    name = b"grl_node_attention_fwd_bf16kv"
    for kw in ({"B": -1}, {"N": -1, "q1": 0}):
        rc, msg = run(**kw)
        assert rc == _lib.GRL_E_INVALID and b"negative" in msg and name in msg, kw
    for kw in ({"q0": -1}, {"q1": 301}, {"q0": 200, "q1": 100}, {"q0": 301, "q1": 301}):  # a range outside [0, N]
        rc, msg = run(**kw)
        assert rc == _lib.GRL_E_INVALID and b"outside" in msg and name in msg, kw
    for kw in ({"k": None}, {"h": None}, {"q": None}, {"v": None}, {"gamma": None}, {"out": None}):
        rc, msg = run(**kw)
        assert rc == _lib.GRL_E_INVALID and b"NULL pointer" in msg and name in msg, kw
    for kw in ({"rmax": None}, {"rsum": None}):  # the statistics: both or none
        rc, msg = run(**kw)
        assert rc == _lib.GRL_E_INVALID and b"both or none" in msg and name in msg, kw
    rc, msg = run(dk=65)
    assert rc == _lib.GRL_E_INVALID and name in msg
    rc, msg = run(dv=0)
    assert rc == _lib.GRL_E_INVALID and name in msg


def test_empty_cases_are_ok_whatever_the_pointers():
    assert run(B=0, k=None, h=None)[0] == _lib.GRL_OK
    assert run(N=0, q1=0, k=None, h=None)[0] == _lib.GRL_OK
    assert run(q0=100, q1=100, k=None, h=None)[0] == _lib.GRL_OK


def test_calls_without_a_path_are_unsupported(grl_option):
    grl_option("attn_x6", 1)
    name = b"grl_node_attention_fwd_bf16kv"
    for kw in ({"dk": 9, "dv": 100}, {"dv": 96}, {"dk": 8}, {"dk": 64}, {"dk": 0, "q": None, "k": None}):
        rc, msg = run(**kw)
        assert rc == _lib.GRL_E_UNSUPPORTED and name in msg, kw
    for kw in ({"k": K16 + 2}, {"h": H16 + 2}, {"k": K16 + 8}, {"h": H16 + 8}):  # not 16 B-aligned
        rc, msg = run(**kw)
        assert rc == _lib.GRL_E_UNSUPPORTED and b"16 B-aligned" in msg and name in msg, kw
    grl_option("attn_x6", 0)
    rc, msg = run()
    assert rc == _lib.GRL_E_UNSUPPORTED and b"attn_x6" in msg


# ---- what stays float32 ----------------------------------------------------------
def test_the_sharded_op_and_the_backward_refuse_bf16_tables():
    """sharded_node_attention gathers K and H and runs the ranged fp32 backward
    on them, and node_attention_backward hands its tensors to fp32 kernels:
    both refuse anything but float32 before any work (no graph, no device)."""
    import torch

    from grl.dist import sharded_node_attention
    from grl.ops import node_attention_backward

    Q, K = torch.zeros(1, 8, 16), torch.zeros(1, 8, 16)
    H, V, gamma = torch.zeros(1, 8, 32), torch.zeros(1, 8, 32), torch.zeros(32)
    b16 = torch.bfloat16
    for args in ((Q, K.to(b16), H.to(b16), V, gamma), (Q, K.to(b16), H, V, gamma), (Q, K, H.to(b16), V, gamma),
                 (Q.to(b16), K, H, V, gamma), (Q, K, H, V.to(b16), gamma)):
        with pytest.raises(_lib.GrlError, match="sharded_node_attention.*must be float32"):
            sharded_node_attention(*args, None)
    stats = (torch.zeros(1, 8, 32), torch.zeros(1, 8), torch.ones(1, 8), torch.zeros(1, 8, 32))
    for q, k, h in ((Q, K.to(b16), H.to(b16)), (Q, K.to(b16), H), (Q, K, H.to(b16)), (Q.to(b16), K, H)):
        with pytest.raises(_lib.GrlError, match="attention backward.*must be float32"):
            node_attention_backward(q, k, h, gamma, *stats)


# ---- the numerical argument ----------------------------------------------------
THREE_A = ((0, 2), (0, 1), (0, 0))  # x3a_mfma's order: the single plane in the A position


def test_three_products_are_the_six_for_one_plane_in_the_a_position_bitwise():
    """One accumulator fed T terms, as a score is over its K16 steps: a bf16
    values (K or H: some of them -0.0 and +0.0, whole chains of -0), b full fp32
    values (Q or P, three planes).  a's planes 1 and 2 are +0, their products
    +-0, and an accumulator that starts at +0 never holds -0, so dropping them
    changes no bit."""
    rng = np.random.default_rng(22)
    n, T = 1 << 14, 24
    a = xi.bf16_rne(rng.standard_normal((T, n)).astype(np.float32))
    b = xi.full_values(rng, (T, n))
    zero = rng.random((T, n)) < 0.2
    a[zero] = np.where(rng.random(zero.sum()) < 0.5, np.float32(-0.0), np.float32(0.0))
    zero = rng.random((T, n)) < 0.1
    b[zero] = np.where(rng.random(zero.sum()) < 0.5, np.float32(-0.0), np.float32(0.0))
    a[:, :64] = np.float32(-0.0)    # whole chains of -0 terms: the accumulator must stay +0
    b[:, 32:96] = np.float32(-0.0)  # ... on either side, and (-0)(-0) = +0 where both are
    assert np.signbit(a[a == 0]).any() and not np.signbit(a[a == 0]).all()
    a0, a1, a2 = xi.split3(a)
    assert np.array_equal(a0.view(np.uint32), a.view(np.uint32))  # one plane: the value's own bits (-0 kept)
    assert not a1.view(np.uint32).any() and not a2.view(np.uint32).any()  # the other two: +0
    assert all(p.any() for p in xi.split3(b))  # b is a split operand: every plane is live
    acc6 = acc3 = None
    for t in range(T):
        acc6 = xi.six_product(a[t], b[t], xi.ORDER, acc6)
        acc3 = xi.six_product(a[t], b[t], THREE_A, acc3)
        assert np.array_equal(acc3.view(np.uint32), acc6.view(np.uint32)), t
    assert not acc3[:96].view(np.uint32).any()  # +0, not -0
    assert THREE_A == tuple(o for o in xi.ORDER if o[0] == 0)  # x6_mfma's sequence less the products on a1, a2
    xi.check_products(xi.six_product(a[0], b[0], THREE_A), a[0], b[0], xi.BARE, "three products")


def test_an_accumulator_that_enters_as_minus_zero_differs_in_sign_only():
    """The forward's o can be -0 when a block begins (an alpha rescale that
    underflowed): the six products turn it into +0 (a2 b0 = +0 first), the
    three keep it where every term is -0.  Values stay equal."""
    a = xi.bf16_rne(np.array([-1.0, 1.0, -0.0, 2.0], np.float32))
    b = np.array([0.0, 0.0, 3.0, 1.0 + 2.0 ** -20], np.float32)
    start = np.full(4, -0.0, np.float32)
    acc6 = xi.six_product(a, b, xi.ORDER, start)
    acc3 = xi.six_product(a, b, THREE_A, start)
    assert np.array_equal(acc3, acc6)  # as values
    assert np.signbit(acc3[0]) and not np.signbit(acc6[0])  # -0 kept / turned into +0
    assert np.array_equal(acc3[3:].view(np.uint32), acc6[3:].view(np.uint32))  # non-zero results: the same bits
