"""GPU: the bf16-output training forward whose Z holds bf16 bits too
(grl_graphconv_fwd_train_bf16_z16; graphconv_ws_bf16oz_kernel).

The gather waves round only the copy of a finished row that goes to memory, so
every check is on BITS: out equals grl_graphconv_fwd_train_bf16_to_bf16's, Z
equals that call's fp32 Z cast by torch (finite data: the same round to nearest
even), a sentinel row behind Z and the columns beside an out slice keep their
pattern.  The shapes are test_gpu_graphconv_bf16_out.py's, just above the x6
GEMM's flop floor; every one-kernel case checks the path by the entry's own
workspace query."""
import ctypes

import numpy as np
import pytest
import torch

from grl import DropEdge, EdgeBlockedGraph, TypedGraph, _lib
from grl.ops import graph_conv_fwd_train
from oracle import hash as ohash

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SENTINEL = 0x5A5A


def _query(X, g, W, C, out, Z):
    csr = g.csr_c(X.shape[1])
    return _lib.lib().grl_graphconv_fwd_train_bf16_z16_workspace_query(
        ctypes.byref(csr), X.data_ptr(), X.stride(0), X.shape[1], W.data_ptr(), C, out.data_ptr(), out.stride(0),
        Z.data_ptr())


def _planes_only(ws, N, K, C):
    """W's planes (and the status word), far below a bf16 Z: the one kernel."""
    return ws < 3 * (256 if C <= 256 else 512) * K * 2 + 4096 < N * K * 2


def _bits(t):
    return t.view(torch.int16)


def _z_with_guard(N, K, offset=0):
    """A contiguous bf16 [N, K] view `offset` elements into a sentinel buffer, with one sentinel row behind it."""
    buf = torch.full((offset + (N + 1) * K,), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)
    return buf, buf[offset:offset + N * K].view(N, K)


def _guard_ok(buf, N, K, offset=0):
    return bool((_bits(buf[:offset]) == SENTINEL).all()) and bool((_bits(buf[offset + N * K:]) == SENTINEL).all())


CASES = [
    # N, L, F, C, has_self, deg
    (20_011, 6, 256, 256, True, 16.0),   # ragged last tile
    (60_001, 3, 256, 200, False, 20.0),  # no self term, ragged C
    (24_001, 6, 256, 512, True, 12.0),   # 4 gather + 8 MFMA waves: two row groups per gather wave
    (10_007, 6, 1024, 512, True, 8.0),   # four virtual segments: the hv column offset of Z
    (70_001, 6, 64, 256, True, 12.0),    # lanes with col_ok false
]


@pytest.mark.parametrize("N,L,F,C,has_self,deg", CASES)
@pytest.mark.parametrize("variant", ["plain", "drop_bias_relu"])
def test_out_is_the_siblings_and_z_its_rounded_z(N, L, F, C, has_self, deg, variant, grl_option):
    full = variant == "drop_bias_relu"
    g = TypedGraph.synthetic(N, deg, L, seed=N % 7, device=DEV)
    if not has_self:
        g = TypedGraph(g.rowptr, g.colidx, L, has_self=False, num_cols=N)
    g = g.with_dropedge(DropEdge(0.3, 3, 2, True) if full else None)
    gen = torch.Generator(device=DEV).manual_seed(N + F)
    Xb = torch.randn(N, F, device=DEV, generator=gen).to(BF16)
    K = g.segments * F
    W = torch.randn(K, C, device=DEV, generator=gen) / K ** 0.5
    b = torch.randn(C, device=DEV, generator=gen) if full else None
    out_ref, Z_ref = graph_conv_fwd_train(Xb, g, W, b, full, out=torch.empty(N, C, dtype=BF16, device=DEV))
    want_out, want_z = _bits(out_ref).clone(), _bits(Z_ref.to(BF16))
    del Z_ref

    def run(offset, one_kernel):
        table = torch.full((N, C + 128), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)
        out = table[:, 64:64 + C]
        buf, Z = _z_with_guard(N, K, offset)
        ws = _query(Xb, g, W, C, out, Z)
        if one_kernel:
            assert _planes_only(ws, N, K, C)
        else:
            assert ws >= N * K * 4
        res, Zr = graph_conv_fwd_train(Xb, g, W, b, full, out=out, Z=Z)
        assert res is out and Zr is Z and Z.dtype == BF16
        assert torch.equal(_bits(out), want_out)
        assert torch.equal(_bits(Z), want_z)
        assert _guard_ok(buf, N, K, offset)
        assert bool((_bits(table[:, :64]) == SENTINEL).all()) and bool((_bits(table[:, 64 + C:]) == SENTINEL).all())

    run(0, True)
    run(1, False)  # a Z that is only 2 B-aligned: the two-kernel form, the same bits
    grl_option("graphconv_fused", 0)
    run(0, False)


def test_z_dtype_allocates_and_edge_values():
    """z_dtype=bfloat16 allocates out and Z; fc_similarity-style edge values (vals != NULL)."""
    N, L, F, C = 20_480, 6, 256, 256
    rowptr, colidx = ohash.synth_csr(0, L, N, N * 12, 5)
    rng = np.random.default_rng(3)
    vals = rng.random(len(colidx)).astype(np.float32)
    g = TypedGraph.from_csr_host(rowptr, colidx, L, DEV, vals=vals).with_dropedge(DropEdge(0.3, 1, 4, True))
    K = 7 * F
    Xb = torch.from_numpy(rng.standard_normal((N, F)).astype(np.float32)).to(DEV).to(BF16)
    W = torch.from_numpy((rng.standard_normal((K, C)) / np.sqrt(K)).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).to(DEV)
    out_ref, Z_ref = graph_conv_fwd_train(Xb, g, W, b, True, out=torch.empty(N, C, dtype=BF16, device=DEV))
    out, Z = graph_conv_fwd_train(Xb, g, W, b, True, z_dtype=BF16)
    assert out.dtype == BF16 and Z.dtype == BF16 and Z.is_contiguous() and tuple(Z.shape) == (N, K)
    assert _planes_only(_query(Xb, g, W, C, out, Z), N, K, C)
    assert torch.equal(_bits(out), _bits(out_ref)) and torch.equal(_bits(Z), _bits(Z_ref.to(BF16)))


def test_what_a_bf16_z_cannot_go_with_raises():
    N, L, F, C = 2_000, 6, 64, 64
    g = TypedGraph.synthetic(N, 8.0, L, seed=1, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(1)
    X = torch.randn(N, F, device=DEV, generator=gen)
    W = torch.randn(7 * F, C, device=DEV, generator=gen)
    with pytest.raises(_lib.GrlError, match="bfloat16 node features"):
        graph_conv_fwd_train(X, g, W, z_dtype=BF16)
    with pytest.raises(_lib.GrlError, match="bfloat16 out"):
        graph_conv_fwd_train(X.to(BF16), g, W, out=torch.empty(N, C, device=DEV), z_dtype=BF16)
    with pytest.raises(_lib.GrlError, match="contiguous bfloat16"):
        graph_conv_fwd_train(X.to(BF16), g, W, Z=torch.empty(N, 14 * F, dtype=BF16, device=DEV)[:, ::2])
    with pytest.raises(_lib.GrlError, match="z_dtype"):
        graph_conv_fwd_train(X.to(BF16), g, W, z_dtype=torch.float16)
    blocked = EdgeBlockedGraph.__new__(EdgeBlockedGraph)  # the type alone decides: nothing of it is read
    with pytest.raises(_lib.GrlError, match="TypedGraph"):
        graph_conv_fwd_train(X.to(BF16), blocked, W, z_dtype=BF16)
    # below the x6 floor the two-kernel form runs: the same contract
    out_ref, Z_ref = graph_conv_fwd_train(X.to(BF16), g, W, out=torch.empty(N, C, dtype=BF16, device=DEV))
    out, Z = graph_conv_fwd_train(X.to(BF16), g, W, z_dtype=BF16)
    assert torch.equal(_bits(out), _bits(out_ref)) and torch.equal(_bits(Z), _bits(Z_ref.to(BF16)))
