"""GPU: the one-kernel GraphConv layer over a bf16 feature table
(grl_graphconv_fwd_bf16, grl_graphconv_fwd_train_bf16; graphconv_ws_bf16_kernel).

The gather waves load a lane's 4 columns as 8 B of bf16 bits and widen them
at the fmaf; widening is exact and the chain, the ring, the MFMA side and the
epilogue are the fp32 kernel's, so every result here is required to be
BITWISE (torch.equal, no tolerance) what the existing fp32 entry gives on
X.float() -- which tests/test_gpu_graphconv.py pins bitwise to the two-kernel
path.  The shapes sit just above the x6 GEMM's 1.6e10-flop floor, as there:
below it no fusion runs and these tests would pass without the kernel, so
every one-kernel case also checks the path by the workspace query."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from grl import DropEdge, TypedGraph, _lib
from grl.ops import graph_conv, graph_conv_fwd_train, graph_conv_infer, spmm_forward
from oracle import hash as ohash

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _ws_query(X, g, W, C):
    """The workspace the forward entry for X's dtype asks for."""
    name = "grl_graphconv_fwd_bf16_workspace_query" if X.dtype == torch.bfloat16 else "grl_graphconv_fwd_workspace_query"
    csr = g.csr_c(X.shape[1])
    return getattr(_lib.lib(), name)(ctypes.byref(csr), X.data_ptr(), X.stride(0), X.shape[1], W.data_ptr(), C)


def _planes_only(ws, N, K, C):
    """The fp32 test's bound: W's planes (and the status word), far below Z."""
    return ws < 3 * (256 if C <= 256 else 512) * K * 2 + 4096 < N * K * 4


def _bf16_randn(N, F, gen, wide=None):
    """A seeded bf16 table [N, F]; wide: a column slice of a [N, wide] one."""
    X = torch.randn(N, wide or F, device=DEV, generator=gen).to(torch.bfloat16)
    return X[:, :F] if wide else X


CASES = [
    # N, L, F, C, has_self, deg
    (20_011, 6, 256, 256, True, 16.0),   # the base case
    (70_001, 6, 64, 256, True, 12.0),    # lanes past the segment, NH = 1
    (40_007, 6, 128, 256, True, 16.0),   # likewise, 32 lanes
    (20_000, 6, 256, 256, True, 120.0),  # more than one 64-entry fetch per list
    (18_001, 7, 256, 256, True, 14.0),   # a full rowptr window
    (60_001, 3, 256, 200, False, 20.0),  # no self term, ragged C
    (20_011, 6, 512, 256, True, 10.0),   # two virtual segments
    (10_007, 6, 1024, 512, True, 8.0),   # four virtual segments, 4 + 8 waves, non-temporal gathers
    (24_001, 6, 256, 512, True, 12.0),   # 4 + 8 waves
]
VARIANTS = ["plain", "drop_bias_relu", "drop_spare_self", "strided_relu"]


@pytest.mark.parametrize("N,L,F,C,has_self,deg", CASES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_inference_bitwise_equals_the_fp32_layer(N, L, F, C, has_self, deg, variant, grl_option):
    de = {"plain": None, "drop_bias_relu": DropEdge(0.3, 3, 2, True), "drop_spare_self": DropEdge(0.25, 9, 0, False),
          "strided_relu": None}[variant]
    bias = variant == "drop_bias_relu"
    relu = variant in ("drop_bias_relu", "strided_relu")
    g = TypedGraph.synthetic(N, deg, L, seed=N % 7, device=DEV)
    if not has_self:
        g = TypedGraph(g.rowptr, g.colidx, L, has_self=False, num_cols=N)
    g = g.with_dropedge(de)
    gen = torch.Generator(device=DEV).manual_seed(N + F)
    Xb = _bf16_randn(N, F, gen, wide=F + 64 if variant == "strided_relu" else None)
    if variant == "strided_relu":  # a column slice of a wider bf16 tensor, read in place
        assert Xb.stride(0) == F + 64 and not Xb.is_contiguous()
    K = g.segments * F
    W = torch.randn(K, C, device=DEV, generator=gen) / K ** 0.5
    b = torch.randn(C, device=DEV, generator=gen) if bias else None
    if deg > 64:  # no heavy-row split plan on this graph: the one-kernel path applies
        assert g.split_stats()["csr"]["heavy_segments"] == 0
    ref = graph_conv_infer(Xb.float(), g, W, b, relu)
    ws = _ws_query(Xb, g, W, C)
    assert _planes_only(ws, N, K, C), ws  # W planes only: one kernel, not SpMM + GEMM
    out = graph_conv_infer(Xb, g, W, b, relu)
    assert out.dtype == torch.float32
    assert torch.equal(out, ref)
    with torch.no_grad():  # graph_conv routes here when no gradient is wanted
        assert torch.equal(graph_conv(Xb, g, W, b, relu), ref)
    grl_option("graphconv_fused", 0)
    assert _ws_query(Xb, g, W, C) >= N * K * 4
    assert torch.equal(graph_conv_infer(Xb, g, W, b, relu), ref)


def test_edge_values():
    """fc_similarity-style edge values (vals != NULL) through the bf16 kernel."""
    N, L, F, C = 20_480, 6, 256, 256
    rowptr, colidx = ohash.synth_csr(0, L, N, N * 12, 5)
    rng = np.random.default_rng(3)
    vals = rng.random(len(colidx)).astype(np.float32)
    g = TypedGraph.from_csr_host(rowptr, colidx, L, DEV, vals=vals).with_dropedge(DropEdge(0.3, 1, 4, True))
    K = 7 * F
    Xb = torch.from_numpy(rng.standard_normal((N, F)).astype(np.float32)).to(DEV).to(torch.bfloat16)
    W = torch.from_numpy((rng.standard_normal((K, C)) / np.sqrt(K)).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).to(DEV)
    assert _planes_only(_ws_query(Xb, g, W, C), N, K, C)
    assert torch.equal(graph_conv_infer(Xb, g, W, b, True), graph_conv_infer(Xb.float(), g, W, b, True))


@functools.lru_cache(maxsize=None)
def _base():
    """The base shape's operands, shared (read-only) by the tests below."""
    N, L, F, C = 20_011, 6, 256, 256
    g = TypedGraph.synthetic(N, 16.0, L, seed=3, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    Xb = _bf16_randn(N, F, gen)
    W = torch.randn(7 * F, C, device=DEV, generator=gen) / 40
    b = torch.randn(C, device=DEV, generator=gen)
    R = torch.randn(N, C, device=DEV, generator=gen)
    return g, Xb, W, b, R


@pytest.mark.parametrize("F,C", [(256, 256), (512, 512)])
@pytest.mark.parametrize("de", [None, DropEdge(0.3, 4, 2, True)])
def test_training_forward_writes_the_bf16_spmm_z(F, C, de):
    N, L = 20_011, 6
    g = TypedGraph.synthetic(N, 10.0 if F > 256 else 16.0, L, seed=2, device=DEV).with_dropedge(de)
    gen = torch.Generator(device=DEV).manual_seed(F + C)
    Xb = _bf16_randn(N, F, gen)
    K = 7 * F
    W = torch.randn(K, C, device=DEV, generator=gen) / K ** 0.5
    b = torch.randn(C, device=DEV, generator=gen)
    assert _planes_only(_ws_query(Xb, g, W, C), N, K, C)  # the shape and table the one kernel takes
    out, Z = graph_conv_fwd_train(Xb, g, W, b, True)
    assert Z.dtype == torch.float32 and out.dtype == torch.float32
    assert torch.equal(Z, spmm_forward(Xb, g))
    out_f, Z_f = graph_conv_fwd_train(Xb.float(), g, W, b, True)
    assert torch.equal(out, out_f) and torch.equal(Z, Z_f)


def _layer(X0, g, W0, b0, R, recompute):
    X, W, b = (t.clone().requires_grad_(True) for t in (X0, W0, b0))
    out = graph_conv(X, g, W, b, relu=True, recompute=recompute)
    (out * R).sum().backward()
    return out.detach(), X.grad, W.grad, b.grad


@pytest.mark.parametrize("recompute", [False, True])
def test_layer_gradients(recompute, grl_option):
    """graph_conv on a bf16 X (one autograd node): out, dW, db bitwise the
    fp32 layer's on X.float(), X.grad that layer's rounded once.  The fp32
    reference is its saved-Z path (recompute=False) under the same path
    options: the fp32 recompute=True layer takes dW_s = X^T G_s (another
    summation order, fp32 X only), which the bf16 layer by design does not --
    it re-aggregates Z from the kept bf16 X.  With the one-kernel data
    gradient off, the fp32 recompute=True layer re-aggregates too, and the
    two are compared recompute for recompute."""
    g, Xb, W, b, R = _base()
    g = g.with_dropedge(DropEdge(0.3, 4, 2, True))
    assert _planes_only(_ws_query(Xb, g, W, W.shape[1]), Xb.shape[0], W.shape[0], W.shape[1])
    ref = _layer(Xb.float(), g, W, b, R, False)
    got = _layer(Xb, g, W, b, R, recompute)
    assert got[1].dtype == torch.bfloat16 and ref[1].dtype == torch.float32
    assert torch.equal(got[0], ref[0]), "out"
    assert torch.equal(got[2], ref[2]), "dW"
    assert torch.equal(got[3], ref[3]), "db"
    assert torch.equal(got[1], ref[1].to(torch.bfloat16)), "dX"
    grl_option("graphconv_fused_bwd", 0)  # dX by the dZ chain; the fp32 recompute layer re-aggregates Z
    ref = _layer(Xb.float(), g, W, b, R, recompute)
    got = _layer(Xb, g, W, b, R, recompute)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])
    assert torch.equal(got[1], ref[1].to(torch.bfloat16))


def test_recompute_keeps_the_bf16_table_not_z():
    """recompute=True holds X (bf16, already the caller's) between the passes:
    the memory held drops by Z against recompute=False."""
    g, Xb, W, b, R = _base()
    held = {}
    for rc in (False, True):
        X = Xb.clone().requires_grad_(True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(DEV)
        out = graph_conv(X, g, W, b, relu=True, recompute=rc)
        torch.cuda.synchronize()
        held[rc] = torch.cuda.memory_allocated(DEV) - base
        del out
    assert held[False] - held[True] >= 0.9 * Xb.shape[0] * W.shape[0] * 4, held


def test_an_ineligible_table_takes_two_kernels_and_gives_the_same_bits():
    """A table offset by one element is 2 B-aligned: no 8 B loads, so the call
    runs grl_typed_spmm_fwd_bf16 into Z, then the linear."""
    g, Xb, W, b, _ = _base()
    N, F = Xb.shape
    K, C = W.shape
    big = torch.empty(N, F + 8, device=DEV, dtype=torch.bfloat16)
    view = big[:, 1:1 + F]
    view.copy_(Xb)
    assert view.data_ptr() % 8 == 2 and view.stride(0) % 4 == 0
    assert _ws_query(view, g, W, C) >= N * K * 4  # Z whole: the two-kernel form
    ref = graph_conv_infer(Xb.float(), g, W, b, True)
    assert torch.equal(graph_conv_infer(view, g, W, b, True), ref)
    out, Z = graph_conv_fwd_train(view, g, W, b, True)
    assert torch.equal(out, ref) and torch.equal(Z, spmm_forward(Xb, g))
    with pytest.raises(_lib.GrlError, match="workspace"):  # no row-chunked form
        graph_conv_infer(view, g, W, b, True, max_workspace_bytes=1 << 20)


def test_no_widened_copy_of_the_table():
    g, Xb, W, b, _ = _base()
    N, F = Xb.shape
    K, C = W.shape
    ws = _ws_query(Xb, g, W, C)
    assert _planes_only(ws, N, K, C)
    ref = graph_conv_infer(Xb, g, W, b, True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = graph_conv_infer(Xb, g, W, b, True)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    assert extra < ws + N * C * 4 + N * F * 2, f"the call allocated {extra} bytes (a widened copy of X is {N * F * 4})"
    assert torch.equal(out, ref)


def test_forced_timeout_names_the_bf16_entries(grl_option):
    """The bounded-wait hook of test_persistent_kernel_timeout_is_an_error on
    the bf16 entries: with a one-sleep bound the call's outputs are poisoned
    (stream-ordered) and grl.check() raises GrlError naming the bf16 entry,
    then clears; with the normal bound the next call is correct again."""
    import grl

    g, Xb, W, b, _ = _base()
    ref = graph_conv_infer(Xb, g, W, b, True)
    assert torch.equal(ref, graph_conv_infer(Xb.float(), g, W, b, True))
    grl.check()  # nothing pending
    grl_option("ws_spin", 1)
    out = graph_conv_infer(Xb, g, W, b, True)  # no raise, no sync: the failure is stream-ordered
    with pytest.raises(_lib.GrlError, match=r"grl_graphconv_fwd_bf16: a wave .* gave up waiting"):
        grl.check()
    assert bool(torch.isnan(out).all())
    grl.check()  # cleared
    out_t, Z_t = graph_conv_fwd_train(Xb, g, W, b, True)
    with pytest.raises(_lib.GrlError, match=r"grl_graphconv_fwd_train_bf16: a wave .* gave up waiting"):
        grl.check()
    assert bool(torch.isnan(out_t).all()) and bool(torch.isnan(Z_t).all())
    grl_option("ws_spin", 0)
    assert torch.equal(graph_conv_infer(Xb, g, W, b, True), ref)
    grl.check()


def test_unsupported_dtypes_still_raise():
    g, Xb, W, b, _ = _base()
    for bad in (torch.float16, torch.float64):
        with pytest.raises(_lib.GrlError, match="float32 or bfloat16"):
            graph_conv_infer(Xb.to(bad), g, W, b, True)
        with pytest.raises(_lib.GrlError, match="float32 or bfloat16"):
            graph_conv_fwd_train(Xb.to(bad), g, W, b, True)
        with pytest.raises(_lib.GrlError, match="float32 or bfloat16"):
            graph_conv(Xb.to(bad), g, W, b, True)
    for fn in (graph_conv_infer, graph_conv_fwd_train, graph_conv):
        with pytest.raises(_lib.GrlError, match="must be float32"):
            fn(Xb, g, W.to(torch.bfloat16), b, True)
        with pytest.raises(_lib.GrlError, match="must be float32"):
            fn(Xb, g, W, b.to(torch.bfloat16), True)
