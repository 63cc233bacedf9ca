"""GPU: the typed SpMM over a bf16 feature table (grl_typed_spmm_fwd_bf16).

Widening bf16 to fp32 is exact and the kernel runs the fp32 kernel's fmaf
chain in CSR order, so every result here is required to be BITWISE equal to
the CPU oracle (and to the fp32 kernel) on the widened table Xb.float() --
through every form of the kernel: two edges per 16 B-a-lane instruction
(F <= 256), one row per instruction (F <= 512), 512-column blocks, the
one-element-a-lane fallback, hub rows through the split plan, row ranges and
column slices.  The gradient is the fp32 backward rounded once to bf16.
"""
import numpy as np
import pytest
import torch

from grl import DropEdge, TypedGraph, _lib
from grl.ops import graph_conv, spmm_forward, spmm_forward_slice, typed_aggregate
from oracle import c_oracle
from oracle import hash as ohash

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EBASE, SBASE = 1234, 10 ** 9 + 7


def host_graph(N, L, deg, seed, hub=0, vals=False):
    """ER typed CSR (oracle generator) + optional hub row with `hub` extra
    edges spread over types, + optional float values (as test_gpu_kernels)."""
    rowptr, colidx = ohash.synth_csr(0, L, N, int(N * deg), seed)
    if hub:
        rng = np.random.default_rng(seed + 1)
        rows = [colidx[rowptr[s]:rowptr[s + 1]] for s in range(N * L)]
        for t in range(L):
            extra = rng.integers(0, N, size=hub // L + 1)
            rows[t] = np.unique(np.concatenate([rows[t], extra])).astype(np.int32)
        colidx = np.concatenate(rows).astype(np.int32)
        rowptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    v = np.random.default_rng(seed + 2).uniform(0.1, 2.0, colidx.size).astype(np.float32) if vals else None
    return rowptr, colidx, v


def bf16_table(N, F, seed):
    """(Xb, Xw): a seeded standard-normal table rounded to bf16, a handful of
    rows scaled by 2^40 and 2^-40, and its exact fp32 widening (host)."""
    X = np.random.default_rng(seed).standard_normal((N, F)).astype(np.float32)
    for i, r in enumerate((1, 5, 17, 40, 63)):
        X[r % N] *= np.float32(2.0 ** (40 if i % 2 == 0 else -40))
    Xb = torch.from_numpy(X).to(torch.bfloat16)
    return Xb, Xb.float()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def assert_bitwise(got, ref, what):
    if isinstance(ref, np.ndarray):
        ref = torch.from_numpy(ref)
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), what
    if not torch.equal(bits(got), bits(ref)):
        d = (got.detach().cpu().double() - ref.double()).abs()
        raise AssertionError(f"{what}: not bitwise equal, max|d|={d.max():.3e}, {int((bits(got) != bits(ref)).sum())} "
                             f"of {d.numel()} elements differ")


def oracle_drop(de):
    return None if de is None else c_oracle.drop(de.p, de.seed, de.call, de.drop_self)


CASES = [
    # N, L, deg, F, hub, vals, has_self
    (300, 6, 16.0, 256, 0, False, True),   # pair form, full half-waves
    (300, 6, 16.0, 512, 0, True, True),    # one row per instruction
    (257, 6, 4.0, 16, 0, False, True),     # pair form, 2 lanes per row
    (129, 6, 8.0, 10, 0, True, True),      # scalar form
    (200, 3, 12.0, 100, 0, False, False),  # F % 4 == 0 but F % 8 != 0: falls back; no identity block
    (90, 6, 6.0, 1000, 0, False, True),    # two column blocks of 512, the second partial
    (500, 6, 2.0, 256, 700, False, True),  # > 64 edges in a segment, odd survivor counts for the pair form
    (64, 7, 0.0, 64, 0, False, True),      # no edges at all
]
DROPS = [None, DropEdge(0.3, 7, 1, True), DropEdge(0.2, 99, 4, False), DropEdge(1.0, 5, 0, True)]


def build_case(case, de):
    N, L, deg, F, hub, vals, hs = case
    rowptr, colidx, v = host_graph(N, L, deg, 1000 + N, hub, vals)
    g = TypedGraph.from_csr_host(rowptr, colidx, L, DEV, vals=v, has_self=hs, edge_id_base=EBASE,
                                 self_id_base=SBASE).with_dropedge(de)
    Xb, Xw = bf16_table(N, F, N + F)
    return rowptr, colidx, v, g, Xb, Xw


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("di", range(len(DROPS)))
def test_forward_bitwise(case, di):
    N, L, deg, F, hub, vals, hs = case
    de = DROPS[di]
    rowptr, colidx, v, g, Xb, Xw = build_case(case, de)
    Z = typed_aggregate(Xb.to(DEV), g)
    assert Z.dtype == torch.float32
    Zref = c_oracle.spmm_fwd(rowptr, colidx, Xw.numpy(), L, hs, vals=v, d=oracle_drop(de), edge_base=EBASE,
                             self_base=SBASE)
    assert_bitwise(Z, Zref, "bf16 forward vs oracle on the widened table")
    assert_bitwise(Z, typed_aggregate(Xw.to(DEV), g), "bf16 forward vs fp32 kernel on the widened table")


@pytest.mark.parametrize("ci", [0, 3, 6])
@pytest.mark.parametrize("di", range(len(DROPS)))
def test_backward_is_the_fp32_gradient_rounded_once(ci, di):
    N, L, deg, F, hub, vals, hs = CASES[ci]
    de = DROPS[di]
    rowptr, colidx, v, g, Xb, Xw = build_case(CASES[ci], de)
    Xt = Xb.to(DEV).requires_grad_()
    Z = typed_aggregate(Xt, g)
    dZ = np.random.default_rng(N + F + 1).standard_normal(tuple(Z.shape)).astype(np.float32)
    Z.backward(torch.from_numpy(dZ).to(DEV))
    assert Xt.grad.dtype == torch.bfloat16
    colptr, zrow, eid, cvals = c_oracle.csr_to_csc(rowptr, colidx, L, N, hs, v)
    dXref = c_oracle.spmm_bwd(colptr, zrow, eid, dZ, L, F, N, hs, cvals, d=oracle_drop(de), edge_base=EBASE,
                              self_base=SBASE)
    assert_bitwise(Xt.grad, torch.from_numpy(dXref).to(torch.bfloat16), "backward")


@pytest.mark.parametrize("F", [256, 10])
@pytest.mark.parametrize("di", [0, 1])
def test_split_plan_bitwise_rmat(F, di):
    """Hub rows of a power-law graph: chunk partials in fp32, summed by the
    fixup in chunk order -- the oracle's restatement of that order, bitwise."""
    N, L, split = 1 << 12, 6, (64, 24)
    rowptr, colidx = ohash.synth_csr(1, L, N, N * 40, 21)
    assert np.diff(rowptr[::L]).max() > split[0]
    de = DROPS[di]
    g = TypedGraph.from_csr_host(rowptr, colidx, L, DEV).with_dropedge(de)
    g.split_threshold, g.split_chunk = split
    Xb, Xw = bf16_table(N, F, F)
    Z = typed_aggregate(Xb.to(DEV), g)
    assert g.split_stats()["csr"]["heavy_segments"] > 0
    Zref = c_oracle.spmm_fwd(rowptr, colidx, Xw.numpy(), L, True, d=oracle_drop(de), split=split)
    assert_bitwise(Z, Zref, "forward (split)")


def test_strided_table_is_read_in_place():
    """A column slice of a wider table (ldx = 3F), 16 B-aligned, and one that
    starts at an odd column (2 B-aligned: the one-element-a-lane form)."""
    N, L, F = 150, 6, 128
    rowptr, colidx, _ = host_graph(N, L, 10.0, 5)
    g = TypedGraph.from_csr_host(rowptr, colidx, L, DEV)
    big, big_w = bf16_table(N, 3 * F, 0)
    big_dev = big.to(DEV)
    for c0 in (F, 1):
        view = big_dev[:, c0:c0 + F]
        assert view.data_ptr() == big_dev.data_ptr() + 2 * c0 and view.stride(0) == 3 * F
        Z = typed_aggregate(view, g)
        Zref = c_oracle.spmm_fwd(rowptr, colidx, big_w[:, c0:c0 + F].numpy().copy(), L, True)
        assert_bitwise(Z, Zref, f"strided forward from column {c0}")


@pytest.mark.parametrize("F", [256, 10])
def test_row_ranges_equal_the_whole_result(F):
    case = (300, 6, 16.0, F, 0, True, True)
    _, _, _, g, Xb, _ = build_case(case, DROPS[1])
    Xd = Xb.to(DEV)
    Z = spmm_forward(Xd, g)
    for r0, r1 in ((0, 1), (37, 200), (299, 300)):
        assert_bitwise(spmm_forward(Xd, g.rows_view(r0, r1)), Z[r0:r1], f"rows [{r0}, {r1})")


@pytest.mark.parametrize("col0,F", [(64, 128), (3, 5), (8, 184)])
def test_column_slice_into_a_wider_out(col0, F):
    """spmm_forward_slice: the slice's table is a view of the whole-width one
    (no copy), out is whole-width; the columns written are bitwise the
    whole-width result's and the others are untouched."""
    N, L, Ft = 300, 6, 192
    case = (N, L, 16.0, Ft, 0, True, True)
    _, _, _, g, Xb, _ = build_case(case, DROPS[1])
    Xd = Xb.to(DEV)
    S = g.segments
    Zw = spmm_forward(Xd, g).view(N, S, Ft)
    out = torch.full((N, S * Ft), -7.0, device=DEV)
    spmm_forward_slice(Xd[:, col0:col0 + F], g, out, col0)
    out = out.view(N, S, Ft)
    assert_bitwise(out[:, :, col0:col0 + F], Zw[:, :, col0:col0 + F], "slice columns")
    assert bool((out[:, :, :col0] == -7.0).all()) and bool((out[:, :, col0 + F:] == -7.0).all())


def test_no_widened_copy_of_the_table():
    N, F = 4096, 256
    g = TypedGraph.synthetic(N, 8.0, 6, seed=3, device=DEV)
    Xb = torch.randn(N, F, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)).to(torch.bfloat16)
    Z = torch.empty(N, g.segments * F, device=DEV)
    spmm_forward(Xb, g, out=Z)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    spmm_forward(Xb, g, out=Z)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - torch.cuda.memory_allocated()
    assert extra < N * F * 2, f"the call allocated {extra} bytes (a widened copy of X is {N * F * 4})"
    assert_bitwise(Z, spmm_forward(Xb.float(), g), "bf16 vs fp32 forward")


def test_graph_conv_layer_bitwise_and_gradients():
    N, L, F, C = 300, 6, 64, 32
    rowptr, colidx, _ = host_graph(N, L, 16.0, 1300)
    g = TypedGraph.from_csr_host(rowptr, colidx, L, DEV).with_dropedge(DropEdge(0.3, 11, 2, True))
    Xb, Xw = bf16_table(N, F, 9)
    rng = np.random.default_rng(10)
    W = (rng.standard_normal(((L + 1) * F, C)) / np.sqrt((L + 1) * F)).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    res = []
    for X in (Xb, Xw):
        Xt = X.to(DEV).requires_grad_()
        Wt = torch.from_numpy(W).to(DEV).requires_grad_()
        bt = torch.from_numpy(b).to(DEV).requires_grad_()
        out = graph_conv(Xt, g, Wt, bt, relu=True)
        out.sum().backward()
        res.append((out, Wt.grad, bt.grad, Xt.grad))
    (ob, dWb, dbb, dXb), (ow, dWw, dbw, dXw) = res
    assert ob.dtype == torch.float32 and dXb.dtype == torch.bfloat16 and dXw.dtype == torch.float32
    assert_bitwise(ob, ow, "layer output")
    assert_bitwise(dWb, dWw, "dW")
    assert_bitwise(dbb, dbw, "db")
    assert_bitwise(dXb, dXw.to(torch.bfloat16), "dX")
    with torch.no_grad():
        assert_bitwise(graph_conv(Xb.to(DEV), g, torch.from_numpy(W).to(DEV), torch.from_numpy(b).to(DEV), relu=True),
                       ow, "layer output without autograd")


def test_edge_blocked_graph_takes_bf16():
    """An EdgeBlockedGraph aggregates block by block through the slice form,
    so it reads a bf16 table as well: forward, gradient and the layer."""
    from grl import EdgeBlockedGraph

    N, L, F, C = 1 << 12, 6, 40, 16
    de = DropEdge(0.3, 5, 2)
    g = TypedGraph.synthetic(N, 12.0, L, seed=3, device=DEV).with_dropedge(de)
    gb = EdgeBlockedGraph.synthetic(N, 12.0, L, seed=3, device=DEV, max_block_edges=20_000).with_dropedge(de)
    assert len(gb.blocks) > 1
    Xb, Xw = bf16_table(N, F, 4)
    Xt = Xb.to(DEV).requires_grad_()
    Zw = spmm_forward(Xw.to(DEV), g)
    Z = typed_aggregate(Xt, gb)
    assert_bitwise(Z, Zw, "blocked bf16 forward vs one fp32 CSR")
    dZ = torch.randn(Z.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    Z.backward(dZ)
    Xf = Xw.to(DEV).requires_grad_()
    typed_aggregate(Xf, gb).backward(dZ)
    assert_bitwise(Xt.grad, Xf.grad.to(torch.bfloat16), "blocked backward")
    W = torch.randn((L + 1) * F, C, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7)) / 16
    with torch.no_grad():
        assert_bitwise(graph_conv(Xb.to(DEV), gb, W, None, relu=True), graph_conv(Xw.to(DEV), gb, W, None, relu=True),
                       "blocked layer")


def test_other_dtypes_still_raise():
    g = TypedGraph.from_csr_host(np.zeros(13, np.int32), np.zeros(0, np.int32), 6, DEV)
    with pytest.raises(_lib.GrlError, match="float32"):
        typed_aggregate(torch.zeros(2, 8, device=DEV, dtype=torch.float16), g)
    with pytest.raises(_lib.GrlError, match="bfloat16"):
        spmm_forward_slice(torch.zeros(2, 8, device=DEV, dtype=torch.float64), g, torch.zeros(2, 56, device=DEV), 0)
