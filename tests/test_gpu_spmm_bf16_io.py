"""GPU: the typed SpMM with bf16 on both sides -- grl_typed_spmm_fwd_bf16_to_bf16
(bf16 table gathered, bf16 Z written) and grl_typed_spmm_bwd_bf16 (bf16 dZ
gathered, bf16 dX written).

The arithmetic is the fp32 kernels': exact widening, one fmaf per kept entry
in CSR / CSC order into fp32 accumulators, heavy rows as fp32 chunk partials
added in chunk order by a fixup.  Only the store differs: one rounding to
nearest even.  So every result here is required to be BITWISE torch's CPU
`.to(torch.bfloat16)` of the CPU oracle's fp32 result on the widened
operands (c_oracle.spmm_fwd / spmm_bwd, with split= where a plan is forced).
Every output buffer handed to a call is filled with the bf16 sentinel -7.0
first, so a store that does not happen shows.

No query tells which kernel ran; the forms are selected by what the launcher
reads (launch_spmm_bf16io): 16 B a lane when the gathered rows and the output
are 16 B-aligned and every stride, F and the segment stride are multiples of
8 -- F <= 256 two entries per instruction (the pair kernel), else one row per
instruction in 512-column blocks; otherwise one bf16 a lane with NV = 1
(F <= 64), 2 (F <= 128) or 4.
"""
import functools

import numpy as np
import pytest
import torch

import graph_patterns as gp
import spmm_patterns as sp
import test_spmm_bf16_io_design as rd
from grl import DropEdge, EdgeBlockedGraph, TypedGraph, _lib
from grl.ops import (spmm_backward, spmm_backward_slice, spmm_forward, spmm_forward_slice, typed_aggregate)
from oracle import c_oracle
from oracle import hash as ohash

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SENTINEL = -7.0
EBASE, SBASE = sp.EDGE_ID_BASE, sp.SELF_ID_BASE


def bits(t):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.array(t))
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def rounded(a):
    """torch's CPU round-to-nearest-even bf16 of an fp32 host array."""
    return torch.from_numpy(np.array(a)).to(BF16)


def assert_bitwise(got, ref, what):
    assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), what
    g, r = bits(got), bits(ref)
    if not torch.equal(g, r):
        bad = (g != r).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ, first at {bad[0].tolist()}: "
                             f"{got.detach().cpu()[tuple(bad[0])]} vs {ref[tuple(bad[0])]}")


def sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=BF16, device=DEV)


def odrop(de):
    return None if de is None else c_oracle.drop(de.p, de.seed, de.call, de.drop_self)


# ------------------------------------------------------------------ random cases
def host_graph(N, L, deg, seed, hub=0, vals=False):
    """ER typed CSR (oracle generator) + optional hub row with `hub` extra
    edges spread over types, + optional float values."""
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


def bf16_table(shape, seed):
    """A seeded standard-normal table rounded to bf16, a handful of rows
    scaled by 2^40 and 2^-40 (host)."""
    X = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    for i, r in enumerate((1, 5, 17, 40, 63)):
        X[r % shape[0]] *= np.float32(2.0 ** (40 if i % 2 == 0 else -40))
    return torch.from_numpy(X).to(BF16)


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


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("di", range(len(DROPS)))
def test_random_cases_both_directions(case, di):
    N, L, deg, F, hub, vals, hs = case
    de = DROPS[di]
    S = L + (1 if hs else 0)
    rowptr, colidx, v = host_graph(N, L, deg, 1000 + N, hub, vals)
    g = TypedGraph.from_csr_host(rowptr, colidx, L, DEV, vals=v, has_self=hs, edge_id_base=EBASE,
                                 self_id_base=SBASE).with_dropedge(de)
    Xb = bf16_table((N, F), N + F)
    dZb = torch.from_numpy(np.random.default_rng(N + F + 1).standard_normal((N, S * F)).astype(np.float32)).to(BF16)
    Zref = rounded(c_oracle.spmm_fwd(rowptr, colidx, Xb.float().numpy(), L, hs, vals=v, d=odrop(de), edge_base=EBASE,
                                     self_base=SBASE))
    colptr, zrow, eid, cvals = c_oracle.csr_to_csc(rowptr, colidx, L, N, hs, v)
    dXref = rounded(c_oracle.spmm_bwd(colptr, zrow, eid, dZb.float().numpy(), L, F, N, hs, cvals, d=odrop(de),
                                      edge_base=EBASE, self_base=SBASE))
    Xd, dZd = Xb.to(DEV), dZb.to(DEV)
    Z16 = spmm_forward(Xd, g, out=sentinel(N, S * F))
    assert_bitwise(Z16, Zref, "bf16 forward vs the oracle, rounded once")
    assert_bitwise(Z16, spmm_forward(Xd, g).to(BF16).cpu(), "bf16 forward vs the fp32-Z forward, rounded")
    Xt = Xd.clone().requires_grad_()
    Za = typed_aggregate(Xt, g, out_dtype=BF16)
    assert Za.dtype == BF16
    assert_bitwise(Za, Zref, "typed_aggregate(out_dtype=bf16)")
    Za.backward(dZd)
    assert Xt.grad.dtype == BF16
    assert_bitwise(Xt.grad, dXref, "autograd backward")
    dX16 = spmm_backward(dZd, g, F, out=sentinel(N, F))
    assert_bitwise(dX16, dXref, "spmm_backward(out=bf16)")
    assert_bitwise(spmm_backward(dZd, g, F, out_dtype=BF16), dXref, "spmm_backward(out_dtype=bf16)")


# ---------------------------------------------------------------- designed graphs
VARIANTS = {"none": None, "vals": None, **{k: DropEdge(*v) for k, v in sp.VARIANTS.items()}}
GRID = [("A", v) for v in VARIANTS] + [("B", v) for v in ("none", "drop03", "vals")]
SIDES = ["P", "PT"]
SPLITS = [None, sp.SPLIT]
# name: F, whether the operands are views that start one element into a wider allocation
FORMS = {"pair256": (256, False), "pair16": (16, False), "row512": (512, False), "scalar_nv1": (10, False),
         "scalar_nv2": (100, False), "scalar_nv4": (130, False), "scalar_by_alignment": (128, True)}
XCOLS = 520


class Case:
    """One shape's host arrays on one side (P or its transpose), read-only."""

    def __init__(self, shape, side):
        self.N, self.L, self.has_self = N, L, hs = sp.SHAPES[shape]
        rp, ci, self.at = sp.pattern_graph(N, L, sp.SEED)
        if side == "PT":
            rp, ci = gp.transpose_host(rp, ci, L, N)
        self.rowptr, self.colidx = rp, ci
        self.S = L + (1 if hs else 0)
        self.vals = sp.edge_values(rp, L, N)
        rng = np.random.default_rng(N + L)
        self.Xb = torch.from_numpy(rng.standard_normal((N, XCOLS)).astype(np.float32)).to(BF16)
        self.Xw = self.Xb.float().numpy()
        self.dZb = torch.from_numpy(rng.standard_normal((N, self.S, 512)).astype(np.float32)).to(BF16)
        self.dZw = self.dZb.float().numpy()
        self.csc = c_oracle.csr_to_csc(rp, ci, L, N, hs, None)
        self.csc_vals = c_oracle.csr_to_csc(rp, ci, L, N, hs, self.vals)

    def graph(self, variant, split=None):
        g = TypedGraph.from_csr_host(self.rowptr, self.colidx, self.L, DEV, has_self=self.has_self,
                                     vals=self.vals if variant == "vals" else None, edge_id_base=EBASE,
                                     self_id_base=SBASE).with_dropedge(VARIANTS[variant])
        if split is not None:
            g.split_threshold, g.split_chunk = split
        return g

    def dz(self, F):
        """(bf16 host tensor [N, S * F], its widening) of the first F columns of every segment."""
        return (self.dZb[:, :, :F].reshape(self.N, self.S * F).contiguous(),
                np.ascontiguousarray(self.dZw[:, :, :F]).reshape(self.N, self.S * F))


@functools.lru_cache(maxsize=4)
def _case(shape, side):
    return Case(shape, side)


@functools.lru_cache(maxsize=128)
def _oracle_fwd(shape, side, variant, split, F, col0):
    """The CPU oracle's Z over table columns [col0, col0 + F), rounded once; computed once."""
    c = _case(shape, side)
    X = np.ascontiguousarray(c.Xw[:, col0:col0 + F])
    return rounded(c_oracle.spmm_fwd(c.rowptr, c.colidx, X, c.L, c.has_self, vals=c.vals if variant == "vals" else None,
                                     d=odrop(VARIANTS[variant]), edge_base=EBASE, self_base=SBASE, split=split))


@functools.lru_cache(maxsize=128)
def _oracle_bwd(shape, side, variant, split, F):
    c = _case(shape, side)
    colptr, zrow, eid, cvals = c.csc_vals if variant == "vals" else c.csc
    return rounded(c_oracle.spmm_bwd(colptr, zrow, eid, c.dz(F)[1], c.L, F, c.N, c.has_self, cvals,
                                     d=odrop(VARIANTS[variant]), edge_base=EBASE, self_base=SBASE, split=split))


def _one_in(numel):
    """A sentinel-filled contiguous bf16 vector of `numel` elements that starts
    one element (2 B) into its allocation."""
    buf = sentinel(numel + 8)
    v = buf[1:1 + numel]
    assert v.data_ptr() % 16 == 2
    return v


@pytest.mark.parametrize("split", SPLITS, ids=["default_split", "split_64_24"])
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("shape,variant", GRID)
def test_designed_graphs_every_form_both_directions(shape, variant, side, split):
    """Every load / store form, forward and backward, on the pattern graph and
    its transpose: whole rows and columns on the default split, chunk partials
    and the rounding fixup at split (64, 24)."""
    c = _case(shape, side)
    N, S = c.N, c.S
    g = c.graph(variant, split)
    for name, (F, one_in) in FORMS.items():
        what = f"{shape} {side} {variant} split={split} {name} F={F}"
        dzb, _ = c.dz(F)
        if one_in:
            wide = c.Xb[:, :1 + F + 3].contiguous().to(DEV)
            X = wide[:, 1:1 + F]
            assert X.data_ptr() % 16 == 2
            Z = _one_in(N * S * F).view(N, S * F)
            dZ = _one_in(N * S * F).view(N, S * F).copy_(dzb)
            dX = _one_in(N * F).view(N, F)
        else:
            X = c.Xb[:, :F].contiguous().to(DEV)
            Z, dZ, dX = sentinel(N, S * F), dzb.to(DEV), sentinel(N, F)
            assert all(t.data_ptr() % 16 == 0 for t in (X, Z, dZ, dX))
        spmm_forward(X, g, out=Z)
        assert_bitwise(Z, _oracle_fwd(shape, side, variant, split, F, 1 if one_in else 0), what + " forward")
        spmm_backward(dZ, g, F, out=dX)
        assert_bitwise(dX, _oracle_bwd(shape, side, variant, split, F), what + " backward")
    stats = g.split_stats()
    if split is None:
        assert stats == {"csr": {"heavy_segments": 0, "chunks": 0}, "csc": {"heavy_segments": 0, "chunks": 0}}
    else:
        assert stats["csr"]["heavy_segments"] > 0 and stats["csr"]["chunks"] > 0
        assert stats["csc"]["heavy_segments"] > 0 and stats["csc"]["chunks"] > 0


# ----------------------------------------------------------------------- rounding
@pytest.mark.parametrize("F_pad", [0, 3], ids=["vector", "scalar"])
@pytest.mark.parametrize("split", [None, rd.SPLIT], ids=["default_split", "split_64_24"])
def test_rounding_design(split, F_pad):
    """tests/test_spmm_bf16_io_design.py's sums -- exact ties with an even and
    an odd lower neighbour, just above and just below a tie, both signs --
    forward on P and backward on its transpose; with the split forced the hub's
    ties are rounded by the fixup.  F_pad = 3 reads the 16 columns from a table
    of row stride 19: the one-element-a-lane store."""
    d = rd.design()
    N, L, F, S = rd.N, rd.L, rd.F, rd.S
    Zf, dXf = rd.oracle(d, split)
    gf = TypedGraph.from_csr_host(d["rowptr"], d["colidx"], L, DEV, has_self=rd.HAS_SELF)
    gt = TypedGraph.from_csr_host(d["rowptr_t"], d["colidx_t"], L, DEV, has_self=rd.HAS_SELF)
    if split is not None:
        for g in (gf, gt):
            g.split_threshold, g.split_chunk = split
    Xwide = torch.zeros(N, F + F_pad, dtype=BF16)
    Xwide[:, :F] = torch.from_numpy(d["X"]).to(BF16)
    X = Xwide.to(DEV)[:, :F]
    Z = spmm_forward(X, gf, out=sentinel(N, S * F))
    assert_bitwise(Z, rounded(Zf), "design forward")
    dXbuf = sentinel(N, F + F_pad)
    dX = spmm_backward(torch.from_numpy(d["dZ"]).to(BF16).to(DEV), gt, F, out=dXbuf[:, :F])
    assert_bitwise(dX, rounded(dXf), "design backward")
    assert bool((dXbuf[:, F:] == SENTINEL).all())
    if split is not None:
        assert gf.split_stats()["csr"]["heavy_segments"] == L and gt.split_stats()["csc"]["heavy_segments"] == 1
    # the classes are in what the GPU wrote: a tie with an even neighbour stays, one with an odd neighbour goes up
    cf = rd.classes(Zf)
    got, trunc = bits(Z).numpy().view(np.uint16), (Zf.view(np.uint32) >> 16).astype(np.uint16)
    assert (got == trunc)[cf["tie_even"] | cf["below"]].all() and (got == trunc + 1)[cf["tie_odd"] | cf["above"]].all()


# ------------------------------------------------------------------ column slices
@pytest.mark.parametrize("variant", ["none", "drop03"])
@pytest.mark.parametrize("col0,F", [(64, 128), (3, 5), (8, 184)])
def test_column_slices_both_directions(col0, F, variant):
    """spmm_forward_slice into a wider bf16 out and spmm_backward_slice from a
    wider bf16 dZ, on the heavy graph: the columns written are bitwise the whole
    call's, the others still hold the sentinel; dX goes into a strided view."""
    c = _case("A", "P")
    g = c.graph(variant, sp.SPLIT)
    N, S, Ft = c.N, c.S, 192
    Xd = c.Xb[:, :Ft].contiguous().to(DEV)
    whole = spmm_forward(Xd, g, out=sentinel(N, S * Ft))
    assert_bitwise(whole, _oracle_fwd("A", "P", variant, sp.SPLIT, Ft, 0), "whole-width forward")
    out = spmm_forward_slice(Xd[:, col0:col0 + F], g, sentinel(N, S * Ft), col0).view(N, S, Ft)
    assert_bitwise(out[:, :, col0:col0 + F], whole.view(N, S, Ft)[:, :, col0:col0 + F].cpu(), "forward slice columns")
    assert bool((out[:, :, :col0] == SENTINEL).all()) and bool((out[:, :, col0 + F:] == SENTINEL).all())
    dZ = c.dz(Ft)[0].to(DEV)
    dXw = spmm_backward(dZ, g, Ft, out=sentinel(N, Ft))
    assert_bitwise(dXw, _oracle_bwd("A", "P", variant, sp.SPLIT, Ft), "whole-width backward")
    buf = sentinel(N, F + 4)
    spmm_backward_slice(dZ, g, col0, buf[:, :F])
    assert_bitwise(buf[:, :F], dXw[:, col0:col0 + F].cpu(), "backward slice columns")
    assert bool((buf[:, F:] == SENTINEL).all())


# --------------------------------------------------------------------- row ranges
@pytest.mark.parametrize("F", [256, 512, 10])
def test_row_ranges_equal_the_whole_result(F):
    c = _case("A", "P")
    g = c.graph("drop03")
    Xd = c.Xb[:, :F].contiguous().to(DEV)
    Z = spmm_forward(Xd, g, out_dtype=BF16)
    assert_bitwise(Z, _oracle_fwd("A", "P", "drop03", None, F, 0), "whole")
    for r0, r1 in ((0, 1), (37, 411), (c.N - 1, c.N)):
        out = spmm_forward(Xd, g.rows_view(r0, r1), out=sentinel(r1 - r0, c.S * F))
        assert_bitwise(out, Z[r0:r1].cpu(), f"rows [{r0}, {r1})")


# ------------------------------------------------------------- expanded gradient
def test_expanded_gradient_is_copied_in_bf16():
    """Z16.sum().backward(): autograd hands over an expanded (stride-0) bf16
    gradient of ones; dX is the oracle's for an all-ones dZ."""
    c = _case("A", "P")
    F = 64
    g = c.graph("drop03", sp.SPLIT)
    Xt = c.Xb[:, :F].contiguous().to(DEV).requires_grad_()
    typed_aggregate(Xt, g, out_dtype=BF16).sum().backward()
    colptr, zrow, eid, cvals = c.csc
    ref = c_oracle.spmm_bwd(colptr, zrow, eid, np.ones((c.N, c.S * F), dtype=np.float32), c.L, F, c.N, c.has_self,
                            cvals, d=odrop(VARIANTS["drop03"]), edge_base=EBASE, self_base=SBASE, split=sp.SPLIT)
    assert Xt.grad.dtype == BF16
    assert_bitwise(Xt.grad, rounded(ref), "dX of an all-ones dZ")


# ---------------------------------------------------------------- no widened copy
def test_no_widened_copy_on_either_side():
    N, F = 4096, 256
    g = TypedGraph.synthetic(N, 8.0, 6, seed=3, device=DEV)
    S = g.segments
    gen = torch.Generator(device=DEV).manual_seed(2)
    Xb = torch.randn(N, F, device=DEV, generator=gen).to(BF16)
    dZb = torch.randn(N, S * F, device=DEV, generator=gen).to(BF16)
    Z, dX = sentinel(N, S * F), sentinel(N, F)

    def extra(fn):
        fn()  # warm: the graph's cached CSC and plans
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - torch.cuda.memory_allocated()

    e = extra(lambda: spmm_forward(Xb, g, out=Z))
    assert e < N * F * 2, f"the forward allocated {e} bytes (an fp32 Z is {N * S * F * 4})"
    e = extra(lambda: spmm_backward(dZb, g, F, out=dX))
    assert e < N * F * 2, f"the backward allocated {e} bytes beyond its output (an fp32 dZ copy is {N * S * F * 4})"
    assert_bitwise(Z, spmm_forward(Xb, g).to(BF16).cpu(), "bf16-out vs fp32-Z forward, rounded")
    assert_bitwise(dX, spmm_backward(dZb.float(), g, F).to(BF16).cpu(), "bf16 backward vs the fp32 chain, rounded")


# ------------------------------------------------------------------- edge blocks
def test_edge_blocked_graph_equals_one_csr():
    N, L, F = 1 << 12, 6, 40
    de = DropEdge(0.3, 5, 2)
    g = TypedGraph.synthetic(N, 12.0, L, seed=3, device=DEV).with_dropedge(de)
    gb = EdgeBlockedGraph.synthetic(N, 12.0, L, seed=3, device=DEV, max_block_edges=20_000).with_dropedge(de)
    assert len(gb.blocks) > 1
    Xb = bf16_table((N, F), 4).to(DEV)
    dZ = torch.randn(N, g.segments * F, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6)).to(BF16)
    res = []
    for graph in (g, gb):
        Xt = Xb.clone().requires_grad_()
        Z = typed_aggregate(Xt, graph, out_dtype=BF16)
        Z.backward(dZ)
        assert Z.dtype == BF16 and Xt.grad.dtype == BF16
        res.append((Z.detach(), Xt.grad))
    assert_bitwise(res[1][0], res[0][0].cpu(), "blocked bf16 forward vs one CSR")
    assert_bitwise(res[1][1], res[0][1].cpu(), "blocked bf16 backward vs one CSR")
    assert_bitwise(res[0][0], spmm_forward(Xb.float(), g).to(BF16).cpu(), "one CSR vs the fp32 forward, rounded")
    assert_bitwise(spmm_forward(Xb, gb, out=sentinel(N, g.segments * F)), res[0][0].cpu(), "blocked forward into out")
    assert_bitwise(spmm_backward(dZ, gb, F, out=sentinel(N, F)), res[0][1].cpu(), "blocked backward into out")


# ------------------------------------------------------------------------ errors
def test_mixed_forms_raise_and_defaults_are_unchanged():
    N, L, deg, F, hub, vals, hs = CASES[0]
    rowptr, colidx, _ = host_graph(N, L, deg, 1000 + N)
    g = TypedGraph.from_csr_host(rowptr, colidx, L, DEV, edge_id_base=EBASE,
                                 self_id_base=SBASE).with_dropedge(DROPS[1])
    S = g.segments
    Xb = bf16_table((N, F), 1).to(DEV)
    dZb = bf16_table((N, S * F), 2).to(DEV)
    with pytest.raises(_lib.GrlError, match="mixed"):
        spmm_forward(Xb.float(), g, out_dtype=BF16)
    with pytest.raises(_lib.GrlError, match="mixed"):
        typed_aggregate(Xb.float(), g, out_dtype=BF16)
    with pytest.raises(_lib.GrlError, match="mixed"):
        spmm_forward_slice(Xb.float(), g, sentinel(N, S * F), 0)
    with pytest.raises(_lib.GrlError, match="mixed"):
        spmm_backward(dZb.float(), g, F, out_dtype=BF16)
    with pytest.raises(_lib.GrlError, match="mixed"):
        spmm_backward(dZb.float(), g, F, out=sentinel(N, F))
    with pytest.raises(_lib.GrlError, match="mixed"):
        spmm_backward_slice(dZb.float(), g, 0, sentinel(N, F))
    for fn in (lambda: spmm_forward(Xb, g, out_dtype=torch.float16), lambda: typed_aggregate(Xb, g, out_dtype=torch.float16),
               lambda: spmm_backward(dZb, g, F, out_dtype=torch.float16)):
        with pytest.raises(_lib.GrlError, match="out_dtype"):
            fn()
    # defaults: fp32 out of a bf16 table, fp32 dX of a bf16 dZ -- today's bits
    de = odrop(DROPS[1])
    Z = typed_aggregate(Xb, g)
    assert Z.dtype == torch.float32
    Zref = c_oracle.spmm_fwd(rowptr, colidx, Xb.float().cpu().numpy(), L, True, d=de, edge_base=EBASE, self_base=SBASE)
    assert torch.equal(bits(Z), bits(Zref))
    dX = spmm_backward(dZb, g, F)
    assert dX.dtype == torch.float32
    colptr, zrow, eid, cvals = c_oracle.csr_to_csc(rowptr, colidx, L, N, True, None)
    dXref = c_oracle.spmm_bwd(colptr, zrow, eid, dZb.float().cpu().numpy(), L, F, N, True, cvals, d=de, edge_base=EBASE,
                              self_base=SBASE)
    assert torch.equal(bits(dX), bits(dXref))
