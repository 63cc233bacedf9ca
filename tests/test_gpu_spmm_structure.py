"""GPU: the typed SpMM family of csrc/spmm.hip on DESIGNED graphs.

Every other GPU test of these kernels walks uniform random graphs, one hub
row or R-MAT graphs; here the graph is tests/spmm_patterns.py's: row totals
of exactly 64, 65 and 192, segment ends on load boundaries and at lane 63,
leading and interleaved empty segments, segments of exactly U, U + 1, 2 U and
2 U + 1 entries, rows of exactly `threshold` and `threshold + 1` entries,
heavy rows with empty segments, heavy first and last rows, and DropEdge draws
that empty segments, loads, chunks or everything (tests/test_spmm_patterns.py
proves on the CPU that each of these occurs).  Each shape runs on P and on its
transpose PT, so every row pattern is also a CSC column pattern of the
backward.  The reference is the CPU oracle: one fmaf per kept entry in CSR /
CSC order, with split = (threshold, chunk) the chunk order restated -- every
comparison is BITWISE.

No query tells which kernel ran, so the forms are selected by what the
launchers read (pick_shape, launch_spmm, launch_spmm_bf16):
  fp32: float4 lanes when X and Z (backward: dZ and dX) are 16 B-aligned and
    the row strides, F and the segment stride are multiples of 4.  Then
    F <= 128 is the pair kernel (not the accumulating backward), F in
    (256, 512] with the path option spmm_wide = 1 is NV 2 / U 4, and anything
    else is VEC 4 / NV 1 / U 8 over ceil(F / 256) column blocks (F = 512 with
    spmm_wide = 0: two).  Otherwise one float a lane with NV = 1 (F <= 64),
    2 (F <= 128) or 4: F = 10, 70, 130, and F = 128 read from a view that
    starts 4 B into an allocation;
  bf16: eight columns a lane when X and Z are 16 B-aligned, ldx % 8 == 0,
    F % 8 == 0 and Z's strides are multiples of 4: F <= 256 the pair kernel,
    else one row per instruction in 512-column blocks.  Otherwise one bf16 a
    lane with the same NV rule: F = 100 (NV 2) and F = 10 (NV 1).
Every forward output buffer is filled with a sentinel first, so a store that
does not happen (an empty segment, a heavy segment without chunks) shows."""
import functools

import numpy as np
import pytest
import torch

import graph_patterns as gp
import spmm_patterns as sp
from grl import DropEdge, EdgeBlockedGraph, TypedGraph
from grl.ops import (spmm_backward, spmm_backward_slice, spmm_forward, spmm_forward_slice, typed_aggregate)
from oracle import c_oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SENTINEL = -7.0
EBASE, SBASE = sp.EDGE_ID_BASE, sp.SELF_ID_BASE

DROPS = {"none": None, "vals": None, **{k: DropEdge(*v) for k, v in sp.VARIANTS.items()}}
GRID = [("A", v) for v in DROPS] + [("B", v) for v in ("none", "drop03", "vals")]
SIDES = ["P", "PT"]
# name: F, spmm_wide option (None: untouched), first column of the view in a wider allocation (None: own tensor)
FORMS_F32 = {"vec4_nv1": (256, None, None), "vec4_nv2": (512, 1, None), "two_blocks": (512, 0, None),
             "pair128": (128, None, None), "pair16": (16, None, None), "scalar_nv1": (10, None, None),
             "scalar_nv2": (70, None, None), "scalar_nv4": (130, None, None), "scalar_by_alignment": (128, None, 1)}
FORMS_BF16 = {"pair": (256, None, None), "row512": (512, None, None), "scalar_nv2": (100, None, None),
              "scalar_nv1": (10, None, None)}
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
        self.X = rng.standard_normal((N, XCOLS)).astype(np.float32)
        self.Xb = torch.from_numpy(self.X).to(BF16)          # the bf16 table and its exact widening
        self.Xw = self.Xb.float().numpy()
        self.dZ = rng.standard_normal((N, self.S, 512)).astype(np.float32)
        self.csc = c_oracle.csr_to_csc(rp, ci, L, N, hs, None)
        self.csc_vals = c_oracle.csr_to_csc(rp, ci, L, N, hs, self.vals)
        self.lens = np.diff(rp).reshape(N, L)

    def graph(self, variant, split=None, edge_id_base=EBASE, self_id_base=SBASE):
        g = TypedGraph.from_csr_host(self.rowptr, self.colidx, self.L, DEV, has_self=self.has_self,
                                     vals=self.vals if variant == "vals" else None, edge_id_base=edge_id_base,
                                     self_id_base=self_id_base).with_dropedge(DROPS[variant])
        if split is not None:
            g.split_threshold, g.split_chunk = split
        return g

    def columns(self, table, F, col0):
        return np.ascontiguousarray(table[:, (col0 or 0):(col0 or 0) + F])

    def dz(self, F):
        return np.ascontiguousarray(self.dZ[:, :, :F]).reshape(self.N, self.S * F)


@functools.lru_cache(maxsize=4)
def _case(shape, side):
    return Case(shape, side)


def _odrop(variant):
    de = DROPS[variant]
    return None if de is None else c_oracle.drop(de.p, de.seed, de.call, de.drop_self)


@functools.lru_cache(maxsize=64)
def _oracle_fwd(shape, side, variant, split, table, F, col0):
    """The CPU oracle's Z, computed once per (shape, side, variant, split, table columns)."""
    c = _case(shape, side)
    X = c.columns(c.X if table == "f32" else c.Xw, F, col0)
    Z = c_oracle.spmm_fwd(c.rowptr, c.colidx, X, c.L, c.has_self, vals=c.vals if variant == "vals" else None,
                          d=_odrop(variant), edge_base=EBASE, self_base=SBASE, split=split)
    Z.setflags(write=False)
    return Z


@functools.lru_cache(maxsize=64)
def _oracle_bwd(shape, side, variant, split, F):
    c = _case(shape, side)
    colptr, zrow, eid, cvals = c.csc_vals if variant == "vals" else c.csc
    dX = c_oracle.spmm_bwd(colptr, zrow, eid, c.dz(F), c.L, F, c.N, c.has_self, cvals, d=_odrop(variant),
                           edge_base=EBASE, self_base=SBASE, split=split)
    dX.setflags(write=False)
    return dX


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _table(c, table, F, col0):
    """The device table of a form: its own tensor, or columns [col0, col0 + F)
    of a wider allocation (a view that starts col0 elements in)."""
    src = c.X if table == "f32" else c.Xb
    if col0 is None:
        t = torch.as_tensor(src[:, :F]).contiguous().to(DEV)
        assert t.data_ptr() % 16 == 0
        return t
    wide = torch.as_tensor(src[:, :col0 + F + 3]).contiguous().to(DEV)
    t = wide[:, col0:col0 + F]
    assert t.data_ptr() % 16 != 0 and t.stride(0) == col0 + F + 3
    return t


def _bits(t):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.array(t))  # (a copy: the cached oracle arrays are read-only)
    return t.detach().cpu().contiguous().view(torch.int32)


def _assert_bitwise(got, ref, what):
    got, ref = _bits(got), _bits(ref)
    assert got.shape == ref.shape, what
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {bad[0].tolist()}")


def _run_forms(shape, side, variant, split, grl_option):
    """Every form forward (into a sentinel-filled Z) and every fp32 form backward
    (autograd and spmm_backward) against the oracle; returns how many ran."""
    c = _case(shape, side)
    g = c.graph(variant, split)
    ran = 0
    for table, forms in (("f32", FORMS_F32), ("bf16", FORMS_BF16)):
        for name, (F, wide, col0) in forms.items():
            what = f"{shape} {side} {variant} split={split} {table} {name} F={F}"
            if wide is not None:
                grl_option("spmm_wide", wide)
            X = _table(c, table, F, col0)
            Z = torch.full((c.N, c.S * F), SENTINEL, device=DEV)
            spmm_forward(X, g, out=Z)
            Zref = _oracle_fwd(shape, side, variant, split, table, F, col0)
            _assert_bitwise(Z, Zref, what + " forward")
            ran += 1
            if table == "bf16":
                continue
            Xt = X.detach().requires_grad_(True)
            Za = typed_aggregate(Xt, g)
            _assert_bitwise(Za, Zref, what + " typed_aggregate")
            dZ = _dev(c.dz(F))
            Za.backward(dZ)
            dXref = _oracle_bwd(shape, side, variant, split, F)
            _assert_bitwise(Xt.grad, dXref, what + " typed_aggregate backward")
            _assert_bitwise(spmm_backward(dZ, g, F), dXref, what + " spmm_backward")
            ran += 1
    return g, ran


# ------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("shape,variant", GRID)
def test_default_split_every_form_is_the_oracle(shape, variant, side, grl_option):
    """(a) Nothing is heavy on the default split: every kernel form walks whole
    rows (forward) and whole columns (backward), bitwise the oracle."""
    g, ran = _run_forms(shape, side, variant, None, grl_option)
    assert g.split_stats() == {"csr": {"heavy_segments": 0, "chunks": 0}, "csc": {"heavy_segments": 0, "chunks": 0}}
    assert ran == len(FORMS_F32) * 2 + len(FORMS_BF16)


# ------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("shape,variant", GRID)
def test_split_every_form_is_the_oracle_in_chunk_order(shape, variant, side, grl_option):
    """(b) split (64, 24): the plan is the census's, every form is bitwise the
    oracle restating the chunk order, a heavy row's empty segments are exactly
    zero (a fixup with c_begin == c_end) and a row of exactly `threshold`
    entries is walked whole."""
    c = _case(shape, side)
    N, L, S, hs = c.N, c.L, c.S, int(c.has_self)
    g, ran = _run_forms(shape, side, variant, sp.SPLIT, grl_option)
    assert ran == len(FORMS_F32) * 2 + len(FORMS_BF16)
    ones = np.ones(c.colidx.size, dtype=bool)
    cf = sp.census(c.rowptr, L, N, ones, sp.U, sp.SPLIT)
    cb = sp.census(c.csc[0], 1, N, ones, sp.U, sp.SPLIT)
    assert cf["heavy_segments"] > 0 and cb["heavy_segments"] > 0
    assert g.split_stats() == {"csr": {"heavy_segments": cf["heavy_segments"], "chunks": cf["chunks"]},
                               "csc": {"heavy_segments": cb["heavy_segments"], "chunks": cb["chunks"]}}
    heavy = c.lens.sum(1) > sp.SPLIT[0]
    rows, types = np.nonzero(heavy[:, None] & (c.lens == 0))
    assert rows.size > 0
    if side == "P":
        for r in c.at["th65"]:
            assert heavy[r] and types[rows == r].tolist() == [t for t in range(L) if t not in sp.recipes(L)["th65"]]
    exact = [r for r in range(N) if c.lens[r].sum() == sp.SPLIT[0]]
    assert (side == "PT") or set(c.at["th64"]) <= set(exact)
    for table, F in (("f32", 256), ("f32", 10), ("bf16", 256), ("bf16", 10)):
        X = _table(c, table, F, None)
        Z = torch.full((N, S * F), SENTINEL, device=DEV)
        spmm_forward(X, g, out=Z)
        Z3 = _bits(Z).view(N, S, F)
        empty = Z3[torch.from_numpy(rows), torch.from_numpy(hs + types)]
        assert not bool(empty.any()), f"{table} F={F}: an empty segment of a heavy row is not exactly zero"
        whole = _oracle_fwd(shape, side, variant, None, table, F, None)
        if exact:
            _assert_bitwise(Z[exact], whole[exact], f"{table} F={F}: rows of exactly {sp.SPLIT[0]} entries")


# ------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("variant", ["none", "drop03"])
@pytest.mark.parametrize("table", ["f32", "bf16"])
@pytest.mark.parametrize("col0,F", [(64, 128), (3, 5), (8, 184)])
def test_split_forward_slice_into_a_wider_out(col0, F, table, variant):
    """(c) spmm_forward_slice on the heavy graph: the slice's table is a view
    of the whole-width one, out is whole-width and sentinel-filled (zseg > F,
    so the fixup and the empty-segment stores stride by zseg); the columns
    written are bitwise the whole-width result's, the others untouched."""
    c = _case("A", "P")
    g = c.graph(variant, sp.SPLIT)
    N, S, Ft = c.N, c.S, 192
    Xd = _table(c, table, Ft, None)
    whole = torch.full((N, S * Ft), SENTINEL, device=DEV)
    spmm_forward(Xd, g, out=whole)
    _assert_bitwise(whole, _oracle_fwd("A", "P", variant, sp.SPLIT, table, Ft, None), "whole width")
    out = torch.full((N, S * Ft), SENTINEL, device=DEV)
    spmm_forward_slice(Xd[:, col0:col0 + F], g, out, col0)
    out, whole = out.view(N, S, Ft), whole.view(N, S, Ft)
    _assert_bitwise(out[:, :, col0:col0 + F], whole[:, :, col0:col0 + F], "slice columns")
    assert bool((out[:, :, :col0] == SENTINEL).all()) and bool((out[:, :, col0 + F:] == SENTINEL).all())


@pytest.mark.parametrize("variant", ["none", "drop03", "vals"])
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("col0,F", [(64, 128), (3, 5), (8, 184)])
def test_split_backward_slice_from_a_column_offset(col0, F, side, variant):
    """(c) spmm_backward_slice with col0 > 0 on the heavy graph: dZ segments
    Ft wide, dX columns [col0, col0 + F) into a strided out; bitwise the
    whole-width gradient's columns (col0 = 3: dZ + col0 is not 16 B-aligned,
    the scalar form by alignment in the backward)."""
    c = _case("A", side)
    g = c.graph(variant, sp.SPLIT)
    N, Ft = c.N, 192
    dZ = _dev(c.dz(Ft))
    whole = spmm_backward(dZ, g, Ft)
    _assert_bitwise(whole, _oracle_bwd("A", side, variant, sp.SPLIT, Ft), "whole width")
    buf = torch.full((N, F + 4), SENTINEL, device=DEV)
    spmm_backward_slice(dZ, g, col0, buf[:, :F])
    _assert_bitwise(buf[:, :F], whole[:, col0:col0 + F], "slice columns")
    assert bool((buf[:, F:] == SENTINEL).all())


# ------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("variant", ["none", "drop03", "vals"])
@pytest.mark.parametrize("shape", sorted(sp.SHAPES))
def test_rows_view_from_b64_to_t65(shape, variant):
    """(d) rows_view on the default split, cut so that the view's first row is
    a b64 row and its last a t65 row: bitwise the whole result's rows."""
    c = _case(shape, "P")
    r0, r1 = c.at["b64"][0], c.at["t65"][1] + 1
    assert c.lens[r0].tolist()[:3] == [64, 0, 128] and c.lens[r1 - 1].tolist()[:2] == [64, 1] and r1 - r0 > c.N // 3
    g = c.graph(variant)
    for table, F in (("f32", 256), ("f32", 512), ("f32", 16), ("f32", 10), ("bf16", 256), ("bf16", 512), ("bf16", 10)):
        X = _table(c, table, F, None)
        Z = spmm_forward(X, g)
        _assert_bitwise(Z, _oracle_fwd(shape, "P", variant, None, table, F, None), f"{table} F={F} whole")
        out = torch.full((r1 - r0, c.S * F), SENTINEL, device=DEV)
        spmm_forward(X, g.rows_view(r0, r1), out=out)
        _assert_bitwise(out, Z[r0:r1], f"{table} F={F} rows [{r0}, {r1})")


# ------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("variant", ["none", "drop03"])
@pytest.mark.parametrize("side", SIDES)
def test_edge_blocks_equal_one_csr(side, variant):
    """(e) EdgeBlockedGraph.from_csr64 over the pattern graph in blocks of at
    most 400 edges: block bounds fall inside each class of pattern rows, the
    forward runs block by block (the slice entry with self rows at the block's
    first row) and the backward continues each column's sum from block to
    block (grl_typed_spmm_bwd_accum); both bitwise the one-CSR result, for an
    fp32 and a bf16 table."""
    c = _case("A", side)
    N, L = c.N, c.L
    g = c.graph(variant, edge_id_base=0, self_id_base=None)
    gb = EdgeBlockedGraph.from_csr64(_dev(c.rowptr.astype(np.int64)), _dev(c.colidx), L, max_block_edges=400)
    gb = gb.with_dropedge(DROPS[variant])
    bounds = np.array(gb.row_bounds)
    assert len(gb.blocks) > 8 and all(b.nnz <= 400 for b in gb.blocks)
    if side == "P":  # a bound strictly inside each class of pattern rows
        n = len(sp.recipes(L))
        for lo in (0, N // 2, N - n):
            assert np.any((bounds > lo) & (bounds < lo + n)), (lo, bounds)
    for F in (256, 128, 10):
        X = _table(c, "f32", F, None)
        Z = spmm_forward(X, g)
        if variant == "none":  # (with DropEdge the ids differ from the oracle cache's: blocks count edges from 0)
            _assert_bitwise(Z, _oracle_fwd("A", side, variant, None, "f32", F, None), f"F={F} one CSR vs oracle")
        out = torch.full((N, c.S * F), SENTINEL, device=DEV)
        spmm_forward(X, gb, out=out)
        _assert_bitwise(out, Z, f"F={F} blocked forward")
        dZ = _dev(c.dz(F))
        dX = spmm_backward(dZ, g, F)
        _assert_bitwise(spmm_backward(dZ, gb, F), dX, f"F={F} blocked backward")
        if F == 10:
            continue
        Xb = _table(c, "bf16", F, None).requires_grad_(True)
        Zb = typed_aggregate(Xb, gb)
        _assert_bitwise(Zb, spmm_forward(Xb.detach().float(), g), f"F={F} blocked bf16 forward")
        Zb.backward(dZ)
        assert Xb.grad.dtype == BF16
        assert torch.equal(Xb.grad.view(torch.int16), dX.to(BF16).view(torch.int16)), f"F={F} blocked bf16 backward"
