"""CPU: the designed graphs of tests/spmm_patterns.py are what
tests/test_gpu_spmm_structure.py needs them to be, checked before anything
runs on a GPU: well formed, every recipe where placements() says, and every
condition of the row walk of csrc/spmm.hip present at least once on every
side a kernel walks -- the forward rows of P and of its transpose PT, and the
CSC columns of each for the backward -- under every DropEdge variant the GPU
file uses, on the default split and on spmm_patterns.SPLIT.

required() states which conditions can occur where; the rest cannot, or only
by accident of a draw, and are not asserted."""
import functools

import numpy as np
import pytest

import graph_patterns as gp
import spmm_patterns as sp
from oracle import c_oracle
from oracle import hash as ohash

SHAPES, VARIANTS = sp.SHAPES, sp.VARIANTS
ALL_VARIANTS = ["none", "vals"] + sorted(VARIANTS)


@functools.lru_cache(maxsize=None)
def _side(shape, side):
    """(rowptr, colidx, place, colptr, eid, vals) of P or of its transpose."""
    N, L, _ = SHAPES[shape]
    rp, ci, at = sp.pattern_graph(N, L, sp.SEED)
    if side == "PT":
        rp, ci = gp.transpose_host(rp, ci, L, N)
    colptr, eid = sp.csc_host(rp, ci, N)
    return rp, ci, at, colptr, eid, sp.edge_values(rp, L, N)


def _kept(shape, side, variant):
    """(forward, backward) ballot masks in CSR / CSC entry order.  DropEdge's
    id of CSR entry e is EDGE_ID_BASE + e on both walks (the backward reads it
    through eid), which is what the GPU file's edge_id_base gives; a zero edge
    value is dropped by the same ballot."""
    rp, ci, _, _, eid, vals = _side(shape, side)
    if variant == "none":
        k = np.ones(ci.size, dtype=bool)
    elif variant == "vals":
        k = vals != 0.0
    else:
        p, seed, call, drop_self = VARIANTS[variant]
        ids = np.arange(ci.size, dtype=np.uint64) + np.uint64(sp.EDGE_ID_BASE)
        k = ohash.dropedge_keep(p, seed, call, ids)
        mask = c_oracle.dropedge_mask(c_oracle.drop(p, seed, call, drop_self), sp.EDGE_ID_BASE, ci.size)
        assert np.array_equal(k, mask.astype(bool)), "kept is not the oracle's DropEdge mask at EDGE_ID_BASE"
    return k, k[eid]


def required(side, direction, variant, split):
    """The census conditions that must occur at least once.

    Structure (no DropEdge needed).  Forward of P: everything, the recipes put
    it there.  Forward of PT: its rows are P's columns -- the thin base and
    three hub columns of 70 entries in one type -- so only leading empty
    segments; no row total is a multiple of 64 or 64 k + 1 and no segment ends
    on a load boundary.  Backward: a CSC column is ONE segment, so no segment
    condition exists (segment end on a load boundary, leading empty segments,
    several segments flushed at once, a pair across segments, a segment
    dropped between kept ones, a heavy row's empty segment); the columns of PT
    are P's rows with their types merged, so totals of 64, 65 and 192 occur
    there, while P's own columns (70 at most) show none of them.
    On SPLIT every row over 64 entries is a chunk item and is not walked:
    a walked row is one load, which leaves a total of exactly 64.

    Kept counts.  k8 / k16 make a load's kept count exactly U / 2 U only where
    nothing is dropped, and only where the recipes are rows (forward of P) or
    columns (backward of PT); an odd count occurs wherever anything is kept.
    p = 1 shows only "all dropped".  A load without a kept entry before a kept
    one needs the high p and a list of several loads: the hub rows of P
    (forward of P, backward of PT) on the default split.  A one-entry chunk
    needs a heavy segment of 24 k + 1 entries: th65's, in the forward of P
    only.  Chunks without a kept entry need DropEdge."""
    fwd, rows_are_recipes = direction == "fwd", (side == "P") == (direction == "fwd")
    dropping = variant in VARIANTS
    p = VARIANTS[variant][0] if dropping else 0.0
    need = set()
    if rows_are_recipes:
        need |= {"total_multiple_of_64"}
        if split is None:
            need |= {"one_entry_tail_load"} | ({"segment_end_on_load_boundary"} if fwd else set())
    if fwd:
        need |= {"leading_empty_segments"}
    if p < 1.0:
        need |= {"kept_in_load_odd"} | ({"two_or_more_segments_flushed_at_once", "pair_straddles_segments"}
                                        if fwd else set())
        if not dropping and rows_are_recipes:
            need |= {"kept_in_load_exactly_U", "kept_in_load_exactly_2U"}
    if dropping:
        need |= {"row_all_dropped"}
        if p < 1.0 and fwd:
            need |= {"segment_all_dropped_between_kept"}
        if variant == "high_p" and rows_are_recipes and split is None:
            need |= {"load_without_kept_then_kept"}
    if split is not None:
        need |= {"heavy_first_row", "heavy_last_row", "heavy_segments", "chunks"}
        if fwd:
            need |= {"heavy_row_empty_segment"}
        if rows_are_recipes:
            need |= {"total_equals_threshold", "total_equals_threshold_plus_1", "segment_multiple_of_chunk"}
            if fwd:
                need |= {"one_entry_chunk"}
        if dropping and (p >= 0.9 or (fwd and side == "P")):
            need |= {"chunk_all_dropped"}
    return need


def _well_formed(rowptr, colidx, N, L):
    assert rowptr.dtype == np.int32 and colidx.dtype == np.int32
    assert rowptr.size == N * L + 1 and rowptr[0] == 0 and rowptr[-1] == colidx.size
    assert np.all(np.diff(rowptr) >= 0), "rowptr is not monotone"
    assert colidx.min() >= 0 and colidx.max() < N
    seg = np.repeat(np.arange(N * L), np.diff(rowptr))
    same = seg[1:] == seg[:-1]
    assert np.all(colidx[1:][same] > colidx[:-1][same]), "a segment is not sorted and unique"


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_pattern_graph_is_well_formed_and_holds_every_recipe(shape):
    N, L, _ = SHAPES[shape]
    rp, ci, at, colptr, eid, _ = _side(shape, "P")
    _well_formed(rp, ci, N, L)
    rpt, cit, _, colptr_t, eid_t, _ = _side(shape, "PT")
    _well_formed(rpt, cit, N, L)
    deg = np.diff(rp).reshape(N, L)
    for name, edges in sp.recipes(L).items():
        assert len(at[name]) == 3 and at[name][0] < 20 and abs(at[name][1] - N // 2) < 20 and at[name][2] >= N - 20
        for row in at[name]:
            assert deg[row].tolist() == [edges.get(t, 0) for t in range(L)], (name, row)
    assert at["hub"][0] == 0 and at["c48"][2] == N - 1  # a heavy first row and a heavy last row at SPLIT
    assert at["b64"][0] < at["t65"][1]                  # the row range of the rows_view test
    degt = np.diff(rpt).reshape(N, L)
    for col, t in at["hub_columns"]:  # named by 70 rows in one type and by nothing else
        assert degt[col].tolist() == [sp.HUB_COLUMN_ROWS if u == t else 0 for u in range(L)], col
    assert sorted(c for c, _ in at["hub_columns"])[::2] == [0, N - 1]
    # the default split leaves every row and every column whole
    assert deg.sum(1).max() == 300 and degt.sum(1).max() <= 300
    # the CSC of this module is the oracle's
    for (r, c, cp, e) in ((rp, ci, colptr, eid), (rpt, cit, colptr_t, eid_t)):
        ocp, _, oeid, _ = c_oracle.csr_to_csc(r, c, L, N, True, None)
        assert np.array_equal(ocp, cp) and np.array_equal(oeid, e)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_edge_values_hold_zeros_and_one_on_lane_63(shape):
    N, L, _ = SHAPES[shape]
    for side in ("P", "PT"):
        rp, _, _, _, _, vals = _side(shape, side)
        zeros = np.nonzero(vals == 0.0)[0]
        assert 2 <= zeros.size <= 13 and vals.min() >= 0.0 and vals.max() < 2.0
        row0 = rp[:-1:L][np.searchsorted(rp[::L], zeros, side="right") - 1]  # first entry of each zero's row
        assert np.any((zeros - row0) % sp.LOAD == sp.LOAD - 1), "no zero value on a load's lane 63"


@pytest.mark.parametrize("split", [None, sp.SPLIT], ids=["default", "split"])
@pytest.mark.parametrize("variant", ALL_VARIANTS)
@pytest.mark.parametrize("side", ["P", "PT"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_condition_occurs(shape, side, variant, split):
    N, L, _ = SHAPES[shape]
    rp, ci, at, colptr, eid, _ = _side(shape, side)
    kf, kb = _kept(shape, side, variant)
    for direction, ptr, nseg, kept in (("fwd", rp, L, kf), ("bwd", colptr, 1, kb)):
        c = sp.census(ptr, nseg, N, kept, sp.U, split)
        need = required(side, direction, variant, split)
        assert need <= set(c)
        for name in sorted(need):
            assert c[name] >= 1, f"{name} does not occur ({shape} {side} {direction} {variant} split={split}): {c}"
        populated = int((ptr[nseg::nseg] > ptr[:-1:nseg]).sum())
        heavy = c.get("heavy_segments", 0) // nseg
        if variant in VARIANTS and VARIANTS[variant][0] == 1.0:  # p = 1: all dropped and nothing else
            assert c["row_all_dropped"] == populated - heavy, f"row_all_dropped: {c}"
            for name in ("two_or_more_segments_flushed_at_once", "load_without_kept_then_kept", "kept_in_load_odd",
                         "pair_straddles_segments", "segment_all_dropped_between_kept"):
                assert c[name] == 0, f"{name} under p = 1: {c}"
            if split is not None:
                assert c["chunk_all_dropped"] == c["chunks"], f"chunk_all_dropped under p = 1: {c}"
        if variant == "none":
            assert c["row_all_dropped"] == 0 and c["load_without_kept_then_kept"] == 0, f"drops without DropEdge: {c}"
        if nseg == 1:  # one segment: no segment condition
            for name in ("segment_end_on_load_boundary", "leading_empty_segments",
                         "two_or_more_segments_flushed_at_once", "pair_straddles_segments",
                         "segment_all_dropped_between_kept", "heavy_row_empty_segment"):
                assert c.get(name, 0) == 0, f"{name} in a one-segment walk: {c}"
        if split is None:
            assert (ptr[nseg::nseg].astype(np.int64) - ptr[:-1:nseg]).max() <= 2048, "a heavy row on the default split"
        elif side == "P" and direction == "fwd":  # the plan the GPU test's split_stats() must report
            lens = np.diff(rp).reshape(N, L)
            hv = lens.sum(1) > split[0]
            assert c["heavy_segments"] == int(hv.sum()) * L
            assert c["chunks"] == int((-(-lens[hv] // split[1])).sum())
            for name in ("th65", "c48", "hub"):
                assert hv[at[name]].all(), name
            assert not hv[at["th64"]].any()
