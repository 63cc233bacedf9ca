"""TEST INFRASTRUCTURE ONLY.  Designed graphs for the typed SpMM family.

The gather kernels of csrc/spmm.hip (spmm_kernel, spmm_pair_kernel,
spmm_bf16_kernel, spmm_bf16_pair_kernel) walk ONE list per row: the row's
typed segments one after the other, loaded 64 entries at a time from the
row's first entry, dropped entries removed by a ballot, survivors issued U at
a time (2 U as lane-half pairs in the pair kernels), finished segments
flushed by a wave-uniform `while (e >= seg_end)`.  Rows above the split
threshold become chunk items and an ordered fixup.  A uniform random graph
meets the edges of that logic only by accident; pattern_graph() places them
on purpose and census() counts, from the arrays alone, how often each one
occurs -- so a test can assert that its graph is not vacuous before anything
runs on a GPU.  numpy only, host CSR.
"""
from __future__ import annotations

import numpy as np

from oracle import hash as ohash

LOAD = 64  # list entries per load (one per lane)
U = 8      # survivors issued together (GRL_SPMM_U; the pair kernels issue 2 U)

# What tests/test_gpu_spmm_structure.py runs and tests/test_spmm_patterns.py takes the census of.
SEED = 8
SHAPES = {"A": (600, 6, True), "B": (1101, 7, False)}  # name: N, L, has_self
EDGE_ID_BASE, SELF_ID_BASE = 1234, 10 ** 9 + 7
SPLIT = (64, 24)  # (threshold, chunk) of the split tests; the default (2048, 1024) splits nothing here
# DropEdge variants as (p, seed, call, drop_self), chosen on the CPU so that the census holds.  high_p:
# p^64 = 0.14, so the 300-entry hub lists (five loads) have loads without a kept entry.
VARIANTS = {"drop03": (0.3, 7, 1, True), "high_p": (0.97, 11, 0, False), "all_self": (1.0, 5, 0, True),
            "all_spare_self": (1.0, 5, 0, False)}
HUB_COLUMN_ROWS = 70


def recipes(L: int) -> dict:
    """name -> {type: edges}.  U = 8 below."""
    assert L >= 6
    return {
        "empty": {},
        "one": {0: 1},
        "lead": {L - 1: 70},                    # leading empty segments, a 6-entry tail load
        "b64": {0: 64, 2: 128},                 # segment ends on load boundaries, an empty type between; 192
        "each1": {t: 1 for t in range(L)},
        "b63": {0: 63, 1: 2},                   # a segment boundary at lane 63; a pair that straddles it
        "t65": {0: 64, 1: 1},                   # one-entry tail load
        "k8": {1: U}, "k9": {2: U + 1}, "k16": {3: 2 * U}, "k17": {4: 2 * U + 1},
        "th64": {0: 24, 2: 25, 3: 15},          # total 64: not heavy at split (64, 24)
        "th65": {0: 24, 2: 25, 3: 15, 5: 1},    # total 65: heavy; one full chunk, 0, a chunk + 1, 15, 0, 1
        "c48": {0: 48, 1: 48},                  # heavy, whole chunks only
        "hub": {3: 300},                        # five loads; heavy at (64, 24), not at the default split
    }


def placements(N: int, L: int) -> dict:
    """name -> [row at rows 0 onwards, row in mid-graph, row among the last
    rows].  Row 0 is `hub` and the graph's last row is `c48` (both heavy at
    SPLIT); the mid class starts at row N // 2.  Also "hub_columns": the three
    (column, type) that HUB_COLUMN_ROWS unpatterned rows name."""
    names = list(recipes(L))
    n = len(names)
    assert N >= 4 * n + 3 * HUB_COLUMN_ROWS and N > 300
    first = names[names.index("hub"):] + names[:names.index("hub")]
    last = names[names.index("c48") + 1:] + names[:names.index("c48") + 1]
    at = {name: [first.index(name), N // 2 + names.index(name), N - n + last.index(name)] for name in names}
    at["hub_columns"] = [(0, 0), (N - 1, L - 1), (N // 3, 2)]
    return at


def pattern_graph(N: int, L: int, seed: int):
    """(rowptr, colidx, place): a thin uniform base (average degree 3) whose
    pattern rows are overwritten whole by the recipes, each at three position
    classes (placements()), plus three hub columns -- column 0, column N - 1 and
    a mid column -- named by 70 unpatterned rows each in one type and by nothing
    else.  Every segment sorted and unique."""
    rng = np.random.default_rng(seed)
    rec, at = recipes(L), placements(N, L)
    rowptr, colidx = ohash.synth_csr(0, L, N, 3 * N, seed)
    seg = np.repeat(np.arange(N * L, dtype=np.int64), np.diff(rowptr))
    src, typ, dst = seg // L, seg % L, colidx.astype(np.int64)
    patterned = np.zeros(N, dtype=bool)
    for name in rec:
        patterned[at[name]] = True
    hub_cols = np.array([c for c, _ in at["hub_columns"]])
    keep = ~patterned[src] & ~np.isin(dst, hub_cols)
    S, T, D = [src[keep]], [typ[keep]], [dst[keep]]
    allowed = np.setdiff1d(np.arange(N), hub_cols)

    def put(rows, t, cols):
        rows, cols = np.broadcast_arrays(np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64))
        S.append(rows.ravel()), T.append(np.full(rows.size, t, dtype=np.int64)), D.append(cols.ravel())

    for name, edges in rec.items():
        for row in at[name]:
            for t, k in edges.items():
                put(row, t, rng.choice(allowed, size=k, replace=False))
    free = rng.permutation(np.nonzero(~patterned)[0])
    for i, (col, t) in enumerate(at["hub_columns"]):
        put(free[i * HUB_COLUMN_ROWS:(i + 1) * HUB_COLUMN_ROWS], t, col)
    src, typ, dst = (np.concatenate(a) for a in (S, T, D))
    keys = np.unique((src * L + typ) * N + dst)
    colidx = (keys % N).astype(np.int32)
    rowptr = np.searchsorted(keys // N, np.arange(N * L + 1), side="left").astype(np.int32)
    return rowptr, colidx, at


def csc_host(rowptr, colidx, ncols: int):
    """(colptr, eid): the CSC the backward walks -- one segment per column, its
    entries in forward-CSR order; eid[e] = entry e's forward CSR position (its
    DropEdge id minus edge_id_base)."""
    eid = np.argsort(np.asarray(colidx, dtype=np.int64), kind="stable")
    colptr = np.searchsorted(np.asarray(colidx, dtype=np.int64)[eid], np.arange(ncols + 1), side="left")
    return colptr.astype(np.int32), eid.astype(np.int32)


def edge_values(ptr, nseg: int, seed: int) -> np.ndarray:
    """Edge values in (0.1, 2) with a few exact zeros, one of them on lane 63
    of the first load of the first row that has one.  X is finite, so skipping
    a zero-weight entry and adding it are the same bits."""
    ptr = np.asarray(ptr, dtype=np.int64)
    rng = np.random.default_rng(seed)
    E = int(ptr[-1])
    v = rng.uniform(0.1, 2.0, E).astype(np.float32)
    v[rng.choice(E, 12, replace=False)] = 0.0
    tot = ptr[nseg::nseg] - ptr[:-1:nseg]
    v[ptr[int(np.argmax(tot >= LOAD)) * nseg] + LOAD - 1] = 0.0
    return v


CENSUS_WALK = ("total_multiple_of_64", "segment_end_on_load_boundary", "one_entry_tail_load",
               "leading_empty_segments", "two_or_more_segments_flushed_at_once", "load_without_kept_then_kept",
               "kept_in_load_exactly_U", "kept_in_load_exactly_2U", "kept_in_load_odd", "pair_straddles_segments",
               "segment_all_dropped_between_kept", "row_all_dropped")
CENSUS_SPLIT = ("total_equals_threshold", "total_equals_threshold_plus_1", "heavy_row_empty_segment",
                "segment_multiple_of_chunk", "one_entry_chunk", "chunk_all_dropped", "heavy_first_row",
                "heavy_last_row", "heavy_segments", "chunks")


def census(ptr, nseg: int, rows: int, kept, U: int = U, split=None) -> dict:
    """Counts of the conditions the row walk branches on, from the arrays
    alone.  ptr: rows * nseg + 1 segment pointers (forward: rowptr, nseg = L;
    backward: colptr, nseg = 1); kept[e]: entry e survives the ballot (DropEdge
    keeps it and its value is not zero).  The walk is cut as the kernels cut
    it: loads of 64 from the row's first entry, the kept entries of a load
    issued in order, the 2i-th and (2i+1)-th as a pair.  split = (threshold,
    chunk): rows with more than `threshold` entries are not walked (they are
    chunk items); the split counts, with the exact heavy_segments and chunks
    of the plan, are added."""
    ptr = np.asarray(ptr, dtype=np.int64)
    kept = np.asarray(kept, dtype=bool)
    assert ptr.size == rows * nseg + 1 and kept.size == ptr[-1]
    c = dict.fromkeys(CENSUS_WALK + (CENSUS_SPLIT if split is not None else ()), 0)
    for r in range(rows):
        p = ptr[r * nseg:(r + 1) * nseg + 1]
        lens = np.diff(p)
        total = int(p[-1] - p[0])
        if split is not None:
            thr, chunk = split
            c["total_equals_threshold"] += total == thr
            c["total_equals_threshold_plus_1"] += total == thr + 1
            if total > thr:
                c["heavy_segments"] += nseg
                c["chunks"] += int((-(-lens // chunk)).sum())
                c["heavy_row_empty_segment"] += int((lens == 0).sum())
                c["segment_multiple_of_chunk"] += int(((lens > 0) & (lens % chunk == 0)).sum())
                c["one_entry_chunk"] += int((lens % chunk == 1).sum())
                for t in range(nseg):
                    for e in range(p[t], p[t + 1], chunk):
                        c["chunk_all_dropped"] += not kept[e:min(e + chunk, p[t + 1])].any()
                c["heavy_first_row"] += r == 0
                c["heavy_last_row"] += r == rows - 1
                continue
        if total == 0:
            continue
        k = kept[p[0]:p[-1]]
        seg = np.repeat(np.arange(nseg), lens)
        c["total_multiple_of_64"] += total % LOAD == 0
        ends = p[1:-1] - p[0]  # ends of the segments before the last
        c["segment_end_on_load_boundary"] += int(((ends > 0) & (ends < total) & (ends % LOAD == 0)
                                                  & (lens[:-1] > 0)).sum())
        c["one_entry_tail_load"] += total > LOAD and total % LOAD == 1
        c["leading_empty_segments"] += nseg > 1 and lens[0] == 0
        c["row_all_dropped"] += not k.any()
        kseg = seg[k]  # segments of the kept entries, in walk order
        c["two_or_more_segments_flushed_at_once"] += int((np.diff(np.concatenate([[0], kseg])) >= 2).sum())
        khas = np.bincount(kseg, minlength=nseg) > 0
        if khas.any():
            lo, hi = np.nonzero(khas)[0][[0, -1]]
            c["segment_all_dropped_between_kept"] += int(((lens > 0) & ~khas)[lo:hi].sum())
        per_load = np.add.reduceat(k.astype(np.int64), np.arange(0, total, LOAD))
        live = np.nonzero(per_load)[0]
        if live.size:
            c["load_without_kept_then_kept"] += int((per_load[:live[-1]] == 0).sum())
        c["kept_in_load_exactly_U"] += int((per_load == U).sum())
        c["kept_in_load_exactly_2U"] += int((per_load == 2 * U).sum())
        c["kept_in_load_odd"] += int((per_load % 2 == 1).sum())
        for i0 in range(0, total, LOAD):
            ks = seg[i0:i0 + LOAD][k[i0:i0 + LOAD]]
            n2 = ks.size // 2 * 2
            c["pair_straddles_segments"] += int((ks[0:n2:2] != ks[1:n2:2]).sum())
    return {name: int(v) for name, v in c.items()}
