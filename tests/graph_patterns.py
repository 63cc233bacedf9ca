"""TEST INFRASTRUCTURE ONLY.  Designed graphs for the one-kernel GraphConv.

The gather role of graphconv_ws_body.inc walks, per 8-row group and edge
type, ONE list: the eight rows' edges concatenated, fetched 64 entries at a
time, dropped entries removed by a ballot, row ends found by comparing the
running position with the rows' inclusive prefix counts.  A uniform random
graph meets the edges of that logic only by accident; pattern_graph() places
them on purpose, and census() counts, from the arrays and the kernel's
geometry alone, how often each one occurs -- so a test can assert that its
graph is not vacuous before anything runs on a GPU.  numpy only, host CSR.
"""
from __future__ import annotations

import numpy as np

from oracle import hash as ohash

GR = 8        # rows per gather group (graphconv_ws_body.inc: GR)
FETCH = 64    # list entries per fetch (one per lane)
TILE = 64     # rows per tile (WS_R)
HEAVY = 2048  # grl.graph.SPLIT_THRESHOLD: a row with more edges over all types is split, and the layer
#               then runs as two kernels

PATTERNS = ("P0", "P1", "P2", "P3", "P4", "P5", "P6", "P7", "P8")
QUIET_GROUP = 900   # the 8 node ids of this group appear in no colidx (P8: an all-empty group of the transpose)
EMPTY_TILE = 60     # a whole tile of P0; the next tile's first row is populated

# What the GPU tests (tests/test_gpu_graphconv_structure.py) run and tests/test_graph_patterns.py takes the
# census of: the graph seed, the (N, L) of the shapes, and the DropEdge variants as (p, seed, call, drop_self),
# chosen on the CPU so that the census holds.  HIGH_P: p^64 = 0.14, so a 2048-entry list (32 fetches) has about
# 4 fetch blocks without a kept entry.
SEED = 1
SHAPES_NL = [(17_473, 6), (17_529, 6), (17_473, 7)]
HIGH_P = (0.97, 11, 0, False)
VARIANTS = {"drop03": (0.3, 7, 1, True), "high_p": HIGH_P, "all_self": (1.0, 5, 0, True),
            "all_spare_self": (1.0, 5, 0, False)}


def placements(N: int) -> dict:
    """Where the patterns sit: name -> list of group indices (group g = rows
    [8 g, 8 g + 8)).  A group holds one pattern, so "rows 0-7" and "the last
    group" are classes of positions here: pattern k takes
      the first gather wave's group of tile k (tile 0, rows 0-7: P3),
      the last gather wave's group of tile 10 + k,
      an even and an odd group in mid-graph (tiles 120 + k, 140 + k: with
        C > 256 a gather wave owns both groups of such a pair and prefetches
        the next list in another branch for each),
      one of the nine last full groups (the group after them has the graph's
        last valid row alone, N % 8 == 1, which carries its own pattern)."""
    assert N % GR == 1 and N >= TILE * 160
    last_full = N // GR - 1
    order = PATTERNS[3:] + PATTERNS[:3]  # tile 0 / rows 0-7 get P3
    at = {p: [] for p in PATTERNS}
    for k, p in enumerate(order):
        at[p] += [8 * k, 8 * (10 + k) + 7, 8 * (120 + k) + 2, 8 * (140 + k) + 3, last_full - 8 + k]
    at["P0"] += list(range(8 * EMPTY_TILE, 8 * EMPTY_TILE + 8))
    at["P5_rows"] = [g * GR + (i % GR) for i, g in enumerate(at["P5"])]  # the 2048-edge row of each P5 group
    at["P6_rows"] = [g * GR + ((i + 3) % GR) for i, g in enumerate(at["P6"])]
    return at


def pattern_graph(N: int, L: int, seed: int):
    """(rowptr, colidx, census): a sparse uniform base (average degree 4, so
    many (group, type) lists are short or empty) with whole 8-row groups
    overwritten by the patterns P0..P8 (placements()), every column segment
    sorted and unique:
      P0  all 8 rows empty in every type (also one whole 64-row tile, and the
          next tile's first row populated)
      P1  only row 7: 1 edge of type 0 (seven leading empty rows)
      P2  only row 0: 70 edges of type L-1 (seven trailing, a second fetch)
      P3  type 0: row 0 has 64 edges, row 1 has 1 (a row end on entry 64,
          total 65); type 1: row 7 has 63; type 2: row 0 has 128, row 3 has 1
      P4  type 0: 8 edges a row (total exactly 64); type 1: 16 (exactly 128)
      P5  one row with 2048 edges of one type, seven empty (32 fetches; the
          largest row that is not heavy)
      P6  one row with 2048 edges spread over all L types, its neighbours
          with about 300 of each type
      P7  odd rows 1 edge in every type, even rows none
      P8  every row: type 0 -> column 0, type 1 -> column N-1, type 2 -> itself
    plus 8 consecutive node ids that no colidx names (QUIET_GROUP), and the
    last valid row of the graph with 65 edges of one type."""
    assert 3 <= L <= 7
    rng = np.random.default_rng(seed)
    at = placements(N)
    rowptr, colidx = ohash.synth_csr(0, L, N, 4 * N, seed)
    seg = np.repeat(np.arange(N * L, dtype=np.int64), np.diff(rowptr))
    src, typ, dst = seg // L, seg % L, colidx.astype(np.int64)
    q0 = QUIET_GROUP * GR
    cleared = np.zeros(N + GR, dtype=bool)
    for p in PATTERNS:
        for g in at[p]:
            cleared[g * GR:(g + 1) * GR] = True
    cleared[N - 1] = True
    cleared[(EMPTY_TILE + 1) * TILE] = True
    keep = ~cleared[src] & ~((dst >= q0) & (dst < q0 + GR))
    S, T, D = [src[keep]], [typ[keep]], [dst[keep]]
    allowed = np.r_[0:q0, q0 + GR:N]

    def put(row, t, cols):
        cols = np.asarray(cols, dtype=np.int64)
        S.append(np.full(cols.size, row, dtype=np.int64))
        T.append(np.full(cols.size, t, dtype=np.int64))
        D.append(cols)

    def draw(k):
        return rng.choice(allowed, size=k, replace=False)

    for g in at["P1"]:
        put(g * GR + 7, 0, draw(1))
    for g in at["P2"]:
        put(g * GR, L - 1, draw(70))
    for g in at["P3"]:
        put(g * GR, 0, draw(64)), put(g * GR + 1, 0, draw(1))
        put(g * GR + 7, 1, draw(63))
        put(g * GR, 2, draw(128)), put(g * GR + 3, 2, draw(1))
    for g in at["P4"]:
        for i in range(GR):
            put(g * GR + i, 0, draw(8)), put(g * GR + i, 1, draw(16))
    for i, (g, row) in enumerate(zip(at["P5"], at["P5_rows"])):
        put(row, i % L, draw(HEAVY))
    per = min(300, (HEAVY - 8) // L)  # a neighbour's L segments stay below the heavy threshold together
    for g, row in zip(at["P6"], at["P6_rows"]):
        for t in range(L):
            put(row, t, draw(HEAVY // L + (1 if t < HEAVY % L else 0)))
        for r in range(g * GR, (g + 1) * GR):
            if r != row:
                for t in range(L):
                    put(r, t, draw(per))
    for g in at["P7"]:
        for i in range(1, GR, 2):
            for t in range(L):
                put(g * GR + i, t, draw(1))
    for g in at["P8"]:
        for r in range(g * GR, (g + 1) * GR):
            put(r, 0, [0]), put(r, 1, [N - 1]), put(r, 2, [r])
    put((EMPTY_TILE + 1) * TILE, 0, draw(3))
    put(N - 1, 1, draw(65))
    src, typ, dst = (np.concatenate(a) for a in (S, T, D))
    keys = np.unique((src * L + typ) * N + dst)
    colidx = (keys % N).astype(np.int32)
    rowptr = np.searchsorted(keys // N, np.arange(N * L + 1), side="left").astype(np.int32)
    return rowptr, colidx, census(rowptr, colidx, L, N)


def transpose_host(rowptr, colidx, L: int, N: int, return_eid: bool = False):
    """Host CSR of the graph with every edge (n, t, m) turned into (m, t, n).
    Stable: the entries of a segment of the result stay in forward-CSR order,
    i.e. sorted by source row n.  return_eid: also the forward CSR position of
    every entry of the result (what TypedGraph.typed_transpose calls eid)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    seg = np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))
    key = np.asarray(colidx, dtype=np.int64) * L + seg % L
    order = np.argsort(key, kind="stable")
    rp = np.searchsorted(key[order], np.arange(N * L + 1), side="left").astype(np.int32)
    ci = (seg[order] // L).astype(np.int32)
    return (rp, ci, order.astype(np.int32)) if return_eid else (rp, ci)


def census(rowptr, colidx, L: int, N: int, dropedge=None) -> dict:
    """Counts of the conditions the gather role's index logic branches on,
    over the (group, type) lists of the graph as the kernel cuts it: 8-row
    groups, 64-entry fetches, 64-row tiles; the last tile's groups past N
    included.  dropedge = (p, seed, call): also the conditions that depend on
    which entries DropEdge keeps (entry e's id is its CSR position, the
    forward kernels' id with edge_id_base 0)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    tiles = -(-N // TILE)
    G = tiles * (TILE // GR)
    cnt = np.zeros((G * GR, L), dtype=np.int64)
    cnt[:N] = np.diff(rowptr).reshape(N, L)
    cnt = cnt.reshape(G, GR, L)
    incl = np.cumsum(cnt, axis=1)
    total = incl[:, GR - 1, :]
    valid = np.clip(N - np.arange(G) * GR, 0, GR)
    has = cnt > 0
    first = np.where(has.any(1), has.argmax(1), GR)            # first populated row of the list
    last = np.where(has.any(1), GR - 1 - has[:, ::-1].argmax(1), -1)
    inner = (incl[:, :GR - 1] > 0) & (incl[:, :GR - 1] % FETCH == 0) & (incl[:, :GR - 1] < total[:, None, :]) \
        & has[:, :GR - 1]
    real = (valid > 0)[:, None]
    c = {
        "lists": int(G * L),
        "total_zero": int(((total == 0) & real).sum()),
        "total_multiple_of_64": int(((total > 0) & (total % FETCH == 0)).sum()),
        "row_end_on_fetch_boundary": int(inner.any(1).sum()),
        "total_over_64": int((total > FETCH).sum()),
        "total_2048_or_more": int((total >= HEAVY).sum()),
        "seven_leading_empty_rows": int(((total > 0) & (first >= GR - 1)).sum()),
        "seven_trailing_empty_rows": int(((total > 0) & (last == 0)).sum()),
        "groups_without_valid_row": int((valid == 0).sum()),
        "groups_with_one_valid_row": int((valid == 1).sum()),
        "empty_tiles": int((cnt.reshape(tiles, -1).sum(1) == 0).sum()),
        "max_row_degree": int(cnt.sum(2).max()),
        "max_in_degree": int(np.bincount(np.asarray(colidx, dtype=np.int64), minlength=N).max()) if len(colidx) else 0,
    }
    if dropedge is None:
        return c
    p, seed, call = dropedge
    kept = ohash.dropedge_keep(p, seed, call, np.arange(len(colidx), dtype=np.uint64))
    ck = np.concatenate([[0], np.cumsum(kept)])
    kseg = np.zeros((G * GR, L), dtype=np.int64)                # kept entries per (row, type)
    kseg[:N] = (ck[rowptr[1:]] - ck[rowptr[:-1]]).reshape(N, L)
    kseg = kseg.reshape(G, GR, L)
    khas = kseg > 0
    before = np.cumsum(khas, axis=1) - khas > 0                 # a row with a kept entry earlier in the list
    after = (np.cumsum(khas[:, ::-1], axis=1) - khas[:, ::-1] > 0)[:, ::-1]
    c["row_all_dropped_between_kept_rows"] = int((has & ~khas & before & after).sum())
    c["list_all_dropped"] = int(((total > 0) & (kseg.sum(1) == 0)).sum())
    # fetch blocks: the list's entries in list order are rows' segments one after the other
    n = 0
    for g, t in zip(*np.nonzero(total > FETCH)):
        rows = np.arange(g * GR, min((g + 1) * GR, N))
        k = np.concatenate([kept[rowptr[r * L + t]:rowptr[r * L + t + 1]] for r in rows])
        blocks = np.add.reduceat(k.astype(np.int64), np.arange(0, k.size, FETCH))
        live = np.nonzero(blocks > 0)[0]
        if live.size:
            n += int((blocks[:live[-1]] == 0).sum())
    c["empty_fetch_block_then_kept_entry"] = n
    return c


def add_edge(rowptr, colidx, L: int, N: int, row: int, t: int):
    """The graph with one more edge in segment (row, t): the smallest column id
    the segment does not hold yet (outside the quiet ids)."""
    rowptr = np.asarray(rowptr, dtype=np.int32)
    e0, e1 = int(rowptr[row * L + t]), int(rowptr[row * L + t + 1])
    have = set(colidx[e0:e1].tolist()) | set(range(QUIET_GROUP * GR, QUIET_GROUP * GR + GR))
    col = next(c for c in range(N) if c not in have)
    at = e0 + int(np.searchsorted(colidx[e0:e1], col))
    rp = rowptr.copy()
    rp[row * L + t + 1:] += 1
    return rp, np.insert(colidx, at, col).astype(np.int32)
